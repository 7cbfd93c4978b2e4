"""k_search_triangulation / k_tri_geometry (sdslam_amd/csrc/track_tri.hip) on the MI355X against the numpy restatement
tests/triangulation_ref.py: the crafted cases of tests/triangulation_cases.py through the debug entry, bit for bit; the
batched path through extraction on six views of the textured surface (paired slots and the broadcast, dense and sparse
extractors, map-point flags, mvuRight mixes), fed the device's own F12 and epipole so an ulp in F12 cannot flip a gate; the
device's ComputeF12 against the float64 restatement within 64 x the restatement's own float64 / longdouble gap, measured
here on the same poses; one broadcast call + an in-order walk = CreateNewMapPoints' sequential loop; lifetime and errors.

Measured on the MI355X when this was written (printed by test_device_compute_f12): largest relative F12 deviation 0, float64 /
longdouble gap of the restatement 3.49e-14, bound 2.23e-12."""
import numpy as np
import pytest

import triangulation_cases as TC
import triangulation_ref as TR
from sdslam_amd import synth

pytestmark = pytest.mark.gpu
B, W, H = 3, 640, 480
BOUNDS = (0.0, float(W), 0.0, float(H))
RIGS = {"dense": dict(name="dense", cfg=(1000, 1.2, 8, 20), dense=True), "sparse": dict(name="sparse", cfg=(50, 1.2, 8, 20), dense=False)}
# KF2 = frame b of the ref extractor, KF1 = frame b of the cur extractor: forward motion (the epipole lies inside KF2's image),
# sideways with a small z component, sideways the other way
T_REF = [np.eye(4), synth.se3_exp((-0.05, 0.02, 0.0), (0.0, 0.3, 0.0)), synth.se3_exp((0.04, -0.06, 0.01), (0.2, 0.0, -0.3))]
MOTION = [synth.se3_exp((-0.03, -0.02, -0.25), (0.2, 0.1, -0.3)), synth.se3_exp((0.2, 0.01, 0.02), (0.3, -0.5, 0.4)),
          synth.se3_exp((-0.18, 0.03, -0.015), (-0.2, 0.4, 0.2))]
T_CUR = [MOTION[b] @ T_REF[b] for b in range(B)]
SEED = 31
_IMAGES, _RIG = {}, {}


def images():
    if not _IMAGES:
        tex = synth.make_image(SEED, 2 * W, 2 * H)
        _IMAGES["cur"] = np.stack([synth.render_plane_view(tex, T, W, H) for T in T_CUR])
        _IMAGES["ref"] = np.stack([synth.render_plane_view(tex, T, W, H) for T in T_REF])
    return _IMAGES["cur"], _IMAGES["ref"]


def scene(cfg, oracle=None, extracted=None):
    """Keypoints (the oracle's on a host without GPU: they are the device's), flags, mvuRight and the restatement's F12 / epipole
    for both pairings ([broadcast][slot])."""
    if extracted is None:
        cur, ref = images()
        ks, ds = [[], []], [[], []]
        for side, imgs in enumerate((cur, ref)):
            for b in range(B):
                k, d = oracle.OrbOracle(*cfg["cfg"]).extract(imgs[b])
                ks[side].append(k)
                ds[side].append(d)
        cap = max(len(k) for side in ks for k in side)
        n1, n2 = np.array([len(k) for k in ks[0]]), np.array([len(k) for k in ks[1]])
        pad = lambda lst, dt, tail: np.stack([np.concatenate([np.asarray(a), np.zeros((cap - len(a),) + tail, dt)]) for a in lst])
        k1, k2 = pad(ks[0], ks[0][0].dtype, ()), pad(ks[1], ks[1][0].dtype, ())
        d1, d2 = pad(ds[0], np.uint8, (32,)), pad(ds[1], np.uint8, (32,))
    else:
        k1, d1, n1, k2, d2, n2 = extracted
        cap = k1.shape[1]
    rng = np.random.default_rng(77)
    h1, h2 = (rng.random((B, cap)) < 0.5).astype(np.uint8), (rng.random((B, cap)) < 0.5).astype(np.uint8)
    u1, u2 = np.full((B, cap), -1, np.float32), np.full((B, cap), -1, np.float32)
    u1[0, rng.random(cap) < 0.2] = 100.0                      # the broadcast frame's row
    u1[2, rng.random(cap) < 0.4] = 50.0
    u2[2, rng.random(cap) < 0.4] = 0.0                        # == 0 is stereo too
    F_ref = [[TR.compute_f12(T_CUR[0 if bc else b], T_REF[b], TC.K) for b in range(B)] for bc in (0, 1)]
    epi_ref = [[TR.epipole(T_CUR[0 if bc else b], T_REF[b], TC.K) for b in range(B)] for bc in (0, 1)]
    return dict(k1=k1, d1=d1, n1=np.asarray(n1), k2=k2, d2=d2, n2=np.asarray(n2), h1=h1, h2=h2, u1=u1, u2=u2, F_ref=F_ref,
                epi_ref=epi_ref, cap=cap)


def restate(sc, b, bc, ori, F12, epi, h1=None, counts=None):
    f1 = 0 if bc else b
    n1, n2 = int(sc["n1"][f1]), int(sc["n2"][b])
    h1 = sc["h1"][b] if h1 is None else h1
    return TR.search_for_triangulation(sc["k1"][f1, :n1], sc["d1"][f1, :n1], h1[:n1], sc["u1"][f1, :n1], sc["k2"][b, :n2],
                                       sc["d2"][b, :n2], sc["h2"][b, :n2], sc["u2"][b, :n2], F12, epi, TC.SF, TC.SIGMA2, ori, counts)


@pytest.fixture(scope="module")
def sd():
    import sdslam_amd
    if sdslam_amd.device_count() < 1:
        pytest.fail("no HIP device: the gpu-marked tests need a real MI355X")
    return sdslam_amd


def rig(sd, name):
    if name not in _RIG:
        cfg = RIGS[name]
        cur, ref = sd.ORBextractor(*cfg["cfg"], W, H, B), sd.ORBextractor(*cfg["cfg"], W, H, B)
        ci, ri = images()
        k1, d1, n1 = cur.extract_batch(ci)
        k2, d2, n2 = ref.extract_batch(ri)
        trk = sd.Tracker(cur, ref, max_points=max(k1.shape[1], 8), max_batch=B, pnp_max_iterations=8)
        trk.set_camera(*TC.K, 0.0, BOUNDS)
        _RIG[name] = dict(trk=trk, cur=cur, ref=ref, sc=scene(cfg, extracted=(k1, d1, n1, k2, d2, n2)), imgs=(ci, ri), cfg=cfg)
    r = _RIG[name]
    upload(r)
    return r


def upload(r, h1=None):
    trk, sc = r["trk"], r["sc"]
    trk.set_current_broadcast(-1)
    trk.set_poses(0, T_REF, T_CUR)
    trk.set_point_flags(0, sc["h1"] if h1 is None else h1, sc["h2"])
    trk.set_uright(0, sc["u1"])
    trk.set_uright_ref(0, sc["u2"])


def raw(trk, n=B):
    g = trk.get_triangulation_matches(0, n)
    return b"".join(np.ascontiguousarray(g[k]).tobytes() for k in ("matches12", "n_matches", "F12", "epipole"))


# ------------------------------------------------------------------------------------------------ 1. the debug entry
@pytest.mark.parametrize("ori", [0, 1])
def test_debug_entry_is_bit_exact_on_every_case(sd, ori):
    from sdslam_amd import capi
    total = 0
    for c, res in TC.cases_with_reference():
        n, m = capi.debug_search_for_triangulation(c["k1"], c["d1"], c["h1"], c["u1"], c["k2"], c["d2"], c["h2"], c["u2"], c["F12"],
                                                   c["epi"], c["sf"], c["sigma2"], ori)
        want_n, want_m, _ = res[ori]
        assert n == want_n and np.array_equal(m, want_m), (c["name"], ori, n, want_n, np.flatnonzero(m != want_m)[:8])
        total += n
    assert total > 200      # the restatement's own count (242 with the rotation check, more without): not vacuous


@pytest.mark.parametrize("n1,n2", [(0, 0), (1, 3)])
def test_debug_entry_on_empty_and_unaligned_inputs(sd, n1, n2):
    """Both sides empty (the entry still launches, on a capacity of 1), and counts that are no multiple of the 16 bytes the
    entry's device arrays are carved in."""
    from sdslam_amd import capi
    c = TC.shape_case("tiny_%dx%d" % (n1, n2), 40 + n1, n1, n2, flagged=0.0)
    for ori in (0, 1):
        want_n, want_m = TC.reference(c, ori)
        n, m = capi.debug_search_for_triangulation(c["k1"], c["d1"], c["h1"], c["u1"], c["k2"], c["d2"], c["h2"], c["u2"], c["F12"],
                                                   c["epi"], c["sf"], c["sigma2"], ori)
        assert n == want_n and len(m) == n1 and np.array_equal(m, want_m), (n1, n2, ori, n, want_n, m, want_m)


# ------------------------------------------------------------------------------------------------ 2. through extraction
@pytest.mark.parametrize("name", list(RIGS))
def test_batched_path_through_extraction(sd, name):
    r = rig(sd, name)
    trk, sc, dense = r["trk"], r["sc"], r["cfg"]["dense"]
    assert (sc["n1"] > 512).all() and (sc["n2"] > 512).all() if dense else (sc["n1"] < 64).all() and (sc["n2"] < 64).all()
    fired = 0
    for bc in (False, True):
        trk.set_poses(0, T_REF, [T_CUR[0]] * B if bc else T_CUR)      # Tcur is per slot: under the broadcast every slot holds KF1's pose
        trk.set_current_broadcast(0 if bc else -1)
        try:
            for ori in (0, 1):
                trk.search_for_triangulation(B, False, ori)
                g = trk.get_triangulation_matches(0, B)
                for b in range(B):
                    counts = {}
                    n, m = restate(sc, b, bc, ori, g["F12"][b], g["epipole"][b], counts=counts)
                    n1 = int(sc["n1"][0 if bc else b])
                    assert g["n_matches"][b] == n, (name, bc, ori, b, g["n_matches"][b], n)
                    assert np.array_equal(g["matches12"][b, :n1], m) and (g["matches12"][b, n1:] == -1).all(), (name, bc, ori, b)
                    assert n >= 20 or not dense or ori, (name, bc, b, n)
                    if (bc or b == 0) and not ori:
                        fired += counts["epipole"]
        finally:
            trk.set_current_broadcast(-1)
    assert fired > 0 or not dense        # forward motion: the epipole gate rejects something


# ------------------------------------------------------------------------------------------------ 3. ComputeF12
def test_device_compute_f12(sd):
    n_rand = 64
    rng = np.random.default_rng(12)
    pairs = [(T_CUR[b], T_REF[b]) for b in range(B)] + [(T_CUR[0], T_REF[b]) for b in range(B)]
    for _ in range(n_rand):
        pairs.append((synth.se3_exp(rng.uniform(-0.5, 0.5, 3), rng.uniform(-20, 20, 3)), synth.se3_exp(rng.uniform(-0.5, 0.5, 3), rng.uniform(-20, 20, 3))))
    n = len(pairs)
    tiny = (50, 1.2, 1, 20, 64, 64)
    ext = [sd.ORBextractor(*tiny, n) for _ in range(2)]
    trk = sd.Tracker(ext[0], ext[1], max_points=8, max_batch=n, pnp_max_iterations=4)
    try:
        trk.set_camera(*TC.K, 0.0, BOUNDS)
        img = synth.make_batch(5, 2, 64, 64)[np.arange(n) % 2]
        ext[0].extract_batch(img)
        ext[1].extract_batch(img)
        trk.set_poses(0, [p[1] for p in pairs], [p[0] for p in pairs])
        trk.search_for_triangulation(n, False, False)
        g = trk.get_triangulation_matches(0, n)
        gap = worst = 0.0
        for i, (T1, T2) in enumerate(pairs):
            F64, Fl = TR.compute_f12(T1, T2, TC.K), TR.compute_f12_longdouble(T1, T2, TC.K)
            scale = float(np.abs(Fl).max())
            gap = max(gap, float(np.abs(F64.astype(np.longdouble) - Fl).max()) / scale)
        bound = 64.0 * gap
        assert 0 < bound < 1e-10
        for i, (T1, T2) in enumerate(pairs):
            F64 = TR.compute_f12(T1, T2, TC.K)
            d = float(np.abs(g["F12"][i] - F64).max() / np.abs(F64).max())
            worst = max(worst, d)
            assert d <= bound, (i, d, bound)
            assert g["epipole"][i].tobytes() == TR.epipole(T1, T2, TC.K).tobytes(), i
        print("k_tri_geometry vs float64 restatement: largest relative F12 deviation %.3e, float64/longdouble gap %.3e, bound %.3e"
              % (worst, gap, bound))
    finally:
        trk.close()
        for e in ext:
            e.close()


def test_caller_supplied_f12(sd):
    r = rig(sd, "dense")
    trk, sc = r["trk"], r["sc"]
    F = np.stack(sc["F_ref"][0][:2])
    trk.set_f12(0, F)                                          # slots 0 and 1 only: slot 2 is never covered (test_errors)
    trk.search_for_triangulation(2, True, False)
    g = trk.get_triangulation_matches(0, 2)
    assert g["F12"].tobytes() == F.tobytes()
    for b in range(2):
        n, m = restate(sc, b, False, 0, F[b], g["epipole"][b])
        assert g["n_matches"][b] == n and np.array_equal(g["matches12"][b, :sc["n1"][b]], m) and n >= 20


# ------------------------------------------------------------------------------------------------ 4. the sequential loop
def test_one_broadcast_call_equals_the_sequential_loop(sd):
    r = rig(sd, "dense")
    trk, sc = r["trk"], r["sc"]
    h1 = np.repeat(sc["h1"][:1], B, axis=0)                    # one current keyframe: the same map points in every slot
    upload(r, h1)
    trk.set_poses(0, T_REF, [T_CUR[0]] * B)
    trk.set_current_broadcast(0)
    try:
        trk.search_for_triangulation(B, False, False)
        g = trk.get_triangulation_matches(0, B)
    finally:
        trk.set_current_broadcast(-1)
    got_point = np.zeros(sc["cap"], bool)
    walked = []
    for b in range(B):
        pairs = [(i, j) for i, j in TR.pairs_of(g["matches12"][b]) if not got_point[i]]
        for i, _ in pairs:
            got_point[i] = True
        walked.append(pairs)
    n1 = int(sc["n1"][0])
    want = TR.create_new_map_points_order(lambda b, flags: restate(sc, b, True, 0, g["F12"][b], g["epipole"][b], h1=flags)[1], h1[0, :n1], B)
    assert walked == want
    assert all(len(p) >= 20 for p in want[:1]) and sum(len(p) for p in want[1:]) > 0
    assert sum(len(TR.pairs_of(g["matches12"][b])) for b in range(B)) > sum(len(p) for p in walked)   # the walk removed something


# ------------------------------------------------------------------------------------------------ 5. lifetime and errors
def test_result_survives_search_by_points_and_sim3_and_vice_versa(sd):
    r = rig(sd, "dense")
    trk, sc = r["trk"], r["sc"]
    rng = np.random.default_rng(3)
    trk.set_rand(0, rng.integers(0, 2 ** 31, size=(B, 30), dtype=np.int64).astype(np.int32))
    trk.set_sim3_points(0, rng.normal(size=(B, sc["cap"], 3)) + (0, 0, 3), rng.normal(size=(B, sc["cap"], 3)) + (0, 0, 3))
    trk.search_by_points(B, 0.75, True)
    trk.sim3(B, 0, 0.99, 20, 8, 5)
    pm, s3 = trk.get_point_matches(0, B), trk.get_sim3(0, B)
    trk.search_for_triangulation(B, False, False)
    tri = raw(trk)
    pm2, s32 = trk.get_point_matches(0, B), trk.get_sim3(0, B)
    assert np.array_equal(pm[0], pm2[0]) and np.array_equal(pm[1], pm2[1]) and pm[1].sum() > 0
    assert all(np.array_equal(np.asarray(s3[k]), np.asarray(s32[k]), equal_nan=True) for k in ("T12", "R", "t", "scale", "inliers", "info"))
    trk.sim3_iterate(B, 1)                                     # the solvers are still alive
    trk.search_by_points(B, 0.75, True)
    trk.sim3(B, 0, 0.99, 20, 8, 5)
    trk.get_sim3(0, B)
    assert raw(trk) == tri


def test_result_ends_with_its_inputs(sd):
    r = rig(sd, "dense")
    trk, sc = r["trk"], r["sc"]
    ci, ri = r["imgs"]
    ending = {
        "extraction of cur": lambda: r["cur"].extract_batch(ci),
        "extraction of ref": lambda: r["ref"].extract_batch(ri),
        "set_point_flags": lambda: trk.set_point_flags(0, sc["h1"], sc["h2"]),
        "set_poses": lambda: trk.set_poses(0, T_REF, T_CUR),
        "set_uright": lambda: trk.set_uright(0, sc["u1"]),
        "set_uright_ref": lambda: trk.set_uright_ref(0, sc["u2"]),
        "set_f12": lambda: trk.set_f12(0, np.stack(sc["F_ref"][0][:1])),
        "broadcast": lambda: trk.set_current_broadcast(0),
    }
    with pytest.raises(sd.SdError) as e:                       # upload() ended whatever there was
        trk.get_triangulation_matches(0, B)
    assert e.value.code == 1
    try:
        for name, call in ending.items():
            trk.search_for_triangulation(B, False, False)
            first = raw(trk)
            assert raw(trk) == first                           # reading does not end it
            call()
            with pytest.raises(sd.SdError) as e:
                trk.get_triangulation_matches(0, B)
            assert e.value.code == 1, name
    finally:
        trk.set_current_broadcast(-1)
    trk.search_for_triangulation(2, False, False)
    trk.get_triangulation_matches(0, 2)
    with pytest.raises(sd.SdError):                            # more slots than the search covered
        trk.get_triangulation_matches(0, B)


def test_errors(sd):
    r = rig(sd, "dense")
    trk, sc = r["trk"], r["sc"]
    with pytest.raises(sd.SdError) as e:                       # slot 2 has never been given an F12
        trk.search_for_triangulation(B, True, False)
    assert e.value.code == 1
    for n in (0, B + 1):
        with pytest.raises(sd.SdError) as e:
            trk.search_for_triangulation(n, False, False)
        assert e.value.code == 3
    with pytest.raises(sd.SdError) as e:
        trk.set_f12(B, np.zeros((1, 3, 3)))
    assert e.value.code == 3
    with pytest.raises(sd.SdError) as e:
        trk.set_uright_ref(0, np.zeros((1, sc["cap"] + 1), np.float32))
    assert e.value.code == 1
    with pytest.raises(sd.SdError) as e:
        trk.set_uright_ref(B, np.zeros((1, 4), np.float32))
    assert e.value.code == 3


def test_queued_equals_synchronised(sd):
    r = rig(sd, "dense")
    trk, sc = r["trk"], r["sc"]
    F = np.stack(sc["F_ref"][0][:2])

    def run(sync):
        upload(r)
        steps = [lambda: trk.set_f12(0, F), lambda: trk.search_for_triangulation(2, True, True),
                 lambda: trk.search_for_triangulation(B, False, False), lambda: trk.set_f12(0, F[::-1].copy()),
                 lambda: trk.search_for_triangulation(2, True, False), lambda: trk.search_for_triangulation(B, False, True)]
        for s in steps:
            s()
            if sync:
                try:
                    raw(trk, 2)
                except sd.SdError:
                    pass                                       # right after set_f12 there is no result to read
        return raw(trk)
    queued = run(False)
    assert run(True) == queued
    assert trk.get_triangulation_matches(0, B)["n_matches"].sum() > 0
