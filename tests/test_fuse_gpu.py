"""k_fuse (sdslam_amd/csrc/track_fuse.hip) on the MI355X against the numpy restatement tests/fuse_ref.py: the crafted cases of
tests/fuse_cases.py through sd_debug_fuse, bit for bit, both overloads; the batched path through extraction on views of the
textured surface (both keyframe sides, with and without the broadcast, own and shared point rows, mvuRight mixes, the Scw
overload), fed the device's keypoints and, for the Scw overload, the device's decomposed pose; the decomposition against
float64 within 64 x the restatement's own float64 / longdouble gap, measured here; the batched search + in-order walk against
the reference's sequential loops on the toy map; lifetime, errors, determinism, and the other results of the handle untouched.

Measured on the MI355X when this was written (printed by test_device_scw_decomposition): largest relative deviation of the
device's Rcw, tcw, Ow 0, float64 / longdouble gap of the restatement 1.485e-16, bound 9.505e-15.

The walk run here is the Python twin (fuse_ref.fuse_batched_walk) of the C++ facade's; the facade itself runs on the GPU in
tests/test_fuse_facade.py."""
import numpy as np
import pytest

import fuse_cases as FC
import fuse_ref as FR
import test_triangulation_gpu as TG
import triangulation_cases as TC
from sdslam_amd import synth

pytestmark = pytest.mark.gpu
B, W, H = TG.B, TG.W, TG.H
BF = 40.0
CAM9 = np.array([*TC.K, BF, 0, W, 0, H], np.float32)
RIGS = TG.RIGS
N_OWN, N_EXTRA = 500, 60                                   # keypoints that get a point, extra points that miss
MIN_FUSED = 20                                             # per slot, every rig and configuration (checked in test_fuse_cpu.py too)
SCALES = (1.7, 0.6, 2.25)
# (kf_side, broadcast, point_row, sim3)
CONFIGS = [(0, False, -1, 0), (0, False, 0, 0), (0, True, -1, 0), (0, True, 0, 0), (1, False, -1, 0), (1, False, 0, 0), (1, False, 0, 1),
           (0, True, 0, 1)]
_RIG = {}


def true_uright(kps, T):
    """mvuRight a rectified stereo rig would measure: x - bf / z of the surface point the keypoint sees from pose T."""
    R, t = T[:3, :3], T[:3, 3]
    rays = np.stack([(kps["x"].astype(np.float64) - TC.K[2]) / TC.K[0], (kps["y"].astype(np.float64) - TC.K[3]) / TC.K[1], np.ones(len(kps))], -1)
    Xw = synth.intersect_surface(-R.T @ t, rays @ R, 2.0)
    z = (Xw @ R.T + t)[:, 2]
    return (kps["x"] - BF / z).astype(np.float32)


def scene(cfg, oracle=None, extracted=None):
    """Keypoints of the cur and ref views (the oracle's on a host without GPU), mvuRight mixes (mono; stereo as a rig at bf = 40
    would measure it; a few stereo keypoints at exactly 0) and the point rows, each point one view's keypoint back-projected
    onto the surface.  Dense rig: row f = every second keypoint of cur view f (all pyramid levels) plus points that miss.
    Sparse rig (28 keypoints a view: one view cannot supply 20 fused points in another): row f = the keypoints of all six
    views, each from its own pose, so every target keyframe meets at least its own."""
    sc = TG.scene(cfg, oracle, extracted)
    views = [(sc["k1"][f, :sc["n1"][f]], sc["d1"][f, :sc["n1"][f]], TG.T_CUR[f]) for f in range(B)]
    views += [(sc["k2"][f, :sc["n2"][f]], sc["d2"][f, :sc["n2"][f]], TG.T_REF[f]) for f in range(B)]
    rows = []
    for f in range(B):
        if cfg["dense"]:
            k, d, T = views[f]
            rows.append(synth.local_map_case(100 + f, k[::2][:N_OWN], d[::2][:N_OWN], T, n_extra=N_EXTRA))
        else:
            parts = [synth.local_map_case(100 + 10 * f + v, k, d, T, n_extra=3) for v, (k, d, T) in enumerate(views)]
            rows.append({key: np.concatenate([p[key] for p in parts]) for key in parts[0]})
    rng = np.random.default_rng(5)
    cap = sc["cap"]
    ur = [np.full((B, cap), -1, np.float32), np.full((B, cap), -1, np.float32)]
    for side, (k, n, poses) in enumerate(((sc["k1"], sc["n1"], TG.T_CUR), (sc["k2"], sc["n2"], TG.T_REF))):
        for f in range(B):
            m = int(n[f])
            stereo = rng.random(m) < (0.0, 0.3, 0.6)[f]
            val = np.where(rng.random(m) < 0.1, np.float32(0.0), true_uright(k[f, :m], poses[f]))
            ur[side][f, :m] = np.where(stereo, val, np.float32(-1.0))
    sc.update(rows=rows, ur=ur, M=max(len(r["cand"]) for r in rows) + 3)
    return sc


def restate(sc, cfg, f, pose=None, counts=None):
    side, bc, prow, sim3 = cfg
    fk = 0 if (bc and side == 0) else f
    k, d, n = (sc["k2"], sc["d2"], sc["n2"]) if side else (sc["k1"], sc["d1"], sc["n1"])
    nk = int(n[fk])
    T = TG.T_REF[f] if side else TG.T_CUR[0 if bc else f]
    if sim3:
        T = T.copy()
        T[:3, :] *= SCALES[f]
    base = sc["rows"][prow if prow >= 0 else f]
    cand = sc["rows"][f]["cand"]
    n_pts = len(base["cand"])
    pts = dict(base, cand=np.concatenate([cand, np.zeros(n_pts, np.uint8)])[:n_pts])
    return FR.fuse_search(k[fk, :nk], d[fk, :nk], sc["ur"][side][fk, :nk], pts, T, CAM9, FC.SF, FC.INV_SIGMA2, FC.SCALE, 3.0, bool(sim3),
                          pose=pose, counts=counts)


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
        ci, ri = TG.images()
        k1, d1, n1 = cur.extract_batch(ci)
        k2, d2, n2 = ref.extract_batch(ri)
        sc = scene(cfg, extracted=(k1, d1, n1, k2, d2, n2))
        trk = sd.Tracker(cur, ref, max_points=sc["M"], max_batch=B, pnp_max_iterations=8)
        trk.set_camera(*TC.K, BF, TG.BOUNDS)
        _RIG[name] = dict(trk=trk, cur=cur, ref=ref, sc=sc, imgs=(ci, ri), cfg=cfg)
    return _RIG[name]


def upload(r, cfg):
    side, bc, prow, sim3 = cfg
    trk, sc = r["trk"], r["sc"]
    trk.set_current_broadcast(-1)
    trk.set_poses(0, TG.T_REF, [TG.T_CUR[0]] * B if bc else TG.T_CUR)
    trk.set_uright(0, sc["ur"][0])
    trk.set_uright_ref(0, sc["ur"][1])
    trk.set_local(0, sc["rows"])
    if sim3:
        S = []
        for f in range(B):
            T = (TG.T_REF[f] if side else TG.T_CUR[0 if bc else f]).copy()
            T[:3, :] *= SCALES[f]
            S.append(T)
        trk.set_fuse_scw(0, S)
    trk.set_current_broadcast(0 if bc else -1)


def raw(trk, n=B):
    g = trk.get_fuse(0, n)
    return b"".join(np.ascontiguousarray(g[k]).tobytes() for k in ("best_idx", "best_dist", "n_found"))


def toy_map(sc):
    """Three target keyframes that hold points already (some of the list, some foreign with more observations) and the list."""
    base = sc["rows"][0]
    n_pts = len(base["cand"])
    rng = np.random.default_rng(21)
    kfs = [FR.KeyFrame("kf%d" % f, int(sc["n2"][f])) for f in range(B)]
    pts = [FR.MapPoint("p%d" % i) if base["cand"][i] else None for i in range(n_pts)]
    home = FR.KeyFrame("home", n_pts)
    for i, p in enumerate(pts):
        if p is not None:
            p.AddObservation(home, i)
            home.points[i] = p
    for f, kf in enumerate(kfs):
        for idx in rng.choice(len(kf.points), len(kf.points) // 3, replace=False):
            p = pts[int(rng.integers(0, n_pts))] if rng.random() < 0.3 else FR.MapPoint("q%d_%d" % (f, idx))
            if p is None or p.IsInKeyFrame(kf):
                continue
            p.AddObservation(kf, int(idx))
            kf.points[int(idx)] = p
            for extra in range(int(rng.integers(0, 3))):
                p.AddObservation(FR.KeyFrame("x", 1), 0)
    return kfs, pts


def toy_search(sc):
    """search(kf, i) of the restatement for target keyframe kf = ref frame f: pure, so evaluated once per keyframe."""
    base = sc["rows"][0]
    every = dict(sc, rows=[dict(base, cand=np.ones(len(base["cand"]), np.uint8))] * B)
    best = {}

    def search(kf, i):
        f = int(kf.name[2:])
        if f not in best:
            best[f] = restate(every, TOY_CFG, f)[0]
        return int(best[f][i])
    return search


TOY_CFG = (1, False, 0, 0)


# ------------------------------------------------------------------------------------------------ 1. the debug entry
@pytest.mark.parametrize("sim3", [0, 1])
def test_debug_entry_is_bit_exact_on_every_case(sd, sim3):
    from sdslam_amd import capi
    total = 0
    for c, res in FC.cases_with_reference():
        want_idx, want_dist, _, T = res[sim3]
        g = capi.debug_fuse(c["kps"], c["desc"], c["uright"], c["pts"], T, c["cam"], FC.SF, FC.INV_SIGMA2, FC.SCALE, c["th"], bool(sim3),
                            c["kp_cap"], c["max_points"])
        bad = np.flatnonzero((g["best_idx"] != want_idx) | (g["best_dist"] != want_dist))
        assert bad.size == 0, (c["name"], sim3, bad[:8], g["best_idx"][bad[:8]], want_idx[bad[:8]], g["best_dist"][bad[:8]], want_dist[bad[:8]])
        assert g["n_found"] == int((want_idx >= 0).sum())
        assert (g["rest_idx"] == -1).all() and (g["rest_dist"] == 256).all()
        R, t, Ow = FR.decompose(T, bool(sim3))
        if not sim3 or c["expect"] is not None:                  # SE3, or the exact scale 2 of the unit cases: to the bit
            assert np.array_equal(g["pose"][0], R) and np.array_equal(g["pose"][1], t) and np.array_equal(g["pose"][2], Ow), c["name"]
        total += g["n_found"]
    assert total > 500


@pytest.mark.parametrize("n_kp,n_pts", [(0, 0), (1, 3)])
def test_debug_entry_on_empty_and_unaligned_inputs(sd, n_kp, n_pts):
    """Nothing at all (the entry still launches, on capacities of 1, and returns the untouched rest of a row), and counts that
    are no multiple of the 16 bytes the entry's device arrays are carved in."""
    from sdslam_amd import capi
    c = FC.shape_case("tiny_%dx%d" % (n_kp, n_pts), 40, n_kp, n_pts)
    for sim3 in (0, 1):
        (want_idx, want_dist), T = FC.reference(c, sim3)
        assert (want_idx >= 0).sum() == (2 if n_pts else 0)          # the one keypoint is found by two of the three points
        g = capi.debug_fuse(c["kps"], c["desc"], c["uright"], c["pts"], T, c["cam"], FC.SF, FC.INV_SIGMA2, FC.SCALE, c["th"], bool(sim3))
        assert len(g["best_idx"]) == n_pts and np.array_equal(g["best_idx"], want_idx) and np.array_equal(g["best_dist"], want_dist)
        assert g["n_found"] == int((want_idx >= 0).sum())
        assert (g["rest_idx"] == -1).all() and (g["rest_dist"] == 256).all() and len(g["rest_idx"]) == (1 if n_pts == 0 else 0)
        if not sim3:
            R, t, Ow = FR.decompose(T, False)
            assert np.array_equal(g["pose"][0], R) and np.array_equal(g["pose"][1], t) and np.array_equal(g["pose"][2], Ow)


# ------------------------------------------------------------------------------------------------ 2. through extraction
@pytest.mark.parametrize("cfg", CONFIGS, ids=lambda c: "side%d-bc%d-row%d-sim%d" % c)
@pytest.mark.parametrize("name", list(RIGS))
def test_batched_path_through_extraction(sd, name, cfg):
    r = rig(sd, name)
    trk, sc = r["trk"], r["sc"]
    upload(r, cfg)
    try:
        trk.fuse(B, cfg[0], cfg[2], 3.0, bool(cfg[3]))
        g = trk.get_fuse(0, B)
        for f in range(B):
            pose = trk.fuse_pose(f) if cfg[3] else None          # an ulp in the Scw decomposition must not flip a gate
            want_idx, want_dist = restate(sc, cfg, f, pose=pose)
            n = len(want_idx)
            assert np.array_equal(g["best_idx"][f, :n], want_idx) and np.array_equal(g["best_dist"][f, :n], want_dist), (name, cfg, f)
            assert (g["best_idx"][f, n:] == -1).all() and (g["best_dist"][f, n:] == 256).all()
            assert g["n_found"][f] == int((want_idx >= 0).sum())
            assert g["n_found"][f] >= MIN_FUSED, (name, cfg, f, g["n_found"][f])
            if not cfg[3]:
                R, t, Ow = FR.decompose(TG.T_REF[f] if cfg[0] else TG.T_CUR[0 if cfg[1] else f], False)
                p = trk.fuse_pose(f)
                assert np.array_equal(p[0], R) and np.array_equal(p[1], t) and np.array_equal(p[2], Ow)
    finally:
        trk.set_current_broadcast(-1)


# ------------------------------------------------------------------------------------------------ 3. the Scw decomposition
def test_device_scw_decomposition(sd):
    """Device Rcw, tcw, Ow of the Sim3 overload against the float64 restatement, bounded by 64 x the restatement's own float64 /
    longdouble gap over the same matrices (both use the same float scw, so the gap is pure rounding).  Printed when run."""
    from sdslam_amd import capi
    rng = np.random.default_rng(9)
    c = FC.cases_with_reference()[0][0]
    gap = worst = 0.0
    mats = []
    for _ in range(48):
        T = synth.se3_exp(rng.uniform(-0.5, 0.5, 3), rng.uniform(-30, 30, 3))
        T[:3, :] *= rng.uniform(0.3, 3.0)
        mats.append(T)
        R, t, Ow = FR.decompose(T, True)
        Rl, tl, Owl = FR.decompose_longdouble(T, True)
        scale = float(max(np.abs(Rl).max(), np.abs(tl).max(), np.abs(Owl).max()))
        gap = max(gap, float(max(np.abs(R - Rl).max(), np.abs(t - tl).max(), np.abs(Ow - Owl).max())) / scale)
    bound = 64.0 * gap
    assert 0 < bound < 1e-12
    for T in mats:
        g = capi.debug_fuse(c["kps"], c["desc"], c["uright"], c["pts"], T, c["cam"], FC.SF, FC.INV_SIGMA2, FC.SCALE, 3.0, True)
        R, t, Ow = FR.decompose(T, True)
        scale = float(max(np.abs(R).max(), np.abs(t).max(), np.abs(Ow).max()))
        d = float(max(np.abs(g["pose"][0] - R).max(), np.abs(g["pose"][1] - t).max(), np.abs(g["pose"][2] - Ow).max())) / scale
        worst = max(worst, d)
        assert d <= bound, (d, bound)
    print("k_fuse Scw decomposition vs float64 restatement: largest relative deviation %.3e, float64/longdouble gap %.3e, bound %.3e"
          % (worst, gap, bound))


# ------------------------------------------------------------------------------------------------ 4. the sequential loops
def test_batched_search_and_walk_equal_the_sequential_loops(sd):
    """SearchInNeighbors' first loop on a toy map over the dense scene: one device call (kf_side 1, shared point row) + the in-order
    walk against the reference's keyframe-after-keyframe loop whose every search runs at the moment the reference runs it."""
    r = rig(sd, "dense")
    trk, sc = r["trk"], r["sc"]
    base, cfg = sc["rows"][0], TOY_CFG
    kfs_a, pts_a = toy_map(sc)
    want = FR.fuse_sequential(kfs_a, pts_a, toy_search(sc))
    kfs_b, pts_b = toy_map(sc)
    cand_rows = [dict(base, cand=np.array([p is not None and not p.isBad() and not p.IsInKeyFrame(kf) for p in pts_b], np.uint8)) for kf in kfs_b]
    upload(r, cfg)
    trk.set_local(0, cand_rows)
    trk.fuse(B, 1, 0, 3.0, False)
    g = trk.get_fuse(0, B)
    got = FR.fuse_batched_walk(kfs_b, pts_b, lambda kf, i: int(g["best_idx"][int(kf.name[2:]), i]))
    assert got == want and FR.map_state(kfs_a, pts_a) == FR.map_state(kfs_b, pts_b)
    assert sum(want) >= 20 and sum(p is not None and p.bad for p in pts_a) > 0
    assert sum(want) < int((g["best_idx"] >= 0).sum())             # the live skip tests removed something


# ------------------------------------------------------------------------------------------------ 5. lifetime and errors
def test_result_ends_with_its_inputs(sd):
    r = rig(sd, "sparse")
    trk, sc = r["trk"], r["sc"]
    ci, ri = r["imgs"]
    cfg = (1, False, 0, 1)
    upload(r, cfg)
    with pytest.raises(sd.SdError) as e:                           # upload() ended whatever there was
        trk.get_fuse(0, B)
    assert e.value.code == 1
    ending = {
        "extraction of ref": lambda: r["ref"].extract_batch(ri),
        "set_local": lambda: trk.set_local(0, sc["rows"]),
        "set_poses": lambda: trk.set_poses(0, TG.T_REF, TG.T_CUR),
        "set_uright": lambda: trk.set_uright(0, sc["ur"][0]),
        "set_uright_ref": lambda: trk.set_uright_ref(0, sc["ur"][1]),
        "set_fuse_scw": lambda: trk.set_fuse_scw(0, [np.eye(4)] * B),
        "set_camera": lambda: trk.set_camera(*TC.K, BF, TG.BOUNDS),
        "broadcast": lambda: trk.set_current_broadcast(0),
    }
    try:
        for name, call in ending.items():
            trk.fuse(B, 1, 0, 3.0, True)
            first = raw(trk)
            assert raw(trk) == first                               # reading does not end it
            call()
            with pytest.raises(sd.SdError) as e:
                trk.get_fuse(0, B)
            assert e.value.code == 1, name
            trk.set_current_broadcast(-1)
        trk.fuse(B, 1, 0, 3.0, True)
        r["cur"].extract_batch(ci)                                 # the other side's extraction does not end a side-1 result
        trk.get_fuse(0, B)
        trk.fuse(B, 0, 0, 3.0, False)
        r["cur"].extract_batch(ci)
        with pytest.raises(sd.SdError):
            trk.get_fuse(0, B)
        trk.fuse(2, 1, -1, 3.0, False)
        trk.get_fuse(0, 2)
        with pytest.raises(sd.SdError):                            # more slots than the search covered
            trk.get_fuse(0, B)
    finally:
        trk.set_current_broadcast(-1)


def test_errors(sd):
    r = rig(sd, "sparse")
    trk = r["trk"]
    L = sd.lib()
    upload(r, (1, False, 0, 0))
    bad = [((0, 1, 0, 3.0, False), 3), ((B + 1, 1, 0, 3.0, False), 3), ((B, 1, 0, 0.0, False), 1), ((B, 1, 0, -1.0, False), 1),
           ((B, 1, 0, float("inf"), False), 1), ((B, 1, 0, float("nan"), False), 1), ((B, 1, -2, 3.0, False), 1), ((B, 1, B, 3.0, False), 1),
           ((B, 2, 0, 3.0, False), 1), ((B, -1, 0, 3.0, False), 1)]
    for args, code in bad:
        with pytest.raises(sd.SdError) as e:
            trk.fuse(*args)
        assert e.value.code == code, args
    assert L.sd_track_fuse(trk.h, B, 1, 0, 3.0, 2) == 1
    assert L.sd_track_fuse(None, B, 1, 0, 3.0, 0) == 1
    tiny = (50, 1.2, 1, 20, 64, 64)
    ext = [sd.ORBextractor(*tiny, 2) for _ in range(2)]
    t2 = sd.Tracker(ext[0], ext[1], max_points=8, max_batch=2, pnp_max_iterations=4)
    try:
        with pytest.raises(sd.SdError) as e:                       # no camera
            t2.fuse(1, 1, -1, 3.0, False)
        assert e.value.code == 1
        t2.set_camera(*TC.K, BF, (0.0, 64.0, 0.0, 64.0))
        for side in (0, 1):                                        # no extraction on the side in use
            with pytest.raises(sd.SdError) as e:
                t2.fuse(1, side, -1, 3.0, False)
            assert e.value.code == 1
        ext[1].extract_batch(synth.make_batch(5, 2, 64, 64))
        with pytest.raises(sd.SdError) as e:                       # Scw never set
            t2.fuse(2, 1, -1, 3.0, True)
        assert e.value.code == 1
        t2.set_fuse_scw(0, [np.eye(4)])
        t2.fuse(1, 1, -1, 3.0, True)
        with pytest.raises(sd.SdError) as e:                       # slot 1 still uncovered
            t2.fuse(2, 1, -1, 3.0, True)
        assert e.value.code == 1
        with pytest.raises(sd.SdError) as e:
            t2.set_fuse_scw(2, [np.eye(4)])
        assert e.value.code == 3
        g = np.zeros((1, 4), np.int32)
        t2.fuse(1, 1, -1, 3.0, False)
        assert L.sd_track_get_fuse(t2.h, 0, 1, g.ctypes.data, None, 4, None) == 3      # cap < max_points
        assert L.sd_track_get_fuse(t2.h, 0, 1, None, None, 0, None) == 0               # NULL outputs are skipped
    finally:
        t2.close()
        for e_ in ext:
            e_.close()


# ------------------------------------------------------------------------------------------------ 6. determinism, neighbours
def test_twice_is_byte_identical_and_other_results_are_untouched(sd):
    r = rig(sd, "dense")
    trk, sc = r["trk"], r["sc"]
    cfg = (1, False, 0, 0)
    upload(r, cfg)
    rng = np.random.default_rng(3)
    trk.set_point_flags(0, (rng.random((B, sc["cap"])) < 0.5).astype(np.uint8), (rng.random((B, sc["cap"])) < 0.5).astype(np.uint8))
    trk.search_by_points(B, 0.75, True)
    trk.search_for_triangulation(B, False, False)
    trk.match_local(B, 3.0, 0.8, 0.5)
    pm, tri, loc = trk.get_point_matches(0, B), TG.raw(trk), trk.get_local(0, B)
    trk.fuse(B, 1, 0, 3.0, False)
    first = raw(trk)
    trk.fuse(B, 1, 0, 3.0, False)
    assert raw(trk) == first and trk.get_fuse(0, B)["n_found"].sum() >= 60
    pm2, loc2 = trk.get_point_matches(0, B), trk.get_local(0, B)
    assert np.array_equal(pm[0], pm2[0]) and np.array_equal(pm[1], pm2[1]) and pm[1].sum() > 0
    assert TG.raw(trk) == tri
    assert all(np.array_equal(loc[k], loc2[k]) for k in loc) and loc["n"].sum() > 0
    trk.search_by_points(B, 0.75, True)                            # ... and they leave the Fuse result alone
    trk.search_for_triangulation(B, False, False)
    trk.match_local(B, 3.0, 0.8, 0.5)
    assert raw(trk) == first
