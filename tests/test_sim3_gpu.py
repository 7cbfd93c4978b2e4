"""k_sim3 (Sim3Solver on the device, sdslam_amd/csrc/track_sim3.hip) against the numpy restatement tests/sim3_ref.py on the ten
slots of tests/sim3_cases.py: both pyramids, fix_scale both ways, once as find() and once as iterate(5) calls, compared call
by call -- info8 and the inlier mask exactly, T12 / R / t to 1e-5 absolute, scale to 1e-5 relative.  Then the API's own
promises: broadcast = paired, a solve on SearchByPoints' device output = a solve on the re-uploaded vector, queued =
synchronised, stale / short-stream / bad-argument calls refused.

Largest deviations measured on the MI355X (printed by test_against_restatement): see DESIGN.md §4 (k_sim3)."""
import numpy as np
import pytest

import sim3_cases as SC

pytestmark = pytest.mark.gpu
B = SC.B
_RIGS, _REF = {}, {}


def _rig(oracle, pyr):
    if pyr in _RIGS:
        return _RIGS[pyr]
    import sdslam_amd as sd
    if sd.device_count() < 1:
        pytest.fail("no HIP device: the gpu-marked tests need a real MI355X")
    cfg = SC.PYR[pyr]
    cur, ref = sd.ORBextractor(*cfg, SC.W, SC.H, B), sd.ORBextractor(*cfg, SC.W, SC.H, B)
    imgs = SC.images()
    k1, _, n1 = cur.extract_batch(imgs[0])
    k2, _, n2 = ref.extract_batch(imgs[1])
    trk = sd.Tracker(cur, ref, max_points=SC.NFEAT, max_batch=B, pnp_max_iterations=SC.MAX_ITS)
    trk.set_camera(*SC.K, 0.0, SC.BOUNDS)
    # the cases (and their margin condition, tests/test_sim3_cpu.py) were built on the oracle's keypoints: the device's are the same
    oct1, on1, oct2, on2 = SC.oracle_keypoints(oracle, pyr)
    assert np.array_equal(n1, on1) and np.array_equal(n2, on2)
    for b in range(B):
        assert np.array_equal(k1["octave"][b, :n1[b]], oct1[b, :n1[b]]) and np.array_equal(k2["octave"][b, :n2[b]], oct2[b, :n2[b]])
    slots, rand = SC.make_batch(pyr, oct1, on1, oct2, on2)
    _RIGS[pyr] = dict(sd=sd, trk=trk, cur=cur, ref=ref, imgs=imgs, slots=slots, rand=rand)
    return _RIGS[pyr]


def _ref(r, pyr, fix):
    if (pyr, fix) not in _REF:
        _REF[(pyr, fix)] = SC.reference_runs(r["slots"], r["rand"], pyr, fix)
    return _REF[(pyr, fix)]


def _raw(trk, n=B):
    g = trk.get_sim3(0, n)
    return b"".join(np.ascontiguousarray(g[k]).tobytes() for k in ("T12", "R", "t", "scale", "inliers", "info"))


def _compare(g, b, result, info, R, t, s, where, worst):
    T12, no_more, inl, n = result
    assert np.array_equal(g["info"][b], info), (where, g["info"][b], info)
    assert np.array_equal(g["inliers"][b], inl), where
    for name, got, want in (("T12", g["T12"][b], T12), ("R", g["R"][b], R), ("t", g["t"][b], t)):
        assert np.array_equal(np.isnan(got), np.isnan(want)), (where, name)
        d = np.abs(got - want)
        d = float(d[~np.isnan(d)].max()) if (~np.isnan(d)).any() else 0.0
        worst[name] = max(worst[name], d)
        assert d <= 1e-5, (where, name, d)
    assert np.isnan(g["scale"][b]) == np.isnan(s), where
    if not np.isnan(s) and s != 0:
        d = abs(g["scale"][b] - s) / abs(s)
        worst["scale"] = max(worst["scale"], d)
        assert d <= 1e-5, (where, "scale", d)
    else:
        assert np.isnan(s) or g["scale"][b] == 0


@pytest.mark.parametrize("fix", [0, 1])
@pytest.mark.parametrize("pyr", list(SC.PYR))
def test_against_restatement(oracle, pyr, fix):
    r = _rig(oracle, pyr)
    trk, slots = r["trk"], r["slots"]
    want = _ref(r, pyr, fix)
    SC.upload(trk, slots, r["rand"])
    worst = dict(T12=0.0, R=0.0, t=0.0, scale=0.0)
    # find()
    trk.sim3(B, fix, SC.PROB, SC.MIN_INLIERS, SC.MAX_ITS, SC.MAX_ITS)
    g = trk.get_sim3(0, B)
    for b, sl in enumerate(slots):
        res, info, sv = want["find"][b]
        _compare(g, b, res, info, sv.best_R, sv.best_t, float(sv.best_s), (pyr, fix, "find", sl["kind"]), worst)
    assert (fix == 1 or g["returned"].sum() >= 5) and g["no_more"].sum() >= 5      # both endings occur
    # iterate(5), call by call
    for c, row in enumerate(want["rounds"]):
        if c == 0:
            trk.sim3(B, fix, SC.PROB, SC.MIN_INLIERS, SC.MAX_ITS, 5)
        else:
            trk.sim3_iterate(B, 5)
        g = trk.get_sim3(0, B)
        for b, sl in enumerate(slots):
            res, info, R, t, s = row[b]
            _compare(g, b, res, info, R, t, s, (pyr, fix, "call %d" % c, sl["kind"]), worst)
    assert len(want["rounds"]) >= 25
    print("k_sim3 vs restatement, largest deviation", pyr, "fix_scale", fix, worst)


K_ANISO = tuple(float(np.float32(v)) for v in (4000.0, 3200.0, 148.5, 131.25))      # fx != fy, principal point off the centre


@pytest.mark.parametrize("fix", [0, 1])
def test_against_restatement_anisotropic_camera(oracle, fix):
    """Project's fx / fy and cx / cy told apart: the n70_out30 and mixed_octaves slots under K_ANISO, as find() and as
    iterate(5) calls, to test_against_restatement's bounds.  (SC.K has fx = fy and the principal point at the centre.)  The
    planted outliers of these slots miss by hundreds of pixels under either camera, so this pins the projection at the
    inliers' errors only: a camera mix-up that leaves every inlier under its threshold would pass."""
    r = _rig(oracle, "p8")
    trk, slots = r["trk"], r["slots"]
    picked = [SC.SLOTS.index("n70_out30"), SC.SLOTS.index("mixed_octaves")]
    want = SC.reference_runs([slots[b] for b in picked], r["rand"][picked], "p8", fix, K=K_ANISO)
    worst = dict(T12=0.0, R=0.0, t=0.0, scale=0.0)
    try:
        trk.set_camera(*K_ANISO, 0.0, SC.BOUNDS)
        SC.upload(trk, slots, r["rand"])
        trk.sim3(B, fix, SC.PROB, SC.MIN_INLIERS, SC.MAX_ITS, SC.MAX_ITS)
        g = trk.get_sim3(0, B)
        for j, b in enumerate(picked):
            res, info, sv = want["find"][j]
            _compare(g, b, res, info, sv.best_R, sv.best_t, float(sv.best_s), ("aniso", fix, "find", slots[b]["kind"]), worst)
        for c, row in enumerate(want["rounds"]):
            if c == 0:
                trk.sim3(B, fix, SC.PROB, SC.MIN_INLIERS, SC.MAX_ITS, 5)
            else:
                trk.sim3_iterate(B, 5)
            g = trk.get_sim3(0, B)
            for j, b in enumerate(picked):
                res, info, R, t, s = row[j]
                _compare(g, b, res, info, R, t, s, ("aniso", fix, "call %d" % c, slots[b]["kind"]), worst)
        print("k_sim3 vs restatement under K_ANISO, largest deviation, fix_scale", fix, worst)
    finally:
        trk.set_camera(*SC.K, 0.0, SC.BOUNDS)
        SC.upload(trk, slots, r["rand"])


def test_broadcast_equals_paired(oracle):
    r = _rig(oracle, "p8")
    trk = r["trk"]
    SC.upload(trk, r["slots"], r["rand"])
    trk.sim3(B, 0, SC.PROB, SC.MIN_INLIERS, SC.MAX_ITS, 5)
    trk.sim3_iterate(B, 7)
    paired = _raw(trk)
    trk.set_current_broadcast(0)
    try:
        with pytest.raises(r["sd"].SdError):       # built under another pairing
            trk.sim3_iterate(B, 7)
        trk.sim3(B, 0, SC.PROB, SC.MIN_INLIERS, SC.MAX_ITS, 5)
        trk.sim3_iterate(B, 7)
        assert _raw(trk) == paired
    finally:
        trk.set_current_broadcast(-1)
    assert trk.get_sim3(0, B)["returned"].sum() >= 3


def test_solves_search_by_points_output_in_place(oracle):
    """The match vector SearchByPoints left on the device, solved without a host copy = the same vector downloaded and given
    back through sd_track_set_point_matches."""
    r = _rig(oracle, "p8")
    trk = r["trk"]
    SC.upload(trk, r["slots"], r["rand"])
    ones = np.ones((B, SC.NFEAT), np.uint8)
    trk.set_point_flags(0, ones, ones)
    trk.search_by_points(B, 0.75, True)
    trk.sim3(B, 0, SC.PROB, SC.MIN_INLIERS, SC.MAX_ITS, SC.MAX_ITS)
    in_place = _raw(trk)
    g = trk.get_sim3(0, B)
    m, nm = trk.get_point_matches(0, B)
    same = SC.SLOTS.index("kf1_is_kf2")
    assert nm[same] >= 250 and g["N"][same] == nm[same] and g["iterations"][same] == SC.MAX_ITS      # not vacuous
    assert np.array_equal(g["N"], nm)
    trk.set_point_matches(0, m)
    trk.sim3(B, 0, SC.PROB, SC.MIN_INLIERS, SC.MAX_ITS, SC.MAX_ITS)
    assert _raw(trk) == in_place


def test_queued_equals_synchronised(oracle):
    r = _rig(oracle, "p5")
    trk = r["trk"]
    SC.upload(trk, r["slots"], r["rand"])
    trk.sim3(B, 0, SC.PROB, SC.MIN_INLIERS, SC.MAX_ITS, 5)
    for n in (5, 3, 64, 70):
        trk.sim3_iterate(B, n)
    queued = _raw(trk)
    trk.sim3(B, 0, SC.PROB, SC.MIN_INLIERS, SC.MAX_ITS, 5)
    _raw(trk)
    for n in (5, 3, 64, 70):
        trk.sim3_iterate(B, n)
        _raw(trk)
    assert _raw(trk) == queued


def test_stale_iterate_is_refused(oracle):
    r = _rig(oracle, "p8")
    sd, trk, slots, rand = r["sd"], r["trk"], r["slots"], r["rand"]
    SC.upload(trk, slots, rand)
    ones = np.ones((B, SC.NFEAT), np.uint8)
    replacing = {
        "extraction of cur": lambda: r["cur"].extract_batch(r["imgs"][0]),
        "extraction of ref": lambda: r["ref"].extract_batch(r["imgs"][1]),
        "set_point_matches": lambda: trk.set_point_matches(0, np.stack([s["matches12"] for s in slots])),
        "set_sim3_points": lambda: trk.set_sim3_points(0, np.stack([s["kf1"]["Xw"] for s in slots]), np.stack([s["kf2"]["Xw"] for s in slots])),
        "set_point_flags": lambda: trk.set_point_flags(0, np.stack([s["kf1"]["has_mp"] for s in slots]), np.stack([s["kf2"]["has_mp"] for s in slots])),
        "set_poses": lambda: trk.set_poses(0, [s["kf2"]["T"] for s in slots], [s["kf1"]["T"] for s in slots]),
        "set_rand": lambda: trk.set_rand(0, rand),
    }
    with pytest.raises(sd.SdError) as e:           # nothing constructed yet (upload() ended whatever was)
        trk.sim3_iterate(B, 5)
    assert e.value.code == 1
    for name, call in replacing.items():
        trk.sim3(B, 0, SC.PROB, SC.MIN_INLIERS, SC.MAX_ITS, 5)
        trk.sim3_iterate(B, 5)
        call()
        with pytest.raises(sd.SdError) as e:
            trk.sim3_iterate(B, 5)
        assert e.value.code == 1, name
    trk.sim3(4, 0, SC.PROB, SC.MIN_INLIERS, SC.MAX_ITS, 5)
    trk.sim3_iterate(3, 5)
    with pytest.raises(sd.SdError):                # more slots than were constructed
        trk.sim3_iterate(5, 5)
    trk.sim3(B, 0, SC.PROB, SC.MIN_INLIERS, SC.MAX_ITS, 5)
    trk.search_by_points(B, 0.75, True)
    with pytest.raises(sd.SdError):
        trk.sim3_iterate(B, 5)
    SC.upload(trk, slots, rand)


def test_short_rand_stream_and_bad_arguments_are_refused(oracle):
    r = _rig(oracle, "p8")
    sd, trk, slots, rand = r["sd"], r["trk"], r["slots"], r["rand"]
    SC.upload(trk, slots, rand)
    trk.set_rand(0, rand[:, :14])
    with pytest.raises(sd.SdError) as e:           # 5 iterations draw 15 values
        trk.sim3(B, 0, SC.PROB, SC.MIN_INLIERS, SC.MAX_ITS, 5)
    assert e.value.code == 1
    trk.set_rand(0, rand[:, :15])
    trk.sim3(B, 0, SC.PROB, SC.MIN_INLIERS, SC.MAX_ITS, 5)
    with pytest.raises(sd.SdError) as e:
        trk.sim3_iterate(B, 1)
    assert e.value.code == 1
    trk.sim3(B, 0, SC.PROB, SC.MIN_INLIERS, 5, 300)          # max_iterations = 5 bounds it however many are asked for
    trk.sim3_iterate(B, 300)
    assert (trk.get_sim3(0, B)["iterations"] <= 5).all()
    with pytest.raises(sd.SdError) as e:           # more than a slot's stream can ever hold (4 x pnp_max_iterations values)
        trk.sim3(B, 0, SC.PROB, SC.MIN_INLIERS, 401, 401)
    assert e.value.code == 3
    trk.set_rand(0, rand)
    bad = [dict(probability=0.0), dict(probability=1.0), dict(min_inliers=2), dict(max_iterations=0), dict(n_iterations=0)]
    for kw in bad:
        args = dict(fix_scale=0, probability=SC.PROB, min_inliers=SC.MIN_INLIERS, max_iterations=SC.MAX_ITS, n_iterations=5)
        args.update(kw)
        with pytest.raises(sd.SdError) as e:
            trk.sim3(B, **args)
        assert e.value.code == 1, kw
    for n in (0, B + 1):
        with pytest.raises(sd.SdError) as e:
            trk.sim3(n, 0, SC.PROB, SC.MIN_INLIERS, SC.MAX_ITS, 5)
        assert e.value.code == 3
    trk.sim3(B, 0, SC.PROB, SC.MIN_INLIERS, SC.MAX_ITS, 5)
    with pytest.raises(sd.SdError):
        trk.sim3_iterate(B, 0)
    m = np.full((1, SC.NFEAT), -1, np.int32)
    m[0, 3] = SC.NFEAT
    with pytest.raises(sd.SdError):
        trk.set_point_matches(0, m)
    with pytest.raises(sd.SdError):
        trk.set_point_matches(0, np.full((1, SC.NFEAT + 1), -1, np.int32))
    with pytest.raises(sd.SdError):
        trk.set_sim3_points(B, np.zeros((1, 4, 3)), np.zeros((1, 4, 3)))
    with pytest.raises(sd.SdError):
        trk.get_sim3(B, 1)
    # shorter rows are padded: NULL matches, untouched points
    trk.set_point_matches(0, np.full((B, 7), -1, np.int32))
    trk.sim3(B, 0, SC.PROB, SC.MIN_INLIERS, SC.MAX_ITS, 5)
    g = trk.get_sim3(0, B)
    assert (g["N"] == 0).all() and g["no_more"].all() and not g["inliers"].any() and not g["T12"].any()
    SC.upload(trk, slots, rand)
