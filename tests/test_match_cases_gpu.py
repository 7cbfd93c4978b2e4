"""The hand-worked gate and tie cases of tests/match_cases.py on the device: the current frame's (for SearchByPoints both
frames') keypoints and descriptors are planted with ORBextractor.set_keypoints, the last-frame / local-map side goes through
set_last / set_local, and all cases of a matcher run in one launch, one slot per case.  The match vectors, counts, in_view and
level equal the hand answers AND the oracle's (tests/test_match_cases_cpu.py shows on the host that the two are the same thing;
both are asserted so a failure says which side moved).  Integer work: no tolerance anywhere."""
import numpy as np
import pytest

import match_cases as MC

pytestmark = pytest.mark.gpu
CFG = (100, 1.2, 8, 20)
MP = 64


def _blank_pair(sd, cfg, B):
    """Two extractors that have extracted once (nothing, from black frames): set_keypoints plants into an existing output set"""
    cur, ref = sd.ORBextractor(*cfg, 640, 480, B), sd.ORBextractor(*cfg, 640, 480, B)
    blank = np.zeros((B, 480, 640), np.uint8)
    for e in (cur, ref):
        assert e.extract_batch(blank)[2].tolist() == [0] * B
    return cur, ref


@pytest.fixture(scope="module")
def rig(oracle):
    import sdslam_amd as sd
    if sd.device_count() < 1:
        pytest.fail("no HIP device: the gpu-marked tests need a real MI355X")
    cases = MC.all_cases()
    B = max(len(cases[g]) for g in ("projection", "stereo", "local", "points"))
    cur, ref = _blank_pair(sd, CFG, B)
    assert np.array_equal(cur.GetScaleFactors(), MC.SF)
    mono, stereo = sd.Tracker(cur, ref, MP, B, 8), sd.Tracker(cur, ref, MP, B, 8)           # one tracker per camera
    mono.set_camera(*MC.K, 0.0, MC.BOUNDS)
    stereo.set_camera(*MC.K, MC.BF, MC.BOUNDS)
    yield dict(sd=sd, cases=cases, B=B, cur=cur, ref=ref, mono=mono, stereo=stereo, cap=mono.cap)
    for h in (mono, stereo, cur, ref):
        h.close()


def _rows(arrays, cap, dtype, fill):
    out = np.full((len(arrays), cap), fill, dtype)
    for i, a in enumerate(arrays):
        out[i, :len(a)] = a
    return out


def _vector_is(got_row, want, what):
    """The first len(want) entries are `want`, every entry behind them is -1"""
    assert got_row[:len(want)].tolist() == list(want), what
    assert (got_row[len(want):] == -1).all(), what


def _run_projection(rig, trk, group, split):
    n = len(group)
    rig["cur"].set_keypoints(0, [c["kps"] for c in group], [c["desc"] for c in group])
    trk.set_uright(0, _rows([c["uright"] for c in group], rig["cap"], np.float32, -1.0))
    trk.set_last(0, [c["last"] for c in group])
    trk.set_poses(0, [c["T_ref"] for c in group], [c["T_cur"] for c in group])
    with rig["sd"].options({"track.match_split": split}):
        trk.match(n, th=MC.TH, mono=group[0]["mono"], check_ori=True)
        cm, nm = trk.get_matches(0, n)
        trk.match(n, th=MC.TH, mono=group[0]["mono"], check_ori=True)
        cm2, nm2 = trk.get_matches(0, n)
    assert cm.tobytes() == cm2.tobytes() and nm.tobytes() == nm2.tobytes()                 # the same launch again: the same bytes
    return cm, nm


def _oracle_projection(oracle, c):
    stereo = not c["mono"]
    return oracle.search_by_projection(c["kps"], c["desc"], MC.SF, MC.BOUNDS, MC.K, c["T_cur"], c["T_ref"], c["last"], th=MC.TH, mono=c["mono"],
                                       check_ori=True, u_right=c["uright"] if stereo else None, mbf=MC.BF if stereo else 0.0,
                                       mb=MC.MB if stereo else 0.0)


@pytest.mark.parametrize("split", [1, 0], ids=["split", "single"])
@pytest.mark.parametrize("group", ["projection", "stereo"])
def test_search_by_projection_cases(oracle, rig, group, split):
    cases = rig["cases"][group]
    assert all(c["mono"] == (group == "projection") for c in cases)
    cm, nm = _run_projection(rig, rig["mono" if group == "projection" else "stereo"], cases, split)
    for i, c in enumerate(cases):
        what = (group, c["name"], split)
        _vector_is(cm[i], c["expect"]["match"], what + ("hand answer",))
        assert nm[i] == c["expect"]["n"], what
        n, m = _oracle_projection(oracle, c)
        _vector_is(cm[i], m.tolist(), what + ("oracle",))
        assert nm[i] == n, what


@pytest.mark.parametrize("th", MC.LOCAL_THS)
def test_local_map_search_cases(oracle, rig, th):
    cases, trk = rig["cases"]["local"], rig["stereo"]
    n = len(cases)
    rig["cur"].set_keypoints(0, [c["kps"] for c in cases], [c["desc"] for c in cases])
    trk.set_uright(0, _rows([c["uright"] for c in cases], rig["cap"], np.float32, -1.0))
    trk.set_local(0, [c["pts"] for c in cases], kp_claimed=[c["kp_claimed"] for c in cases])
    trk.set_poses(0, [np.eye(4)] * n, [c["T_cur"] for c in cases])
    runs = []
    for _ in range(2):
        trk.match_local(n, th=th, nnratio=MC.NNRATIO, cos_limit=MC.COS_LIMIT)
        runs.append(trk.get_local(0, n))
    g = runs[0]
    assert all(g[k].tobytes() == runs[1][k].tobytes() for k in ("match", "n", "in_view", "level"))
    for i, c in enumerate(cases):
        M, e, what = len(c["pts"]["cand"]), c["expect"][th], (c["name"], th)
        r = oracle.search_local_points(c["kps"], c["desc"], MC.SF, MC.LOG_SF, MC.BOUNDS, MC.K, MC.BF, c["T_cur"], c["pts"], th=th,
                                       nnratio=MC.NNRATIO, u_right=c["uright"], kp_claimed=c["kp_claimed"], cos_limit=MC.COS_LIMIT)
        for want, side in ((e, "hand answer"), (dict(match=r["match"].tolist(), n=r["n"], in_view=r["in_view"].tolist(),
                                                     level=r["level"].tolist()), "oracle")):
            _vector_is(g["match"][i], want["match"], what + (side,))
            assert g["n"][i] == want["n"], what + (side,)
            assert g["in_view"][i, :M].tolist() == want["in_view"] and g["level"][i, :M].tolist() == want["level"], what + (side,)


@pytest.mark.parametrize("klist", MC.BF_LIST_KS)
def test_search_by_points_cases(oracle, rig, klist):
    cases, trk, cap, sd = rig["cases"]["points"], rig["mono"], rig["cap"], rig["sd"]
    n = len(cases)
    rig["cur"].set_keypoints(0, [c["k1"] for c in cases], [c["d1"] for c in cases])
    rig["ref"].set_keypoints(0, [c["k2"] for c in cases], [c["d2"] for c in cases])
    trk.set_point_flags(0, _rows([c["h1"] for c in cases], cap, np.uint8, 1), _rows([c["h2"] for c in cases], cap, np.uint8, 1))
    with sd.options({"track.bf_list_k": klist}):
        for ori in (True, False):
            trk.search_by_points(n, MC.NNRATIO_POINTS, ori)
            m, nm = trk.get_point_matches(0, n)
            trk.search_by_points(n, MC.NNRATIO_POINTS, ori)
            m2, nm2 = trk.get_point_matches(0, n)
            assert m.tobytes() == m2.tobytes() and nm.tobytes() == nm2.tobytes()
            for i, c in enumerate(cases):
                what = (c["name"], klist, ori)
                _vector_is(m[i], c["expect"][ori]["match"], what + ("hand answer",))
                assert nm[i] == c["expect"][ori]["n"], what
                on, om = oracle.search_by_points(c["k1"], c["d1"], c["h1"], c["k2"], c["d2"], c["h2"], MC.NNRATIO_POINTS, ori)
                _vector_is(m[i], om.tolist(), what + ("oracle",))
                assert nm[i] == on, what


def test_crowded_window(oracle, rig):
    """1500 candidates per point: the key lists overflow and phase 2 evaluates the late points itself, under both forms"""
    sd, c = rig["sd"], rig["cases"]["crowd"]
    cur, ref = _blank_pair(sd, (MC.CROWD_CAPACITY,) + CFG[1:], 1)
    trk = sd.Tracker(cur, ref, 16, 1, 8)
    try:
        assert trk.cap == MC.CROWD_CAPACITY <= 2047
        trk.set_camera(*MC.K, 0.0, MC.BOUNDS)
        cur.set_keypoints(0, [c["kps"]], [c["desc"]])
        trk.set_last(0, [c["last"]])
        trk.set_poses(0, [c["T_ref"]], [c["T_cur"]])
        n, m = _oracle_projection(oracle, c)
        assert n == len(c["last"]["valid"])
        for split in (1, 0):
            with sd.options({"track.match_split": split}):
                trk.match(1, th=MC.TH, mono=True, check_ori=True)
            cm, nm = trk.get_matches(0, 1)
            _vector_is(cm[0], m.tolist(), ("crowd", split))
            assert nm[0] == n, split
    finally:
        for h in (trk, cur, ref):
            h.close()


def test_set_keypoints_refusals(rig):
    sd, cur, B, cap = rig["sd"], rig["cur"], rig["B"], rig["cap"]
    one = np.zeros(1, sd.capi.KP_DTYPE)

    def refused(call, code):
        with pytest.raises(sd.SdError) as e:
            call()
        assert e.value.code == code, e.value

    refused(lambda: cur.set_keypoints(0, [np.zeros(cap + 1, sd.capi.KP_DTYPE)], [np.zeros((cap + 1, 32), np.uint8)]), 3)   # over the capacity
    refused(lambda: cur.set_keypoints(B, [one], [np.zeros((1, 32), np.uint8)]), 3)                    # slot out of range
    refused(lambda: cur.set_keypoints(B - 1, [one, one], [np.zeros((1, 32), np.uint8)] * 2), 3)
    refused(lambda: cur.set_keypoints(-1, [one], [np.zeros((1, 32), np.uint8)]), 3)
    cur.set_keypoints(B - 1, [np.zeros(cap, sd.capi.KP_DTYPE)], [np.zeros((cap, 32), np.uint8)])      # the capacity itself, the last slot
    assert cur.download(B - 1, 1)[2].tolist() == [cap]
    fresh = sd.ORBextractor(*CFG, 640, 480, 1)
    try:
        refused(lambda: fresh.set_keypoints(0, [one], [np.zeros((1, 32), np.uint8)]), 1)               # nothing extracted yet: no output set geometry
        fresh.extract_batch(np.zeros((1, 480, 640), np.uint8))
        fresh.set_distortion(*MC.K, 0.1)
        refused(lambda: fresh.set_keypoints(0, [one], [np.zeros((1, 32), np.uint8)]), 1)               # mvKeysUn would be a second array
        fresh.set_distortion(*MC.K, 0.0)
        k = np.zeros(2, sd.capi.KP_DTYPE)
        k["x"], k["octave"] = [3.5, 100.25], [0, 7]
        d = np.arange(64, dtype=np.uint8).reshape(2, 32)
        fresh.set_keypoints(0, [k], [d])
        gk, gd, gn = fresh.download(0, 1)
        assert gn.tolist() == [2] and np.array_equal(gk[0, :2], k) and np.array_equal(gd[0, :2], d)     # what was planted is what is there
        assert np.array_equal(fresh.download_undistorted(0, 1)[0, :2], k)
    finally:
        fresh.close()


def test_planting_ends_earlier_results(rig):
    """To a tracker a set_keypoints call is an extraction: a Fuse result on that side's frames is refused afterwards"""
    sd, trk, cur, ref = rig["sd"], rig["stereo"], rig["cur"], rig["ref"]
    cases = rig["cases"]["local"]
    n = len(cases)
    kps, desc = [c["kps"] for c in cases], [c["desc"] for c in cases]
    cur.set_keypoints(0, kps, desc)
    ref.set_keypoints(0, kps, desc)
    trk.set_local(0, [c["pts"] for c in cases])
    trk.set_poses(0, [np.eye(4)] * n, [np.eye(4)] * n)
    for side, planted, other in ((0, cur, ref), (1, ref, cur)):
        trk.fuse(n, side, -1, 3.0, False)
        first = trk.get_fuse(0, n)
        assert first["n_found"].sum() > 0
        other.set_keypoints(0, kps[:1], desc[:1])                   # the other side's frames: the result stays
        assert trk.get_fuse(0, n)["best_idx"].tobytes() == first["best_idx"].tobytes()
        planted.set_keypoints(0, kps[:1], desc[:1])
        with pytest.raises(sd.SdError) as e:
            trk.get_fuse(0, n)
        assert e.value.code == 1
        trk.fuse(n, side, -1, 3.0, False)                           # the stage runs again: a result again, the same one
        assert trk.get_fuse(0, n)["best_idx"].tobytes() == first["best_idx"].tobytes()
