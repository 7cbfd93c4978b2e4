"""The hand-built PoseOptimization problems of tests/poseopt_cases.py on the device: every case is one frame of ONE k_pose_opt
launch (keypoints planted with ORBextractor.set_keypoints, map points through set_last / set_matches, right coordinates through
set_uright), run with one and with four waves per frame and twice each.  Against the oracle: pose within POSE_TOL, identical flags,
identical counts; iterations and LM trials too where tests/test_poseopt_cases_cpu.py certified the case count-stable.  The hand
answers are asserted directly as well, so a failure says which side moved."""
import numpy as np
import pytest

import match_cases as MC
import poseopt_cases as PC

pytestmark = pytest.mark.gpu
CFG = (PC.CAPACITY, 1.2, 8, 20)
BOUNDS = (0.0, 640.0, 0.0, 480.0)


@pytest.fixture(scope="module")
def rig(oracle):
    import sdslam_amd as sd
    if sd.device_count() < 1:
        pytest.fail("no HIP device: the gpu-marked tests need a real MI355X")
    cases = PC.all_cases()
    B = len(cases)
    cur, ref = sd.ORBextractor(*CFG, 640, 480, B), sd.ORBextractor(*CFG, 640, 480, B)
    blank = np.zeros((B, 480, 640), np.uint8)
    for e in (cur, ref):
        assert e.extract_batch(blank)[2].tolist() == [0] * B
    assert cur.cap == PC.CAPACITY and np.array_equal(cur.GetInverseScaleSigmaSquares(), PC.INV_SIGMA2)
    trk = sd.Tracker(cur, ref, cur.cap, B, 8)                      # max_points = the keypoint capacity: the `full` case needs it
    assert trk.cap == PC.CAPACITY
    yield dict(sd=sd, cases=cases, B=B, cur=cur, ref=ref, trk=trk, cap=trk.cap, certs=[PC.certify(oracle, c) for c in cases])
    for h in (trk, cur, ref):
        h.close()


def _plant(rig):
    cases, trk, cap, B = rig["cases"], rig["trk"], rig["cap"], rig["B"]
    dev = [PC.device_inputs(c) for c in cases]
    ur, match = np.full((B, cap), -1.0, np.float32), np.full((B, cap), -1, np.int32)
    for i, (c, d) in enumerate(zip(cases, dev)):
        ur[i, :len(c["kps"])], match[i, :len(c["kps"])] = c["uright"], d[3]
    rig["cur"].set_keypoints(0, [d[0] for d in dev], [d[1] for d in dev])
    trk.set_uright(0, ur)
    trk.set_last(0, [d[2] for d in dev])
    trk.set_matches(0, match)
    trk.set_poses(0, [np.eye(4)] * B, [c["T0"] for c in cases])


def _launch(rig, bf, waves):
    trk, B = rig["trk"], rig["B"]
    trk.set_camera(*PC.K, bf, BOUNDS)
    runs = []
    with rig["sd"].options({"track.poseopt_waves": waves}):
        for _ in range(2):
            trk.pose_opt(B, source=0)
            runs.append(trk.get_pose_opt(0, B))
    a, b = runs
    assert np.array_equal(np.stack(a["T"]), np.stack(b["T"])) and a["outlier"].tobytes() == b["outlier"].tobytes()       # the same launch again: the same bits
    for k in ("n_initial", "n_bad", "rounds", "iterations", "lm_trials", "n_inliers"):
        assert np.array_equal(a[k], b[k]), k
    return a


@pytest.mark.parametrize("waves", [1, 4])
def test_poseopt_cases(rig, waves):
    _plant(rig)
    worst = 0.0
    for bf in sorted({c["bf"] for c in rig["cases"]}):
        g = _launch(rig, bf, waves)
        for i, (c, cert) in enumerate(zip(rig["cases"], rig["certs"])):
            if c["bf"] != bf:
                continue
            r, n, what = cert["ref"], len(c["kps"]), (c["name"], waves)
            got = (g["n_initial"][i], g["n_bad"][i], g["rounds"][i], g["iterations"][i], g["lm_trials"][i])
            d = np.abs(g["T"][i] - r["T"]).max()
            worst = max(worst, d)
            print(f"{c['name']} waves {waves}: pose difference {d:.2e}, device (n, bad, rounds, its, trials) {tuple(int(v) for v in got)}, oracle "
                  f"{tuple(int(v) for v in r['info'])}, count-stable {cert['count_stable']}")
            assert d <= PC.POSE_TOL, what
            assert np.array_equal(g["outlier"][i, :n], r["outlier"]), what + (np.flatnonzero(g["outlier"][i, :n] != r["outlier"]),)
            assert not g["outlier"][i, n:].any(), what
            assert got[:3] == tuple(r["info"][:3]) and g["n_inliers"][i] == r["n_inliers"], what
            if cert["count_stable"]:
                assert got[3:] == tuple(r["info"][3:]), what
            e = c["expect"]
            if e:                                                    # the hand answer itself
                assert np.array_equal(g["outlier"][i, :n], e["outlier"]), what
                assert (got[0], got[2], g["n_inliers"][i]) == (e["n"], e["rounds"], e["n_inliers"]), what
                if e["untouched"]:
                    assert np.array_equal(g["T"][i], c["T0"]) and got[3:] == (0, 0), what
                if e.get("round_trip"):                              # a dozen roundings of numbers below 1
                    assert np.abs(g["T"][i] - PC.quaternion_round_trip(c["T0"])).max() <= 1e-15, what
    print(f"waves {waves}: largest device-oracle pose difference {worst:.2e}")


def test_track_local_map_with_fewer_than_three_points(rig):
    """Source 2 (TrackLocalMap): PoseOptimization returns before touching anything when mvpMapPoints holds fewer than three points,
    and TrackLocalMap still counts them.  Frame 0: one frame-to-frame match and one local match; frame 1: one local match."""
    trk, cur, cap = rig["trk"], rig["cur"], rig["cap"]
    b = MC.Builder(1701)
    k_local = b.kp(102, 102, 2)
    b.pt(102, 102, 2, b.d[k_local], k_local)
    k_frame = b.kp(442, 302, 2)
    c = b.local_case("two_points", ("fewer_than_three",))
    last = dict(valid=np.ones(1, np.uint8), Xw=np.array([[0.5, 0.25, 2.0]]), desc=np.zeros((1, 32), np.uint8), octave=np.full(1, 2, np.int32),
                angle=np.zeros(1, np.float32), obs=np.ones(1, np.int32))
    match = np.full((2, cap), -1, np.int32)
    match[0, k_frame] = 0
    T = [PC.start(), PC.se3_exp((0.1, 0.0, -0.1), (1.0, 2.0, 3.0))]                 # the local case's points sit in the camera frame: world = camera
    pts = dict(c["pts"])
    cur.set_keypoints(0, [c["kps"]] * 2, [c["desc"]] * 2)
    trk.set_camera(*PC.K, PC.BF, BOUNDS)
    trk.set_uright(0, np.full((2, cap), -1.0, np.float32))
    trk.set_last(0, [last] * 2)
    trk.set_matches(0, match)
    for i in range(2):                                              # move the local point into each frame's world
        p = dict(pts)
        Ti = np.linalg.inv(T[i])
        p["Xw"] = pts["Xw"] @ Ti[:3, :3].T + Ti[:3, 3]
        p["normal"] = pts["normal"] @ Ti[:3, :3].T
        trk.set_local(i, [p])
    trk.set_poses(0, [np.eye(4)] * 2, T)
    for waves in (1, 4):
        with rig["sd"].options({"track.poseopt_waves": waves}):
            trk.set_poses(0, [np.eye(4)] * 2, T)
            trk.track_local_map(2, th=1.0, nnratio=MC.NNRATIO, cos_limit=MC.COS_LIMIT)
            tl, po = trk.get_local_map(0, 2), trk.get_pose_opt(0, 2)
        print(waves, tl["n_points"], tl["n_inliers"], tl["n_local"], tl["status"], po["n_initial"], po["rounds"])
        assert tl["n_points"].tolist() == [2, 1] and tl["n_local"].tolist() == [1, 1] and tl["n_inliers"].tolist() == [2, 1]
        assert tl["status"].tolist() == [1, 1]
        assert tl["match"][0, k_local] == trk.M and tl["match"][0, k_frame] == 0 and tl["match"][1, k_local] == trk.M
        assert po["n_initial"].tolist() == [2, 1] and po["rounds"].tolist() == [0, 0] and not po["outlier"].any()
        for i in range(2):
            assert np.array_equal(po["T"][i], T[i]), (waves, i)
