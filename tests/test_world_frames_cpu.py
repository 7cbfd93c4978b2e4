"""The oracle alone, in world frames far from the identity (tests/world_frames.py): the conditions that
tests/test_world_frames_gpu.py relies on when it compares the device with the oracle there.  A rigid change of world
frame leaves images and keypoints untouched, so in every frame PoseOptimization and PnP RANSAC find the planted truth,
the two projection searches find the matches they find today, ImageAlign converges, and the matrix -> quaternion step
of PoseOptimization equals a longdouble statement of the textbook formula.

Pose bounds are the project's own 5e-3 (tests/test_pnp_ransac.py).  They are asserted on the estimate moved back into
the scene's frame in every frame, on the rotation block in the new frame in every frame, and on the whole pose in the
new frame where t_G = 0: in `far` a rotation error of 3e-4 -- what 210 inliers with half a pixel of noise leave -- times
the 500 m lever arm is 0.05 ... 0.18 m of translation in the new frame, in any implementation (world_frames.pose_error)."""
import numpy as np
import pytest

import pnp_cases as PC
import world_frames as WF
from sdslam_amd import synth

K, BOUNDS = WF.K, WF.BOUNDS


@pytest.fixture(scope="module")
def rig(oracle):
    return WF.oracle_rig(oracle)


@pytest.fixture(scope="module")
def id_counts(oracle, rig):
    """Match counts of the two searches in the scenes' own frame: what every other frame is held against."""
    return [_search(oracle, rig, i, WF.FRAMES["id"]) for i in range(rig["B"])]


def _search(oracle, rig, i, G):
    f, s = rig["fr"][i], rig["scenes"][i]
    n, cm = oracle.search_by_projection(f["ck"], f["cd"], f["tab"]["sf"], BOUNDS, K, WF.move_pose(s["T_cur"], G), WF.move_pose(s["T_ref"], G),
                                        WF.move_last(f["last"], G), th=8.0, mono=True, check_ori=True)
    r = oracle.search_local_points(f["ck"], f["cd"], f["tab"]["sf"], np.log(np.float32(WF.CFG[1])), BOUNDS, K, 0.0, WF.move_pose(s["T_cur"], G),
                                   WF.move_local(f["local"], G), th=1.0, nnratio=0.8)
    return n, r["n"]


def test_frames_reach_every_quaternion_branch(rig):
    """From the perturbed start the sweep takes all four branches of the conversion; from the old-frame identity the two
    exact frames hit the `t > 0` boundary and the diagonal ties."""
    T0 = WF.START @ rig["scenes"][0]["T_cur"]
    got = {n: WF.quat_branch(WF.move_pose(T0, G)[:3, :3]) for n, G in WF.FRAMES.items()}
    assert {got["id"], got["rx170"], got["ry170"], got["rz170"], got["far"]} == {"w", "x", "y", "z"} and got["rx170"] == "x", got
    for n in WF.EXACT_TIES:
        R = WF.move_pose(np.eye(4), WF.FRAMES[n])[:3, :3]
        assert R[0, 0] == R[1, 1] == 0.0 and np.trace(R) <= 0.0 and WF.quat_branch(R) == "x", n


@pytest.mark.parametrize("name", WF.NAMES)
def test_pose_optimization_finds_the_planted_truth(oracle, rig, name):
    G = WF.FRAMES[name]
    for i in range(rig["B"]):
        f, T_true = rig["fr"][i], rig["scenes"][i]["T_cur"]
        last, cm, truth = WF.planted_case(rig, i)
        Xw = WF.matched_points(WF.move_last(last, G), cm)
        starts = [WF.START @ T_true] + ([np.eye(4)] if name in WF.EXACT_TIES else [])
        for T0 in starts:
            for ur in (None, WF.planted_uright(rig, i, last, cm, truth)):
                r = oracle.pose_optimization(f["ck"], cm >= 0, Xw, f["tab"]["inv_sigma2"], K, WF.move_pose(T0, G), u_right=ur,
                                             bf=40.0 if ur is not None else 0.0)
                print(name, i, "stereo" if ur is not None else "mono", "pose error (new frame, scene's frame):", WF.pose_error(r["T"], T_true, G))
                WF.assert_converged(r["T"], T_true, G, (name, i))
                assert not (truth & r["outlier"]).any() and r["outlier"][(cm >= 0) & ~truth].mean() > 0.95, (name, i)


@pytest.fixture(scope="module")
def frame1000(oracle):
    """tests/test_pnp_ransac.py's frame: the scenarios keep their own match counts (up to 400) on its 1000 keypoints."""
    s = synth.make_scene(20)
    oc = oracle.OrbOracle(1000, 1.2, 8, 20)
    ck, _ = oc.extract(s["cur"])
    return dict(T_cur=s["T_cur"], ck=ck, sigma2=oc.tables()["sigma2"])


@pytest.mark.parametrize("scenario", ["out30_c4", "out65_chunked"])       # shallow: accepted after a few hypotheses; deep: 65 % outliers
@pytest.mark.parametrize("name", WF.NAMES)
def test_pnp_ransac_finds_the_planted_truth(oracle, frame1000, name, scenario):
    G = WF.FRAMES[name]
    kw, params, calls = PC.SCENARIOS[scenario]
    last, cm, truth = PC.planted(7, frame1000["ck"], frame1000["T_cur"], **kw)
    rs = synth.glibc_rand_stream(PC.rand_needed(params, calls))
    res, _ = PC.run_oracle(oracle, frame1000["ck"], frame1000["sigma2"], WF.move_last(last, G), cm, params, calls, rs)
    assert all(r["ok"] for r in res), (name, scenario)
    for k, r in enumerate(res):
        print(name, scenario, k, r["iterations"], r["n_inliers"], "pose error (new frame, scene's frame):", WF.pose_error(r["T"], frame1000["T_cur"], G))
        assert not (r["inliers"] & ~truth).any() and r["inliers"].sum() >= 0.9 * truth.sum(), (name, scenario, k)
        WF.assert_converged(r["T"].astype(np.float64), frame1000["T_cur"], G, (name, scenario, k))


@pytest.mark.parametrize("name", WF.NAMES)
def test_searches_keep_their_match_counts(oracle, rig, id_counts, name):
    """Rounding at a window edge may move a match: at most 2 % of the count in the scenes' own frame may go missing."""
    for i in range(rig["B"]):
        got = _search(oracle, rig, i, WF.FRAMES[name])
        print(name, i, "SearchByProjection / local-map matches:", got, "in id:", id_counts[i])
        for n, n_id in zip(got, id_counts[i]):
            assert n_id >= 150 and n >= n_id - 0.02 * n_id, (name, i, n, n_id)


@pytest.mark.parametrize("name", WF.NAMES)
def test_image_align_converges(oracle, rig, name):
    G = WF.FRAMES[name]
    for i in range(rig["B"]):
        f, s = rig["fr"][i], rig["scenes"][i]
        lastp = WF.move_last(f["last"], G)
        for mode in (0, 2, 3):
            r = oracle.align(f["pc"], f["pr"], f["tab"]["inv_sf"], f["tab"]["sf"], lastp["Xw"][lastp["valid"] != 0], WF.move_pose(s["T_ref"], G),
                             WF.move_pose(WF.START @ s["T_cur"], G), K, mode=mode)
            assert r["ok"], (name, i, mode)
            if mode != 3:       # (mode 3 accepts or rejects a loop candidate; it returns no pose)
                WF.assert_converged(r["T"], s["T_cur"], G, (name, i, mode))


@pytest.mark.parametrize("name", WF.NAMES)
def test_quaternion_step_known_answer(oracle, rig, name):
    """PoseOptimization on three exact correspondences whose optimum is the start pose (fewer than three return the pose
    without the round trip): the returned rotation is the start's after matrix -> quaternion -> matrix, within 1e-12 of
    the longdouble round trip -- a dozen fp64 operations on unit-size numbers.  The translation does not pass through the
    quaternion; it moves by the Levenberg steps that the rounding of the world points to fp64 leaves, |X'| eps / z
    pixels, i.e. it is known to 1e-12 times the size of t' (measured: 1.6e-15 where |t'| < 1, 1.1e-11 in `far`)."""
    G = WF.FRAMES[name]
    starts = [WF.START @ rig["scenes"][0]["T_cur"], np.eye(4)]
    for T0 in starts:
        T0p = WF.move_pose(T0, G)
        kp, Xw = WF.exact_three_edges(T0p)
        r = oracle.pose_optimization(kp, np.ones(3, bool), Xw, np.ones(WF.CFG[2], np.float32), K, T0p)
        assert r["n_inliers"] == 3 and r["info"][2] == 1          # one round of optimisation ran: the conversion was taken
        want = WF.round_trip_longdouble(T0p[:3, :3])
        dR = float(np.abs(r["T"][:3, :3].astype(np.longdouble) - want).max())
        dt = np.abs(r["T"][:3, 3] - T0p[:3, 3]).max()
        print(name, WF.quat_branch(T0p[:3, :3]), "rotation vs longdouble round trip:", dR, "translation:", dt)
        assert dR <= 1e-12, (name, dR)
        assert dt <= 1e-12 * max(1.0, np.abs(T0p[:3, 3]).max()), (name, dt)
