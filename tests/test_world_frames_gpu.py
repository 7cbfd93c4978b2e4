"""GPU parity of the pose solvers and matchers in world frames far from the identity (tests/world_frames.py).  Every
other tracking test plants its data around T_ref = I and a T_cur half a degree away, so the kernels that take a world pose
have met the oracle only where R ~ I and |t| ~ 0.  Here each stage runs on the same images and keypoints with the world
moved by G (X' = G X, n' = R_G n, T' = T G^-1) and is compared with the oracle called on the same moved inputs: the three
`trace <= 0` branches of k_pose_opt's matrix -> quaternion conversion, its `t > 0` boundary and strict `>` ties, EPnP's
PCA of world points that do not lie in the camera's axes, and projections whose t cancels against R X.
tests/test_world_frames_cpu.py shows that the oracle alone meets the first-principles bounds used here."""
import numpy as np
import pytest

import pnp_cases as PC
import world_frames as WF
from sdslam_amd import synth

pytestmark = pytest.mark.gpu
K, BOUNDS, MP = WF.K, WF.BOUNDS, WF.MP
POSE_TOL = 1e-5


@pytest.fixture(scope="module")
def rig(oracle):
    import sdslam_amd as sd
    if sd.device_count() < 1:
        pytest.fail("no HIP device: the gpu-marked tests need a real MI355X")
    r = WF.oracle_rig(oracle)
    B, scenes, fr = r["B"], r["scenes"], r["fr"]
    cur, ref = sd.ORBextractor(*WF.CFG, 640, 480, B), sd.ORBextractor(*WF.CFG, 640, 480, B)
    ck, cd, cn = cur.extract_batch(np.stack([s["cur"] for s in scenes]))
    rk, rd, rn = ref.extract_batch(np.stack([s["ref"] for s in scenes]))
    for i in range(B):      # the oracle's extraction equals the device's, once
        assert np.array_equal(fr[i]["ck"], ck[i, :cn[i]]) and np.array_equal(fr[i]["cd"], cd[i, :cn[i]])
        assert np.array_equal(fr[i]["rk"], rk[i, :rn[i]]) and np.array_equal(fr[i]["rd"], rd[i, :rn[i]])
    trk = sd.Tracker(cur, ref, max_points=MP, max_batch=B, pnp_max_iterations=512)
    r.update(sd=sd, trk=trk, cap=ck.shape[1])
    _restore(r)
    yield r
    trk.close()
    cur.close()
    ref.close()


def _restore(rig):
    """Camera, last frames, local maps, right coordinates and poses as the fixture leaves them (the scenes' own frame)."""
    trk, B = rig["trk"], rig["B"]
    trk.set_camera(*K, 0.0, BOUNDS)
    trk.stereo_from_depth(np.zeros((B, 480, 640), np.float32))      # resets every mvuRight to -1
    trk.set_last(0, [f["last"] for f in rig["fr"]])
    trk.set_local(0, [f["local"] for f in rig["fr"]])
    trk.set_poses(0, [s["T_ref"] for s in rig["scenes"]], [s["T_cur"] for s in rig["scenes"]])


def _poses(rig, G, T_cur=None):
    """Both pose lists of the batch in the frame; T_cur defaults to the scenes' true poses."""
    T_cur = [s["T_cur"] for s in rig["scenes"]] if T_cur is None else T_cur
    return [WF.move_pose(s["T_ref"], G) for s in rig["scenes"]], [WF.move_pose(T, G) for T in T_cur]


@pytest.mark.parametrize("name", WF.NAMES)
def test_pose_optimization(oracle, rig, name):
    """The planted 30 %-outlier vector through set_matches, one and four waves per frame, mono and with planted uRight,
    from the perturbed start -- and, in the two exact frames, from the old-frame identity, whose rotation is the tie
    matrix.  Identical flags and counts, pose within 1e-5 of the oracle's, and the device's own result within the
    first-principles bounds."""
    G, trk, B, fr = WF.FRAMES[name], rig["trk"], rig["B"], rig["fr"]
    cases = [WF.planted_case(rig, i) for i in range(B)]
    moved = [WF.move_last(c[0], G) for c in cases]
    T_true = [s["T_cur"] for s in rig["scenes"]]
    starts = [("perturbed", [WF.START @ T for T in T_true])] + ([("identity", [np.eye(4)] * B)] if name in WF.EXACT_TIES else [])
    worst = 0.0
    try:
        trk.set_last(0, moved)
        for stereo in (False, True):
            ur = np.full((B, rig["cap"]), -1, np.float32)
            if stereo:
                for i in range(B):
                    ur[i, :len(fr[i]["ck"])] = WF.planted_uright(rig, i, *cases[i])
                trk.set_camera(*K, 40.0, BOUNDS)
                trk.set_uright(0, ur)
            for start, T0 in starts:
                T_ref_p, T0_p = _poses(rig, G, T0)
                want = []
                for i in range(B):
                    n = len(fr[i]["ck"])
                    want.append(oracle.pose_optimization(fr[i]["ck"], cases[i][1] >= 0, WF.matched_points(moved[i], cases[i][1]),
                                                         fr[i]["tab"]["inv_sigma2"], K, T0_p[i], u_right=ur[i, :n] if stereo else None,
                                                         bf=40.0 if stereo else 0.0))
                for waves in (1, 4):
                    trk.set_matches(0, np.stack([c[1] for c in cases]))
                    trk.set_poses(0, T_ref_p, T0_p)
                    with rig["sd"].options({"track.poseopt_waves": waves}):
                        trk.pose_opt(B, 0)
                        g = trk.get_pose_opt(0, B)
                    for i in range(B):
                        key, r, n, (_, cm, truth) = (name, stereo, start, waves, i), want[i], len(fr[i]["ck"]), cases[i]
                        d = np.abs(g["T"][i] - r["T"]).max()
                        worst = max(worst, d)
                        assert np.array_equal(g["outlier"][i, :n], r["outlier"]) and not g["outlier"][i, n:].any(), key
                        assert (g["n_inliers"][i], g["n_initial"][i], g["n_bad"][i]) == (r["n_inliers"], r["info"][0], r["info"][1]), key
                        assert d <= POSE_TOL, (key, d)
                        WF.assert_converged(g["T"][i], T_true[i], G, key)
                        out = g["outlier"][i, :n]
                        assert not (truth & out).any() and out[(cm >= 0) & ~truth].mean() > 0.95, key
        print(f"pose_opt {name}: largest device-oracle pose difference {worst:.3e}")
    finally:
        _restore(rig)


@pytest.mark.parametrize("scenario", ["out30_c4", "out65_chunked"])       # one that refines at once; one re-entered in chunks
@pytest.mark.parametrize("name", WF.NAMES)
def test_pnp_ransac(oracle, rig, name, scenario):
    G, trk, B, fr = WF.FRAMES[name], rig["trk"], rig["B"], rig["fr"]
    cases, moved = [], []
    for i in range(B):
        kw, params, calls = WF.pnp_scenario(scenario, len(fr[i]["ck"]))
        cases.append(PC.planted(7 + i, fr[i]["ck"], rig["scenes"][i]["T_cur"], **kw))
        moved.append(WF.move_last(cases[i][0], G))
    rs = synth.glibc_rand_stream(PC.rand_needed(params, calls))
    worst = 0.0
    try:
        trk.set_last(0, moved)
        trk.set_matches(0, np.stack([c[1] for c in cases]))
        trk.set_rand(0, np.tile(rs, (B, 1)))
        got = []
        for k, n_it in enumerate(calls):
            if k == 0:
                trk.pnp(B, *params, n_it)
            else:
                trk.pnp_iterate(B, n_it)
            got.append(trk.get_pnp(0, B))
        for i in range(B):
            n = len(fr[i]["ck"])
            res, pr = PC.run_oracle(oracle, fr[i]["ck"], fr[i]["tab"]["sigma2"], moved[i], cases[i][1], params, calls, rs)
            for k, r in enumerate(res):
                g, key = got[k], (name, scenario, i, k)
                assert (g["N"][i], g["min_inliers"][i], g["max_its"][i]) == (pr["N"], pr["min_inliers"], pr["max_its"]), key
                assert (bool(g["ok"][i]), int(g["iterations"][i]), int(g["n_inliers"][i]), bool(g["no_more"][i])) == \
                    (r["ok"], r["iterations"], r["n_inliers"], r["no_more"]), key
                assert bool(g["refined"][i]) == (r["ok"] and not r["no_more"]), key
                assert np.array_equal(g["inliers"][i, :n], r["inliers"]), key
                d = np.abs(g["T"][i] - r["T"]).max()
                worst = max(worst, d)
                assert d <= POSE_TOL, (key, d)
        print(f"pnp {name} {scenario}: largest device-oracle pose difference {worst:.3e}")
    finally:
        _restore(rig)


@pytest.mark.parametrize("name", WF.NAMES)
def test_epnp_alone(oracle, rig, name):
    """compute_pose through debug_epnp on the trials of test_epnp_device_vs_oracle; that test's absolute 1e-9 was set for
    |t| ~ 1 and scales with the size of t' here."""
    from sdslam_amd.capi import debug_epnp
    worst = 0.0
    for trial, (Xw, uv, Tp) in enumerate(WF.epnp_trials(WF.FRAMES[name])):
        tol = 1e-9 * max(1.0, np.abs(Tp[:3, 3]).max())
        R, t, e = oracle.epnp(Xw, uv, K)
        Rg, tg, eg = debug_epnp(Xw, uv, K)
        d = max(np.abs(R - Rg).max(), np.abs(t - tg).max())
        worst = max(worst, d)
        assert d <= tol, (name, trial, len(Xw), d, tol)
    print(f"epnp {name}: largest device-oracle difference {worst:.3e}")


def _depth(B):
    yy, xx = np.mgrid[0:480, 0:640].astype(np.float32)
    depth = np.stack([(1.5 + 0.8 * np.sin(xx * 0.013 + i) * np.cos(yy * 0.017)).astype(np.float32) for i in range(B)])
    depth[:, 100:140, :] = 0.0            # holes: no depth -> mvuRight = -1
    return depth


@pytest.mark.parametrize("name", WF.NAMES)
def test_search_by_projection(oracle, rig, name):
    """SearchByProjection(Frame, Frame) as two kernels and as one, mono, and once on RGB-D frames (the forward / backward
    gate reads Tlc = Tcur Tlast^-1): match vector and count equal the oracle's."""
    G, trk, B, fr, sd = WF.FRAMES[name], rig["trk"], rig["B"], rig["fr"], rig["sd"]
    moved = [WF.move_last(f["last"], G) for f in fr]
    T_ref_p, T_cur_p = _poses(rig, G)
    bf = 40.0
    mb = np.float32(bf) / np.float32(K[0])
    try:
        trk.set_last(0, moved)
        trk.set_poses(0, T_ref_p, T_cur_p)
        runs = [(1, True), (0, True), (1, False)]
        for split, mono in runs:
            urs = [None] * B
            if not mono:
                depth = _depth(B)
                trk.set_camera(*K, bf, BOUNDS)
                trk.stereo_from_depth(depth)
                ur, _ = trk.get_stereo(0, B)
                for i in range(B):
                    urs[i], _ = oracle.stereo_from_rgbd(fr[i]["ck"], fr[i]["ck"], depth[i], bf)
                    assert np.array_equal(ur[i, :len(urs[i])], urs[i]) and (urs[i] > 0).any() and (urs[i] == -1).any()
            with sd.options({"track.match_split": split}):
                trk.match(B, th=8.0, mono=mono, check_ori=True)
            cm, nm = trk.get_matches(0, B)
            for i in range(B):
                kw = {} if mono else dict(u_right=urs[i], mbf=bf, mb=mb)
                n, ocm = oracle.search_by_projection(fr[i]["ck"], fr[i]["cd"], fr[i]["tab"]["sf"], BOUNDS, K, T_cur_p[i], T_ref_p[i], moved[i], th=8.0,
                                                     mono=mono, check_ori=True, **kw)
                assert nm[i] == n, (name, split, mono, i, nm[i], n)
                assert np.array_equal(cm[i, :len(ocm)], ocm) and (cm[i, len(ocm):] == -1).all(), (name, split, mono, i)
                assert n >= 100
    finally:
        _restore(rig)


@pytest.mark.parametrize("name", WF.NAMES)
def test_local_map_search(oracle, rig, name):
    """isInFrustum (camera centre -R^T t, view cosine against the moved normals), PredictScale and the search: every
    output equals the oracle's."""
    G, trk, B, fr = WF.FRAMES[name], rig["trk"], rig["B"], rig["fr"]
    moved = [WF.move_local(f["local"], G) for f in fr]
    T_ref_p, T_cur_p = _poses(rig, G)
    try:
        trk.set_poses(0, T_ref_p, T_cur_p)
        trk.set_local(0, moved)
        trk.match_local(B, th=1.0, nnratio=0.8)
        g = trk.get_local(0, B)
        for i in range(B):
            n, M = len(fr[i]["ck"]), len(moved[i]["cand"])
            r = oracle.search_local_points(fr[i]["ck"], fr[i]["cd"], fr[i]["tab"]["sf"], np.log(np.float32(WF.CFG[1])), BOUNDS, K, 0.0, T_cur_p[i],
                                           moved[i], th=1.0, nnratio=0.8)
            assert np.array_equal(g["in_view"][i, :M], r["in_view"]), (name, i)
            assert np.array_equal(g["proj"][i, :M], r["proj"]) and np.array_equal(g["level"][i, :M], r["level"]), (name, i)
            assert np.array_equal(g["cos"][i, :M], r["cos"]), (name, i)
            assert g["n"][i] == r["n"], (name, i, g["n"][i], r["n"])
            assert np.array_equal(g["match"][i, :n], r["match"]) and (g["match"][i, n:] == -1).all(), (name, i)
            assert r["n"] >= 150 and r["in_view"].sum() < M          # and some points fail isInFrustum
    finally:
        _restore(rig)


@pytest.mark.parametrize("name", WF.NAMES)
def test_image_align(oracle, rig, name):
    """ImageAlign from the perturbed start in modes 0 (frame), 2 (keyframe, fast) and 3 (keyframe against keyframe): what
    test_image_align_matches_oracle and test_image_align_modes compare, to their tolerances."""
    G, trk, B, fr = WF.FRAMES[name], rig["trk"], rig["B"], rig["fr"]
    moved = [WF.move_last(f["last"], G) for f in fr]
    T_ref_p, T0_p = _poses(rig, G, [WF.START @ s["T_cur"] for s in rig["scenes"]])
    worst = 0.0
    try:
        trk.set_last(0, moved)
        for mode in (0, 2, 3):
            trk.set_poses(0, T_ref_p, T0_p)
            trk.align(B, mode=mode)
            g = trk.get_align(0, B)
            for i in range(B):
                key = (name, mode, i)
                r = oracle.align(fr[i]["pc"], fr[i]["pr"], fr[i]["tab"]["inv_sf"], fr[i]["tab"]["sf"], moved[i]["Xw"][moved[i]["valid"] != 0],
                                 T_ref_p[i], T0_p[i], K, mode=mode)
                assert g["ok"][i] == r["ok"] and r["ok"], key
                assert np.array_equal(g["iters"][i][:len(r["iters"])], r["iters"]), (key, g["iters"][i][:len(r["iters"])], r["iters"])
                if mode != 3:
                    d = np.abs(g["T"][i] - r["T"]).max()
                    worst = max(worst, d)
                    assert d <= POSE_TOL, (key, d)
                else:
                    assert np.abs(g["T"][i] - T0_p[i]).max() == 0      # pose untouched
                assert abs(g["error"][i] - r["error"]) <= 1e-7 * max(1.0, abs(r["error"])), key
                if mode == 0:
                    assert abs(g["chi2"][i] - r["chi2"]) <= 1e-9 * max(1.0, abs(r["chi2"])), key
        print(f"align {name}: largest device-oracle pose difference {worst:.3e}")
    finally:
        _restore(rig)


@pytest.mark.parametrize("name", ["ry170", "far"])
def test_motion_model_then_local_map(oracle, rig, name):
    """TrackWithMotionModel and TrackLocalMap chained on the device, as test_track_with_motion_model_decisions and
    test_track_local_map_after_motion_model run them, in two frames."""
    G, trk, B, fr = WF.FRAMES[name], rig["trk"], rig["B"], rig["fr"]
    log_sf = np.log(np.float32(WF.CFG[1]))
    lasts = [WF.move_last(f["last"], G) for f in fr]
    for i, l in enumerate(lasts):       # a third of the last frame's points are not in the map yet
        l["obs"] = (np.arange(len(l["obs"])) % 3 != i % 3).astype(np.int32)
    locals_ = [WF.move_local(f["local"], G) for f in fr]
    T_ref_p, T0_p = _poses(rig, G, [WF.START @ s["T_cur"] for s in rig["scenes"]])
    try:
        trk.set_last(0, lasts)
        trk.set_local(0, locals_)
        trk.set_poses(0, T_ref_p, T0_p)
        trk.align(B, 0)             # the device's aligned poses: the matcher is compared on these
        T_al = trk.get_align(0, B)["T"]
        trk.set_poses(0, T_ref_p, T0_p)
        trk.track_with_motion_model(B, th=8.0, mono=True, align_mode=0)
        tw, gp, (fm, nm), ga = trk.get_tracked(0, B), trk.get_pose_opt(0, B), trk.get_matches(0, B), trk.get_align(0, B)
        T_mm = gp["T"]
        for i in range(B):
            n, key = len(fr[i]["ck"]), (name, "motion model", i)
            r = oracle.track_with_motion_model(fr[i]["pc"], fr[i]["pr"], fr[i]["tab"], fr[i]["ck"], fr[i]["cd"], BOUNDS, K, T_ref_p[i], T0_p[i], lasts[i],
                                               8.0, mono=True, align_mode=0, T_aligned=T_al[i])
            assert (tw["status"][i], tw["retried"][i], tw["nmatches"][i], tw["nmatches_map"][i]) == \
                (r["status"], r["retried"], r["nmatches"], r["nmatches_map"]), key
            assert np.array_equal(fm[i, :n], r["match"]) and (fm[i, n:] == -1).all(), key
            assert np.abs(gp["T"][i] - r["T"]).max() <= POSE_TOL, (key, np.abs(gp["T"][i] - r["T"]).max())
            assert np.abs(ga["T"][i] - r["T"]).max() <= POSE_TOL and not gp["outlier"][i].any(), key
            assert r["status"] == 2
            WF.assert_converged(gp["T"][i], rig["scenes"][i]["T_cur"], G, key)
        trk.track_local_map(B, th=1.0, min_inliers=30)
        g, gp, gl = trk.get_local_map(0, B), trk.get_pose_opt(0, B), trk.get_local(0, B)
        for i in range(B):
            n, key = len(fr[i]["ck"]), (name, "local map", i)
            r = oracle.track_local_map(fr[i]["ck"], fr[i]["cd"], fr[i]["tab"], log_sf, BOUNDS, K, T_mm[i], fm[i, :n], lasts[i], locals_[i], th=1.0,
                                       min_inliers=30)
            assert np.array_equal(gl["match"][i, :n], r["local_match"]), key
            want = np.where(r["local_match"] >= 0, r["local_match"] + MP, r["frame_match"])
            assert np.array_equal(g["match"][i, :n], want) and (g["match"][i, n:] == -1).all(), key
            assert g["n_points"][i] == r["n_points"] and g["n_local"][i] == r["n_local"], key
            assert np.array_equal(gp["outlier"][i, :n], r["outlier"]), key
            assert g["n_inliers"][i] == r["n_inliers"] and g["status"][i] == r["status"], (key, g["n_inliers"][i], r["n_inliers"])
            assert np.abs(gp["T"][i] - r["T"]).max() <= POSE_TOL, (key, np.abs(gp["T"][i] - r["T"]).max())
            assert r["n_local"] > 100 and r["status"] == 2
    finally:
        _restore(rig)
