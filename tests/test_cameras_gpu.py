"""GPU parity of the tracking kernels under cameras other than synth's (tests/cameras.py).  Every other tracking test sets
fx = fy = 500, the principal point at the image centre and bounds (0, 640, 0, 480), so fx and fy, cx and cy, invW and invH
and `x - min_x` and `x` have never been told apart on the device, no keypoint has ever been outside the frame grid, and no
matcher or pose solver has seen undistorted keypoints.  Here each stage runs under each camera on the images that camera
sees and is compared with the oracle called on the same inputs and the same float-rounded camera.
tests/test_cameras_cpu.py shows that the cases are sound and that a device using a wrong camera would differ here."""
import numpy as np
import pytest

import cameras as CM
import pnp_cases as PC
from sdslam_amd import synth

pytestmark = pytest.mark.gpu
POSE_TOL = 1e-5
MP = CM.MP
LOG_SF = np.log(np.float32(CM.CFG[1]))


@pytest.fixture(scope="module")
def rigs(oracle):
    """name -> rig, built on first use: the oracle's rig of the camera, two extractors (with the camera's distortion) holding
    the two scenes, and a tracker.  The oracle's extraction and undistorted keypoints equal the device's, asserted once."""
    import sdslam_amd as sd
    if sd.device_count() < 1:
        pytest.fail("no HIP device: the gpu-marked tests need a real MI355X")
    built = {}

    def get(name):
        if name in built:
            return built[name]
        r = dict(CM.oracle_rig(oracle, name))
        cam, B, scenes, fr = r["cam"], r["B"], r["scenes"], r["fr"]
        cur, ref = sd.ORBextractor(*CM.CFG, CM.W, CM.H, B), sd.ORBextractor(*CM.CFG, CM.W, CM.H, B)
        if cam.dist is not None:
            for e in (cur, ref):
                e.set_distortion(*cam.K, *cam.dist)
        ck, cd, cn = cur.extract_batch(np.stack([s["cur"] for s in scenes]))
        rk, rd, rn = ref.extract_batch(np.stack([s["ref"] for s in scenes]))
        cu, ru = cur.download_undistorted(0, B), ref.download_undistorted(0, B)
        for i in range(B):
            assert np.array_equal(fr[i]["ck_raw"], ck[i, :cn[i]]) and np.array_equal(fr[i]["cd"], cd[i, :cn[i]]), (name, i)
            assert np.array_equal(fr[i]["rk_raw"], rk[i, :rn[i]]) and np.array_equal(fr[i]["rd"], rd[i, :rn[i]]), (name, i)
            assert np.array_equal(fr[i]["ck"], cu[i, :cn[i]]) and np.array_equal(fr[i]["rk"], ru[i, :rn[i]]), (name, i)
        trk = sd.Tracker(cur, ref, max_points=MP, max_batch=B, pnp_max_iterations=512)
        r.update(sd=sd, trk=trk, ext=(cur, ref), cap=ck.shape[1])
        _restore(r)
        built[name] = r
        return r

    yield get
    for r in built.values():
        r["trk"].close()
        for e in r["ext"]:
            e.close()


def _restore(rig):
    """Camera, last frames, local maps, right coordinates and poses as the fixture leaves them."""
    trk, B, cam = rig["trk"], rig["B"], rig["cam"]
    trk.set_camera(*cam.K, 0.0, cam.bounds)
    trk.stereo_from_depth(np.zeros((B, CM.H, CM.W), np.float32))      # resets every mvuRight to -1
    trk.set_last(0, [f["last"] for f in rig["fr"]])
    trk.set_local(0, [f["local"] for f in rig["fr"]])
    trk.set_poses(0, [s["T_ref"] for s in rig["scenes"]], [s["T_cur"] for s in rig["scenes"]])


def _refs(rig):
    return [s["T_ref"] for s in rig["scenes"]]


def _starts(rig):
    return [CM.START @ s["T_cur"] for s in rig["scenes"]]


@pytest.mark.parametrize("name", CM.NAMES)
def test_image_align(oracle, rigs, name):
    """ImageAlign from the perturbed start in modes 0 (frame), 1 (keyframe) and 3 (keyframe against keyframe): ok and per-level
    iterations equal, error to a relative 1e-7, pose within 1e-5.  Under aniso and window the fx-only scale of the reference's
    Jacobian is followed, not repaired: the oracle has it."""
    rig = rigs(name)
    trk, B, fr, cam = rig["trk"], rig["B"], rig["fr"], rig["cam"]
    worst, worst_e = 0.0, 0.0
    try:
        for mode in (0, 1, 3):
            trk.set_poses(0, _refs(rig), _starts(rig))
            trk.align(B, mode=mode)
            g = trk.get_align(0, B)
            for i in range(B):
                key = (name, mode, i)
                last = fr[i]["last"]
                r = oracle.align(fr[i]["pc"], fr[i]["pr"], fr[i]["tab"]["inv_sf"], fr[i]["tab"]["sf"], last["Xw"][last["valid"] != 0],
                                 rig["scenes"][i]["T_ref"], _starts(rig)[i], cam.K, mode=mode)
                assert g["ok"][i] == r["ok"] and r["ok"], key
                assert np.array_equal(g["iters"][i][:len(r["iters"])], r["iters"]), (key, g["iters"][i][:len(r["iters"])], r["iters"])
                if mode != 3:
                    d = np.abs(g["T"][i] - r["T"]).max()
                    worst = max(worst, d)
                    assert d <= POSE_TOL, (key, d)
                else:
                    assert np.abs(g["T"][i] - _starts(rig)[i]).max() == 0      # pose untouched
                e = abs(g["error"][i] - r["error"]) / max(1.0, abs(r["error"]))
                worst_e = max(worst_e, e)
                assert e <= 1e-7, (key, e)
        print(f"align {name}: largest device-oracle pose difference {worst:.3e}, relative error difference {worst_e:.3e}")
    finally:
        _restore(rig)


def _planted_cur_uright(rig, i, bf):
    """mvuRight for every third current keypoint from the depth of the surface point it sees; -1 for the others."""
    f, T, cam = rig["fr"][i], rig["scenes"][i]["T_cur"], rig["cam"]
    Xw = CM.keyframe_case(f["ck"], f["cd"], T, cam)["Xw"]
    zc = (Xw @ T[:3, :3].T + T[:3, 3])[:, 2]
    return np.where(np.arange(len(zc)) % 3 == 0, f["ck"]["x"] - bf / zc, -1.0).astype(np.float32)


@pytest.mark.parametrize("name", CM.NAMES)
def test_search_by_projection(oracle, rigs, name):
    """SearchByProjection(Frame, Frame), mono and with planted uRight and bf = 40, th = 8 and th = 1: the match vector and the
    count equal the oracle's."""
    rig = rigs(name)
    trk, B, fr, cam = rig["trk"], rig["B"], rig["fr"], rig["cam"]
    bf = CM.BF
    mb = np.float32(bf) / np.float32(cam.K[0])
    T_cur = [s["T_cur"] for s in rig["scenes"]]
    try:
        for mono in (True, False):
            urs = [None] * B
            if not mono:
                ur = np.full((B, rig["cap"]), -1, np.float32)
                for i in range(B):
                    urs[i] = _planted_cur_uright(rig, i, bf)
                    ur[i, :len(urs[i])] = urs[i]
                trk.set_camera(*cam.K, bf, cam.bounds)
                trk.set_uright(0, ur)
            for th in (8.0, 1.0):
                trk.set_poses(0, _refs(rig), T_cur)
                trk.match(B, th=th, mono=mono, check_ori=True)
                cm, nm = trk.get_matches(0, B)
                for i in range(B):
                    kw = {} if mono else dict(u_right=urs[i], mbf=bf, mb=mb)
                    n, ocm = oracle.search_by_projection(fr[i]["ck"], fr[i]["cd"], fr[i]["tab"]["sf"], cam.bounds, cam.K, T_cur[i],
                                                         rig["scenes"][i]["T_ref"], fr[i]["last"], th=th, mono=mono, check_ori=True, **kw)
                    assert nm[i] == n, (name, mono, th, i, nm[i], n)
                    assert np.array_equal(cm[i, :len(ocm)], ocm) and (cm[i, len(ocm):] == -1).all(), (name, mono, th, i)
                    assert n >= (150 if th == 8.0 else 20), (name, mono, th, i, n)
    finally:
        _restore(rig)


@pytest.mark.parametrize("name", CM.NAMES)
def test_local_map_search(oracle, rigs, name):
    """isInFrustum (its bounds test included: under window, points inside the image are rejected), PredictScale and the
    search: every output equals the oracle's."""
    rig = rigs(name)
    trk, B, fr, cam = rig["trk"], rig["B"], rig["fr"], rig["cam"]
    try:
        trk.match_local(B, th=1.0, nnratio=0.8)
        g = trk.get_local(0, B)
        for i in range(B):
            n, M = len(fr[i]["ck"]), len(fr[i]["local"]["cand"])
            r = oracle.search_local_points(fr[i]["ck"], fr[i]["cd"], fr[i]["tab"]["sf"], LOG_SF, cam.bounds, cam.K, 0.0, rig["scenes"][i]["T_cur"],
                                           fr[i]["local"], th=1.0, nnratio=0.8)
            assert np.array_equal(g["in_view"][i, :M], r["in_view"]), (name, i)
            assert np.array_equal(g["proj"][i, :M], r["proj"]) and np.array_equal(g["level"][i, :M], r["level"]), (name, i)
            assert np.array_equal(g["cos"][i, :M], r["cos"]), (name, i)
            assert g["n"][i] == r["n"], (name, i, g["n"][i], r["n"])
            assert np.array_equal(g["match"][i, :n], r["match"]) and (g["match"][i, n:] == -1).all(), (name, i)
            assert r["n"] >= 150 and r["in_view"].sum() < M
    finally:
        _restore(rig)


@pytest.mark.parametrize("name", CM.NAMES)
def test_features_in_area(oracle, rigs, name):
    """Frame::GetFeaturesInArea on the device grid for cameras.area_queries: the index lists are identical and in order."""
    rig = rigs(name)
    trk, fr, cam = rig["trk"], rig["fr"], rig["cam"]
    total = 0
    for i in range(rig["B"]):
        for q in CM.area_queries(cam):
            got = trk.features_in_area(i, *q)
            want = oracle.features_in_area(fr[i]["ck"], cam.bounds, *q)
            assert np.array_equal(got, want), (name, i, q, got, want)
            total += len(want)
    assert total > 100, (name, total)


@pytest.mark.parametrize("name", CM.NAMES)
def test_pose_optimization(oracle, rigs, name):
    """The planted 30 %-outlier vector, one and four waves per frame, mono and with planted uRight, from the perturbed start:
    identical flags and counts, pose within 1e-5 of the oracle's."""
    rig = rigs(name)
    trk, B, fr, cam = rig["trk"], rig["B"], rig["fr"], rig["cam"]
    cases = [CM.planted_case(rig, i) for i in range(B)]
    worst = 0.0
    try:
        trk.set_last(0, [c[0] for c in cases])
        for stereo in (False, True):
            ur = np.full((B, rig["cap"]), -1, np.float32)
            if stereo:
                for i in range(B):
                    ur[i, :len(fr[i]["ck"])] = CM.planted_uright(rig, i, *cases[i])
                trk.set_camera(*cam.K, CM.BF, cam.bounds)
                trk.set_uright(0, ur)
            want = []
            for i in range(B):
                n = len(fr[i]["ck"])
                want.append(oracle.pose_optimization(fr[i]["ck"], cases[i][1] >= 0, CM.matched_points(cases[i][0], cases[i][1]),
                                                     fr[i]["tab"]["inv_sigma2"], cam.K, _starts(rig)[i], u_right=ur[i, :n] if stereo else None,
                                                     bf=CM.BF if stereo else 0.0))
            for waves in (1, 4):
                trk.set_matches(0, np.stack([c[1] for c in cases]))
                trk.set_poses(0, _refs(rig), _starts(rig))
                with rig["sd"].options({"track.poseopt_waves": waves}):
                    trk.pose_opt(B, 0)
                    g = trk.get_pose_opt(0, B)
                for i in range(B):
                    key, r, n, (_, cm, truth) = (name, stereo, waves, i), want[i], len(fr[i]["ck"]), cases[i]
                    d = np.abs(g["T"][i] - r["T"]).max()
                    worst = max(worst, d)
                    assert np.array_equal(g["outlier"][i, :n], r["outlier"]) and not g["outlier"][i, n:].any(), key
                    assert (g["n_inliers"][i], g["n_initial"][i], g["n_bad"][i]) == (r["n_inliers"], r["info"][0], r["info"][1]), key
                    assert d <= POSE_TOL, (key, d)
                    out = g["outlier"][i, :n]
                    assert not (truth & out).any() and out[(cm >= 0) & ~truth].mean() > 0.95, key
        print(f"pose_opt {name}: largest device-oracle pose difference {worst:.3e}")
    finally:
        _restore(rig)


@pytest.mark.parametrize("scenario", ["out30_c4", "out65_chunked"])       # one that refines at once; one re-entered in chunks
@pytest.mark.parametrize("name", CM.NAMES)
def test_pnp_ransac(oracle, rigs, name, scenario):
    rig = rigs(name)
    trk, B, fr, cam = rig["trk"], rig["B"], rig["fr"], rig["cam"]
    cases = [CM.pnp_case(rig, i, scenario) for i in range(B)]
    params, calls = cases[0][3], cases[0][4]
    rs = synth.glibc_rand_stream(PC.rand_needed(params, calls))
    worst = 0.0
    try:
        trk.set_last(0, [c[0] for c in cases])
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
            res, pr = CM.run_pnp_oracle(oracle, fr[i]["ck"], fr[i]["tab"]["sigma2"], cases[i][0], cases[i][1], cam.K, params, calls, rs)
            for k, r in enumerate(res):
                g, key = got[k], (name, scenario, i, k)
                assert (g["N"][i], g["min_inliers"][i], g["max_its"][i]) == (pr["N"], pr["min_inliers"], pr["max_its"]), key
                assert (bool(g["ok"][i]), int(g["iterations"][i]), int(g["n_inliers"][i]), bool(g["no_more"][i])) == \
                    (r["ok"], r["iterations"], r["n_inliers"], r["no_more"]), key
                assert np.array_equal(g["inliers"][i, :n], r["inliers"]), key
                d = np.abs(g["T"][i] - r["T"]).max()
                worst = max(worst, d)
                assert d <= POSE_TOL, (key, d)
            assert res[-1]["ok"], (name, scenario, i)
        print(f"pnp {name} {scenario}: largest device-oracle pose difference {worst:.3e}")
    finally:
        _restore(rig)


@pytest.mark.parametrize("name", CM.NAMES)
def test_epnp_alone(oracle, rigs, name):
    """compute_pose through sd_debug_epnp on 4, 5 and 60 exact points projected with the camera's K."""
    from sdslam_amd.capi import debug_epnp      # (the rigs fixture has checked that there is a device; no rig is needed)
    cam, worst = CM.CAMERAS[name], 0.0
    for Xw, uv, T in CM.epnp_trials(cam):
        R, t, e = oracle.epnp(Xw, uv, cam.K)
        Rg, tg, eg = debug_epnp(Xw, uv, cam.K)
        d = max(np.abs(R - Rg).max(), np.abs(t - tg).max())
        worst = max(worst, d)
        assert d <= POSE_TOL, (name, len(Xw), d)
        if len(Xw) > 4:
            assert max(np.abs(R - T[:3, :3]).max(), np.abs(t - T[:3, 3]).max()) <= CM.POSE_BOUND, (name, len(Xw))
    print(f"epnp {name}: largest device-oracle difference {worst:.3e}")


@pytest.mark.parametrize("name", CM.NAMES)
def test_motion_model_then_local_map(oracle, rigs, name):
    """TrackWithMotionModel and TrackLocalMap chained on the device: status, counts, the retried flag, match vectors and outlier
    flags identical, poses within 1e-5."""
    rig = rigs(name)
    trk, B, fr, cam = rig["trk"], rig["B"], rig["fr"], rig["cam"]
    lasts = [dict(f["last"]) for f in fr]
    for i, l in enumerate(lasts):       # a third of the last frame's points are not in the map yet
        l["obs"] = (np.arange(len(l["obs"])) % 3 != i % 3).astype(np.int32)
    locals_ = [f["local"] for f in fr]
    T_ref, T0 = _refs(rig), _starts(rig)
    worst = 0.0
    try:
        trk.set_last(0, lasts)
        trk.set_poses(0, T_ref, T0)
        trk.align(B, 0)             # the device's aligned poses: the matcher is compared on these
        T_al = trk.get_align(0, B)["T"]
        trk.set_poses(0, T_ref, T0)
        trk.track_with_motion_model(B, th=8.0, mono=True, align_mode=0)
        tw, gp, (fm, nm), ga = trk.get_tracked(0, B), trk.get_pose_opt(0, B), trk.get_matches(0, B), trk.get_align(0, B)
        T_mm = gp["T"]
        for i in range(B):
            n, key = len(fr[i]["ck"]), (name, "motion model", i)
            r = oracle.track_with_motion_model(fr[i]["pc"], fr[i]["pr"], fr[i]["tab"], fr[i]["ck"], fr[i]["cd"], cam.bounds, cam.K, T_ref[i], T0[i],
                                               lasts[i], 8.0, mono=True, align_mode=0, T_aligned=T_al[i])
            assert (tw["status"][i], tw["retried"][i], tw["nmatches"][i], tw["nmatches_map"][i]) == \
                (r["status"], r["retried"], r["nmatches"], r["nmatches_map"]), key
            assert np.array_equal(fm[i, :n], r["match"]) and (fm[i, n:] == -1).all(), key
            d = np.abs(gp["T"][i] - r["T"]).max()
            worst = max(worst, d)
            assert d <= POSE_TOL, (key, d)
            assert np.abs(ga["T"][i] - r["T"]).max() <= POSE_TOL and not gp["outlier"][i].any(), key
            assert r["status"] == 2
            CM.pose_close(gp["T"][i], rig["scenes"][i]["T_cur"], key)
        trk.track_local_map(B, th=1.0, min_inliers=30)
        g, gp, gl = trk.get_local_map(0, B), trk.get_pose_opt(0, B), trk.get_local(0, B)
        for i in range(B):
            n, key = len(fr[i]["ck"]), (name, "local map", i)
            r = oracle.track_local_map(fr[i]["ck"], fr[i]["cd"], fr[i]["tab"], LOG_SF, cam.bounds, cam.K, T_mm[i], fm[i, :n], lasts[i], locals_[i],
                                       th=1.0, min_inliers=30)
            assert np.array_equal(gl["match"][i, :n], r["local_match"]), key
            want = np.where(r["local_match"] >= 0, r["local_match"] + MP, r["frame_match"])
            assert np.array_equal(g["match"][i, :n], want) and (g["match"][i, n:] == -1).all(), key
            assert g["n_points"][i] == r["n_points"] and g["n_local"][i] == r["n_local"], key
            assert np.array_equal(gp["outlier"][i, :n], r["outlier"]), key
            assert g["n_inliers"][i] == r["n_inliers"] and g["status"][i] == r["status"], (key, g["n_inliers"][i], r["n_inliers"])
            d = np.abs(gp["T"][i] - r["T"]).max()
            worst = max(worst, d)
            assert d <= POSE_TOL, (key, d)
            assert r["n_local"] > 100 and r["status"] == 2
        print(f"track {name}: largest device-oracle pose difference {worst:.3e}")
    finally:
        _restore(rig)


# ---- the kernels whose reference is a Python restatement: no images, a camera through the debug entry or the case builder ----
FUSE_CAMERAS = ["aniso", "window", "tum1", "wide"]      # tum1: its K with its bounds (the debug entry takes keypoints as given)


@pytest.mark.parametrize("sim3", [0, 1])
@pytest.mark.parametrize("name", FUSE_CAMERAS)
def test_fuse_under_cameras(rigs, name, sim3):
    """k_fuse through sd_debug_fuse, both overloads: KeyFrame::IsInImage (>= min && < max) a hair inside and outside each of the
    camera's four bounds, and a random keyframe of 300 keypoints against 70 points (more than one pass of 64): bit for bit."""
    import fuse_cases as FC
    import fuse_ref as FR
    from sdslam_amd import capi
    cam = CM.cam9(CM.CAMERAS[name])
    edges, shape = FC.unit_image_edges(cam), FC.shape_case("shape_" + name, 50, 300, 70, cam=cam)
    found = 0
    for c in (edges, shape):
        (want_idx, want_dist), T = FC.reference(c, sim3)
        g = capi.debug_fuse(c["kps"], c["desc"], c["uright"], c["pts"], T, c["cam"], FC.SF, FC.INV_SIGMA2, FC.SCALE, c["th"], bool(sim3))
        assert np.array_equal(g["best_idx"], want_idx) and np.array_equal(g["best_dist"], want_dist), (name, sim3, c["name"], g["best_idx"], want_idx)
        assert g["n_found"] == int((want_idx >= 0).sum())
        if not sim3:
            R, t, Ow = FR.decompose(T, False)
            assert np.array_equal(g["pose"][0], R) and np.array_equal(g["pose"][1], t) and np.array_equal(g["pose"][2], Ow)
        found += g["n_found"]
    expect = edges["expect_sim3" if sim3 else "expect"]
    got = capi.debug_fuse(edges["kps"], edges["desc"], edges["uright"], edges["pts"], FC.reference(edges, sim3)[1], cam, FC.SF, FC.INV_SIGMA2,
                          FC.SCALE, edges["th"], bool(sim3))["best_idx"]
    assert got.tolist() == [expect[i] for i in range(len(got))], (name, sim3, got)
    assert found >= 4 + 10, (name, sim3, found)


@pytest.mark.parametrize("name", ["aniso", "offaxis"])
def test_triangulation_search_and_f12_under_cameras(rigs, name):
    """SearchForTriangulation on shape cases built with the camera's K, sideways and forward motion (matches identical), and
    k_tri_geometry's F12 and epipole read back from the device for those two pose pairs against triangulation_ref, to
    test_device_compute_f12's bound: 64 x the restatement's own float64 / longdouble gap."""
    import triangulation_cases as TC
    import triangulation_ref as TR
    from sdslam_amd import capi
    sd, K = rigs("synth")["sd"], CM.CAMERAS[name].K
    total = 0
    for tag, motion, n1, n2 in (("sideways", TC.SIDEWAYS, 130, 100), ("forward", TC.FORWARD, 90, 200)):
        c = TC.shape_case("%s_%s" % (name, tag), 60, n1, n2, motion=motion, flagged=0.2, stereo=0.3, K=K)
        assert np.array_equal(c["F12"], TR.compute_f12(*motion, K)) and not np.array_equal(c["F12"], TR.compute_f12(*motion, TC.K))
        for ori in (0, 1):
            want_n, want_m = TC.reference(c, ori)
            n, m = capi.debug_search_for_triangulation(c["k1"], c["d1"], c["h1"], c["u1"], c["k2"], c["d2"], c["h2"], c["u2"], c["F12"], c["epi"],
                                                       c["sf"], c["sigma2"], ori)
            assert n == want_n and np.array_equal(m, want_m), (name, tag, ori, n, want_n)
            total += n
    assert total > 40, (name, total)
    pairs = [TC.SIDEWAYS, TC.FORWARD]
    tiny = (50, 1.2, 1, 20, 64, 64)
    ext = [sd.ORBextractor(*tiny, len(pairs)) for _ in range(2)]
    trk = sd.Tracker(ext[0], ext[1], max_points=8, max_batch=len(pairs), pnp_max_iterations=4)
    try:
        trk.set_camera(*K, 0.0, CM.CAMERAS[name].bounds)
        img = synth.make_batch(5, 2, 64, 64)
        ext[0].extract_batch(img)
        ext[1].extract_batch(img)
        trk.set_poses(0, [p[1] for p in pairs], [p[0] for p in pairs])
        trk.search_for_triangulation(len(pairs), False, False)
        g = trk.get_triangulation_matches(0, len(pairs))
        gap = max(float(np.abs(TR.compute_f12(T1, T2, K).astype(np.longdouble) - TR.compute_f12_longdouble(T1, T2, K)).max())
                  / float(np.abs(TR.compute_f12_longdouble(T1, T2, K)).max()) for T1, T2 in pairs)
        bound, worst = 64.0 * gap, 0.0
        assert 0 < bound < 1e-10
        for i, (T1, T2) in enumerate(pairs):
            F64 = TR.compute_f12(T1, T2, K)
            d = float(np.abs(g["F12"][i] - F64).max() / np.abs(F64).max())
            worst = max(worst, d)
            assert d <= bound, (name, i, d, bound)
            assert g["epipole"][i].tobytes() == TR.epipole(T1, T2, K).tobytes(), (name, i)
        print(f"k_tri_geometry {name}: largest relative F12 deviation {worst:.3e}, bound {bound:.3e}")
    finally:
        trk.close()
        for e in ext:
            e.close()


def test_triangulate_under_anisotropic_camera(rigs):
    """k_triangulate through sd_debug_triangulate with aniso's K and bf = 40: the threshold pairs (re-bisected under this camera),
    the stereo branches and one count case; verdicts and branches identical, Xw bit for bit."""
    import new_points_cases as NC
    import new_points_ref as NR
    from sdslam_amd import capi
    cam5 = CM.cam5(CM.CAMERAS["aniso"])
    cases = [NC.thresholds_case(cam5), NC.stereo_case(cam5), NC.count_case(65, 75, cam5)]
    seen = set()
    for c in cases:
        assert np.array_equal(c["cam5"], cam5)
        margins = []
        v, b, X = NC.reference(c, margins)
        assert all(m > NC.MARGIN for m in margins), (c["name"], min(margins))      # the device's atan2f is not the host's
        gv, gb, gX = capi.debug_triangulate(c["k1u"], c["k1"], c["ur1"], c["z1"], c["k2u"], c["k2"], c["ur2"], c["z2"], c["m"], c["T1"], c["T2"],
                                            c["cam5"], c["sf"], c["sigma2"], c["scale_factor"], c["monocular"], c["median"])
        assert np.array_equal(gv, v), (c["name"], np.flatnonzero(gv != v)[:8], gv[gv != v][:8], v[gv != v][:8])
        assert np.array_equal(gb, b), (c["name"], np.flatnonzero(gb != b)[:8])
        bad = np.flatnonzero((gX.view(np.uint64) != X.view(np.uint64)).any(axis=1))
        assert bad.size == 0, (c["name"], bad[:8], gX[bad[:2]], X[bad[:2]])
        for i, (cv, cb) in c["claims"].items():
            assert (cv is None or v[i] == cv) and (cb is None or b[i] == cb), (c["name"], i, v[i], b[i], cv, cb)
        seen.update(zip(v.tolist(), b.tolist()))
    assert {NR.BR_SVD, NR.BR_UNPROJECT1, NR.BR_UNPROJECT2} <= {b for _, b in seen} and len({v for v, _ in seen}) >= 6, seen
    assert cases[0]["steps"] == NC.thresholds_case()["steps"]          # every gate still has its pair one float step apart


def test_unproject_stereo_under_anisotropic_camera(rigs):
    """k_new_points' Frame::UnprojectStereo through stereo_init on a distorted rig whose K is aniso's: ids in keypoint order, Xw
    bit-equal to the definition (keyframe_points_ref.unproject_stereo) on the undistorted keypoints."""
    import keyframe_points_ref as R
    import test_keyframe_points_gpu as KP
    sd, K = rigs("synth")["sd"], CM.CAMERAS["aniso"].K
    rig = KP.Rig(sd, KP.CFGS["p8"], [121, 122], 1, distorted=True, static=False, K=K)
    trk, B = rig.trk, rig.B
    try:
        trk.cur.extract_batch(rig.views[0])
        rig.stereo(0)
        trk.set_next_map_id(0, np.array([0, 5000], np.int32))
        trk.stereo_init(B, 500)
        got = trk.get_created(0, B)
        _, dd = trk.get_stereo(0, B)
        kk, ku, cd, cn = rig.keys_un()
        for b in range(B):
            n = cn[b]
            assert np.abs(ku[b]["x"][:n] - kk[b]["x"][:n]).max() > 0.5
            want = R.stereo_initialization(dd[b, :n], 500)
            c = len(want)
            assert c > 300 and (got["mode"][b], got["created"][b]) == (2, c), b
            assert got["kp_index"][b, :c].tolist() == want
            differs = 0
            for r, i in enumerate(want):
                X = R.unproject_stereo(ku[b]["x"][i], ku[b]["y"][i], dd[b, i], K, np.eye(4))
                assert np.array_equal(got["Xw"][b, r], X), (b, i, got["Xw"][b, r], X)
                differs += not np.array_equal(X, R.unproject_stereo(ku[b]["x"][i], ku[b]["y"][i], dd[b, i], (K[1], K[0], K[3], K[2]), np.eye(4)))
            assert differs > 0.9 * c          # fx <-> fy, cx <-> cy would show
    finally:
        rig.close()
