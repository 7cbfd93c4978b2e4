"""GPU parity of the tracking kernels under cameras other than synth's (tests/cameras.py).  Every other tracking test sets
fx = fy = 500, the principal point at the image centre and bounds (0, 640, 0, 480), so fx and fy, cx and cy, invW and invH
and `x - min_x` and `x` have never been told apart on the device, no keypoint has ever been outside the frame grid, and no
matcher or pose solver has seen undistorted keypoints.  Here each stage runs under each camera on the images that camera
sees and is compared with the oracle called on the same inputs and the same float-rounded camera.
tests/test_cameras_cpu.py shows that the cases are sound and that a device using a wrong camera would differ here."""
import numpy as np
import pytest

import cameras as CM
import stage_parity as SP
import sweep_rig as SR
from sdslam_amd import synth

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rigs(oracle):
    """name -> rig, built on first use: the oracle's rig of the camera, two extractors (with the camera's distortion) holding
    the two scenes, and a tracker.  The oracle's extraction and undistorted keypoints equal the device's, asserted once."""
    SR.device()
    built = {}

    def get(name):
        if name not in built:
            built[name] = SR.device_rig(CM.oracle_rig(oracle, name), pnp_max_iterations=512)
        return built[name][0]

    yield get
    for _, close in built.values():
        close()


@pytest.mark.parametrize("name", CM.NAMES)
def test_image_align(oracle, rigs, name):
    """ImageAlign from the perturbed start in modes 0 (frame), 1 (keyframe) and 3 (keyframe against keyframe): ok and per-level
    iterations equal, error to a relative 1e-7, pose within 1e-5.  Under aniso and window the fx-only scale of the reference's
    Jacobian is followed, not repaired: the oracle has it."""
    res = SP.image_align(oracle, rigs(name), name)
    print(f"align {name}: largest device-oracle pose difference {res['worst']:.3e}, relative error difference {res['worst_error']:.3e}")


RUNS = [(mono, th, None) for mono in (True, False) for th in (8.0, 1.0)]        # (mono, th, no match_split option)


@pytest.mark.parametrize("name", CM.NAMES)
def test_search_by_projection(oracle, rigs, name):
    """SearchByProjection(Frame, Frame), mono and with planted uRight and bf = 40, th = 8 and th = 1: the match vector and the
    count equal the oracle's."""
    SP.search_by_projection(oracle, rigs(name), name, RUNS, {8.0: 150, 1.0: 20})


@pytest.mark.parametrize("name", CM.NAMES)
def test_local_map_search(oracle, rigs, name):
    """isInFrustum (its bounds test included: under window, points inside the image are rejected), PredictScale and the
    search: every output equals the oracle's."""
    SP.local_map_search(oracle, rigs(name), name, 150)


@pytest.mark.parametrize("name", CM.NAMES)
def test_features_in_area(oracle, rigs, name):
    """Frame::GetFeaturesInArea on the device grid for cameras.area_queries: the index lists are identical and in order."""
    SP.features_in_area(oracle, rigs(name), name, CM.area_queries(CM.CAMERAS[name]))


@pytest.mark.parametrize("name", CM.NAMES)
def test_pose_optimization(oracle, rigs, name):
    """The planted 30 %-outlier vector, one and four waves per frame, mono and with planted uRight, from the perturbed start:
    identical flags and counts, pose within 1e-5 of the oracle's."""
    res = SP.pose_optimization(oracle, rigs(name), name)
    print(f"pose_opt {name}: largest device-oracle pose difference {res['worst']:.3e}")


@pytest.mark.parametrize("scenario", ["out30_c4", "out65_chunked"])       # one that refines at once; one re-entered in chunks
@pytest.mark.parametrize("name", CM.NAMES)
def test_pnp_ransac(oracle, rigs, name, scenario):
    res = SP.pnp_ransac(oracle, rigs(name), name, scenario, ends_ok=True)
    print(f"pnp {name} {scenario}: largest device-oracle pose difference {res['worst']:.3e}")


@pytest.mark.parametrize("name", CM.NAMES)
def test_epnp_alone(oracle, rigs, name):
    """compute_pose through sd_debug_epnp on 4, 5 and 60 exact points projected with the camera's K."""
    cam, trials = CM.CAMERAS[name], CM.epnp_trials(CM.CAMERAS[name])      # (the rigs fixture has checked that there is a device; no rig is needed)
    worst, want = SP.epnp_alone(oracle, name, cam.K, trials, tol=lambda T: SP.POSE_TOL)
    for (Xw, uv, T), (R, t) in zip(trials, want):
        if len(Xw) > 4:
            assert max(np.abs(R - T[:3, :3]).max(), np.abs(t - T[:3, 3]).max()) <= CM.POSE_BOUND, (name, len(Xw))
    print(f"epnp {name}: largest device-oracle difference {worst:.3e}")


@pytest.mark.parametrize("name", CM.NAMES)
def test_motion_model_then_local_map(oracle, rigs, name):
    """TrackWithMotionModel and TrackLocalMap chained on the device: status, counts, the retried flag, match vectors and outlier
    flags identical, poses within 1e-5."""
    rig = rigs(name)
    res = SP.motion_model_then_local_map(oracle, rig, name, ("n_local", 101))
    for i in range(rig["B"]):
        CM.pose_close(res["T_mm"][i], rig["scenes"][i]["T_cur"], (name, "motion model", i))
    print(f"track {name}: largest device-oracle pose difference {res['worst']:.3e}")


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
