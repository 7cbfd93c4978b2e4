"""GPU parity of the image-reading tracking kernels at frame sizes other than VGA (tests/geometries.py).  Almost every tracking
parity test runs at 640 x 480: landscape, multiples of 16, cols > rows on every level, even pitches, and no point within 3 px of
the right or bottom border of an aligned level, so k_align's cols / rows / pitch, k_stereo_from_depth's w / h / stride and a
frame-grid cell that is taller than wide have never been told apart on the device.  Here each stage runs at each geometry on
the images of that size and is compared with the oracle (or, for the depth sampling and the grid occupancy, a numpy statement
of the kernel's lines) called on the same inputs.  tests/test_geometries_cpu.py shows that the cases are sound and that a
device with the wrong size, pitch or bounds would differ here."""
import numpy as np
import pytest

import cameras as CM
import geometries as G
import stage_parity as SP
import sweep_rig as SR
from sdslam_amd import synth

pytestmark = pytest.mark.gpu
POSE_TOL = SP.POSE_TOL
MP = G.MP


@pytest.fixture(scope="module")
def rigs(oracle):
    """name -> rig, built on first use: the oracle's rig of the geometry, two extractors of its frame size holding the two
    scenes, and a tracker.  The oracle's keypoints, descriptors and padded levels 2-4 equal the device's, asserted once."""
    SR.device()
    built = {}

    def get(name):
        if name in built:
            return built[name][0]
        r, close = built[name] = SR.device_rig(G.oracle_rig(oracle, name), pnp_max_iterations=100)
        (cur, ref), fr = r["ext"], r["fr"]
        for i in range(r["B"]):
            for k, l in enumerate(G.ALIGNED_LEVELS):
                assert cur.level_size(l) == fr[i]["shapes"][l][::-1], (name, l)
                assert np.array_equal(cur.level(l, i, padded=True), fr[i]["pc_pad"][k]), (name, i, l, "cur")
                assert np.array_equal(ref.level(l, i, padded=True), fr[i]["pr_pad"][k]), (name, i, l, "ref")
        r["bufs"] = {}
        return r

    yield get
    for r, close in built.values():
        for b in r["bufs"].values():
            b.free()
        close()


def _depth_buffer(rig, tag):
    """The strided, poisoned depth maps of the rig in device memory (uploaded once)."""
    if tag not in rig["bufs"]:
        flat = rig["buf_" + tag][0]
        buf = rig["sd"].DeviceBuffer(flat.nbytes)
        buf.upload(flat)
        rig["bufs"][tag] = buf
    return rig["bufs"][tag]


def _stereo_device(rig, which):
    tag, dtype, factor, _ = which
    geo = rig["geo"]
    _, stride, fstride = rig["buf_" + tag]
    rig["trk"].stereo_from_depth_device(_depth_buffer(rig, tag).ptr, dtype, geo.w, geo.h, stride, fstride, depth_map_factor=factor)
    return rig["trk"].get_stereo(0, rig["B"])


@pytest.mark.parametrize("name", G.NAMES)
def test_image_align(oracle, rigs, name):
    """ImageAlign from the perturbed start in modes 0 (frame) and 1 (keyframe), the twelve planted border points among their 300,
    and in mode 3 (keyframe against keyframe: level 4 alone, the first 100 valid points, scale (float)(1 / sf[4])) on the last
    frame built for it, whose 100 points end with the four level-4 points planted for that scale: ok and per-level iterations
    equal, error to a relative 1e-7, pose within 1e-5; in mode 3 the pose is untouched."""
    res = SP.image_align(oracle, rigs(name), name, modes=[(0, "last"), (1, "last"), (3, "last3")])
    print(f"align {name}: largest device-oracle pose difference {res['worst']:.3e}, relative error difference {res['worst_error']:.3e}")


RUNS = [(mono, th, None) for mono in (True, False) for th in (8.0, 1.0)]        # (mono, th, no match_split option)


@pytest.mark.parametrize("name", G.NAMES)
def test_search_by_projection(oracle, rigs, name):
    """SearchByProjection(Frame, Frame), mono and with planted uRight and bf = 40, th = 8 and th = 1: the match vector and the
    count equal the oracle's."""
    res = SP.search_by_projection(oracle, rigs(name), name, RUNS, {8.0: 60, 1.0: 10})
    print(f"search_by_projection {name}: {res['total']} matches identical, largest device-oracle difference 0")


@pytest.mark.parametrize("name", G.NAMES)
def test_local_map_search(oracle, rigs, name):
    """isInFrustum, PredictScale (the 1.5 pyramid's levels in small15) and the search: every output equals the oracle's."""
    SP.local_map_search(oracle, rigs(name), name, 60, some_out_of_view=False)
    print(f"match_local {name}: every output identical, largest device-oracle difference 0")


@pytest.mark.parametrize("name", G.NAMES)
def test_features_in_area_and_grid(oracle, rigs, name):
    """Frame::GetFeaturesInArea on the device grid for geometries.area_queries (the four bounds corners, straddling the right and
    bottom bounds, around (W - 1, H - 1), discs wider than a cell in one direction only): index lists identical and in order; the
    grid occupancy [64][48] equals Frame::AssignFeaturesToGrid's."""
    rig = rigs(name)
    trk, fr, cam, geo = rig["trk"], rig["fr"], rig["cam"], rig["geo"]
    for i in range(rig["B"]):
        _, grid = trk.features_in_area(i, 0.5 * geo.w, 0.5 * geo.h, 10.0, want_grid=True)
        want_grid = G.grid_occupancy(fr[i]["ck"], cam.bounds)
        assert np.array_equal(grid, want_grid), (name, i, np.argwhere(grid != want_grid)[:8])
        assert grid.sum() == len(fr[i]["ck"])
    total = SP.features_in_area(oracle, rig, name, G.area_queries(geo))
    print(f"features_in_area {name}: {total} indices and the grid occupancy identical, largest device-oracle difference 0")


@pytest.mark.parametrize("name", G.NAMES)
def test_stereo_from_depth_device(rigs, name):
    """sd_track_stereo_from_depth_device on the strided, poisoned maps, float32 and 16-bit, with and without conversion: uright and
    depth equal the numpy statement of k_stereo_from_depth bit for bit, and no output carries the poison value."""
    rig = rigs(name)
    fr, geo, B, cap = rig["fr"], rig["geo"], rig["B"], rig["cap"]
    try:
        rig["trk"].set_camera(*rig["cam"].K, G.BF, rig["cam"].bounds)
        for which in G.DEPTH_CALLS:
            tag, _, factor, convert = which
            flat, stride, fstride = rig["buf_" + tag]
            ur, dd = _stereo_device(rig, which)
            scale = G.depth_scale(factor)
            poison = np.float32(G.POISON_F32 if tag == "f32" else G.POISON_U16) * (scale if convert else np.float32(1))
            for i in range(B):
                n = len(fr[i]["ck"])
                wu, wd = G.stereo_from_depth(fr[i]["ck"], fr[i]["ck"], flat, i, geo.w, geo.h, stride, fstride, convert, scale, G.BF)
                assert ur[i, :n].tobytes() == wu.tobytes() and dd[i, :n].tobytes() == wd.tobytes(), (name, which, i, np.flatnonzero(dd[i, :n] != wd)[:8])
                assert (ur[i, n:] == -1).all() and (dd[i, n:] == -1).all(), (name, which, i)
                assert not (dd[i] == poison).any() and (wd > 0).sum() >= 100 and (wd < 0).sum() >= 10, (name, which, i)
        print(f"stereo_from_depth_device {name}: 4 calls x {B} frames bit-exact, largest device-restatement difference 0")
    finally:
        SR.restore(rig)


@pytest.mark.parametrize("name", G.NAMES)
def test_motion_model_then_local_map(oracle, rigs, name):
    """TrackWithMotionModel and TrackLocalMap chained on the device, monocular: status, counts, the retried flag, match vectors and
    outlier flags identical, poses within 1e-5."""
    res = SP.motion_model_then_local_map(oracle, rigs(name), name, ("n_inliers", 30))
    print(f"track {name}: largest device-oracle pose difference {res['worst']:.3e}")


@pytest.mark.parametrize("name", G.NAMES)
def test_motion_model_then_local_map_rgbd(oracle, rigs, name):
    """The same chain on RGB-D frames whose mvuRight / mvDepth are sampled on the device from the 16-bit strided maps (bf = 40),
    TrackLocalMap at th 3, then close_points on the result against the host restatement of its counts."""
    rig = rigs(name)
    res = SP.motion_model_then_local_map(oracle, rig, name, ("n_inliers", 30), mono=False, th_lm=3.0,
                                         sample_depth=lambda: _stereo_device(rig, G.DEPTH_CALLS[2]))
    print(f"track rgbd {name}: largest device-oracle pose difference {res['worst']:.3e}")


# ---- wide and portrait only: the keyframe map and the sequential loop ------------------------------------------------------------
KF_MOTIONS = [("other", (0.0, 0.0, 0.0), (0.0, 0.0, 0.0)),                     # another place
              ("same", (0.02, -0.005, 0.012), (0.35, -0.1, 0.3)),              # close
              ("same", (0.012, -0.012, 0.008), (0.3, -0.25, 0.45))]            # closest
KF_T_CUR = ((0.015, -0.01, 0.01), (0.3, -0.2, 0.4))


@pytest.fixture(scope="module")
def kfmaps(oracle):
    """name -> one current frame and three keyframes of a small map at that frame size (tests/test_track_gpu.py's kfmap): the
    first keyframe shows another place, the other two see the current frame's scene from nearby."""
    import sdslam_amd as sd
    built = {}

    def get(name):
        if name in built:
            return built[name]
        geo = G.GEOMETRIES[name]
        cam, cfg, NK = geo.cam, geo.cfg, len(KF_MOTIONS)
        tex = {"same": synth.make_image(71, 2 * geo.w, 2 * geo.h), "other": synth.make_image(72, 2 * geo.w, 2 * geo.h)}
        T_cur = synth.se3_exp(*KF_T_CUR)
        T_kf = [synth.se3_exp(u, w) for _, u, w in KF_MOTIONS]
        cur, ref = sd.ORBextractor(*cfg, geo.w, geo.h, 1), sd.ORBextractor(*cfg, geo.w, geo.h, NK)
        im_cur = CM.render(tex["same"], T_cur, cam, geo.w, geo.h)
        im_kf = np.stack([CM.render(tex[t], T, cam, geo.w, geo.h) for (t, _, _), T in zip(KF_MOTIONS, T_kf)])
        ck, cd, cn = cur.extract_batch(im_cur[None])
        rk, rd, rn = ref.extract_batch(im_kf)
        oc = oracle.OrbOracle(*cfg)
        ock, ocd = oc.extract(im_cur)
        assert np.array_equal(ock, ck[0, :cn[0]]) and np.array_equal(ocd, cd[0, :cn[0]]), name
        kfs = []
        for i in range(NK):
            orf = oracle.OrbOracle(*cfg)
            ork, ord_ = orf.extract(im_kf[i])
            assert np.array_equal(ork, rk[i, :rn[i]]) and np.array_equal(ord_, rd[i, :rn[i]]), (name, i)
            kfs.append(dict(orf=orf, last=CM.keyframe_case(ork, ord_, T_kf[i], cam, max_points=MP)))
        trk = sd.Tracker(cur, ref, max_points=MP, max_batch=NK, pnp_max_iterations=100)      # cur holds ONE frame
        trk.set_camera(*cam.K, 0.0, cam.bounds)
        trk.set_last(0, [k["last"] for k in kfs])
        built[name] = dict(geo=geo, cam=cam, NK=NK, T_cur=T_cur, T_kf=T_kf, trk=trk, ext=(cur, ref), oc=oc, ck=ock, cd=ocd, kfs=kfs, tab=oc.tables(),
                           NL=cfg[2])
        return built[name]

    yield get
    for m in built.values():
        m["trk"].close()
        for e in m["ext"]:
            e.close()


@pytest.mark.parametrize("name", G.LOOPED)
def test_relocalization_over_keyframes(oracle, kfmaps, name):
    """Tracking::Relocalization with every keyframe attempt as one batch slot against the broadcast current frame: per slot the
    three stages equal the oracle's ImageAlign(frame, kf, fast) -> SearchByProjection -> PoseOptimization, and the winner is where
    the reference's loop stops (the first keyframe of the right place)."""
    m = kfmaps(name)
    trk, NK, K, bounds = m["trk"], m["NK"], m["cam"].K, m["cam"].bounds
    trk.set_poses(0, m["T_kf"], m["T_kf"])                  # mCurrentFrame.SetPose(kf->GetPose())
    th = 15.0
    winner, st = trk.relocalize(NK, cur_frame=0, th=th, mono=True)
    ga, (cm, nm), gp = trk.get_align(0, NK), trk.get_matches(0, NK), trk.get_pose_opt(0, NK)
    pc = [m["oc"].level(l) for l in range(m["NL"])]
    n, expect, worst = len(m["ck"]), -1, 0.0
    for i in range(NK):
        k = m["kfs"][i]
        pr = [k["orf"].level(l) for l in range(m["NL"])]
        ra = oracle.align(pc, pr, m["tab"]["inv_sf"], m["tab"]["sf"], G.align_points(k["last"]), m["T_kf"][i], m["T_kf"][i], K, mode=2)
        assert ga["ok"][i] == ra["ok"] == st[i, 0], (name, i)
        T_al = ra["T"] if ra["ok"] else m["T_kf"][i]
        worst = max(worst, np.abs(ga["T"][i] - T_al).max())
        assert np.abs(ga["T"][i] - T_al).max() <= POSE_TOL, (name, i)
        # the later stages are checked from the DEVICE's aligned pose, as tests/test_track_gpu.py does
        nmo, ocm = oracle.search_by_projection(m["ck"], m["cd"], m["tab"]["sf"], bounds, K, ga["T"][i], m["T_kf"][i], k["last"], th=th, mono=True,
                                               check_ori=True)
        assert nm[i] == nmo == st[i, 1] and np.array_equal(cm[i, :n], ocm), (name, i)
        rp = oracle.pose_optimization(m["ck"], ocm >= 0, k["last"]["Xw"][np.maximum(ocm, 0)], m["tab"]["inv_sigma2"], K, ga["T"][i])
        assert gp["n_inliers"][i] == rp["n_inliers"] == st[i, 2], (name, i)
        assert np.array_equal(gp["outlier"][i, :n], rp["outlier"]), (name, i)
        worst = max(worst, np.abs(gp["T"][i] - rp["T"]).max())
        assert np.abs(gp["T"][i] - rp["T"]).max() <= POSE_TOL, (name, i)
        if expect < 0 and ra["ok"] and nmo >= 20 and rp["n_inliers"] >= 10:
            expect = i
    assert winner == expect == 1, (name, winner, expect, st)
    assert np.abs(gp["T"][winner][:3, 3] - m["T_cur"][:3, 3]).max() < 1e-2, name      # it found the place (the oracle alone: 3.3e-3 / 4.8e-3)
    print(f"relocalize {name}: winner {winner}, largest device-oracle pose difference {worst:.3e}")


@pytest.mark.parametrize("name", G.LOOPED)
def test_detect_loop_candidates(oracle, kfmaps, name):
    """LoopClosing::DetectLoop's candidate search: KF-KF ImageAlign (mode 3, level 4 alone) of the current keyframe against the
    three keyframes in one launch, then the reference's loop (exclusions, skip-after-failure, 1.5 x best)."""
    m = kfmaps(name)
    trk, NK, K = m["trk"], m["NK"], m["cam"].K
    trk.set_poses(0, m["T_kf"], [np.eye(4)] * NK)
    # KF-KF alignment at level 4 stays under its error gate on these scenes; the failure the loop meets in practice is a keyframe
    # without map points.  Slot 0 is one, so the reference's skip-after-failure hides slot 1 unless slot 0 is excluded.
    lasts = [dict(k["last"]) for k in m["kfs"]]
    lasts[0]["valid"] = np.zeros_like(lasts[0]["valid"])
    trk.set_last(0, lasts)
    pc = [m["oc"].level(l) for l in range(m["NL"])]
    ok, err = [], []
    for i in range(NK):
        pr = [m["kfs"][i]["orf"].level(l) for l in range(m["NL"])]
        r = oracle.align(pc, pr, m["tab"]["inv_sf"], m["tab"]["sf"], G.align_points(lasts[i]), m["T_kf"][i], np.eye(4), K, mode=3)
        ok.append(r["ok"])
        err.append(r["error"])

    def reference_loop(excluded):
        cand, best, i = {}, 1e10, 0
        while i < NK:                           # for (i = 0; i < kfs.size(); i++)
            if not excluded[i]:
                if not ok[i]:
                    i += 1                      # "Skip some keyframes"
                else:
                    cand[i] = err[i]
                    best = min(best, err[i])
            i += 1
        return sorted(j for j, e in cand.items() if e < best * 1.5), best

    worst = 0.0
    try:
        for excluded in ([0, 0, 0], [0, 1, 0], [1, 0, 0], [0, 0, 1], [1, 1, 1]):
            g = trk.detect_loop(NK, cur_frame=0, excluded=excluded)
            want, best = reference_loop(excluded)
            assert list(g["candidates"]) == want, (name, excluded, g, want)
            assert abs(g["best_error"] - best) <= 1e-7 * max(1.0, abs(best)), (name, excluded)
            for i in range(NK):
                e = abs(g["errors"][i] - err[i]) / max(1.0, abs(err[i]))
                worst = max(worst, e)
                assert e <= 1e-7, (name, excluded, i, e)
        assert ok == [False, True, True], (name, ok)
        assert reference_loop([0, 0, 0])[0] != reference_loop([1, 0, 0])[0]          # the skip hid a keyframe
    finally:
        trk.set_last(0, [k["last"] for k in m["kfs"]])
    print(f"detect_loop {name}: candidates identical, largest relative error difference {worst:.3e}")


@pytest.mark.parametrize("name", G.LOOPED)
def test_closed_sequential_loop(oracle, name):
    """2 streams x 4 frames at the geometry's frame size, monocular, on the device's own prior (tests/test_motion_gpu.py's MLoop;
    synth's camera behind bounds (0, W, 0, H)): extraction, motion_predict, TrackWithMotionModel, TrackLocalMap, motion_update and
    the device hand-off per frame.  The prior, X and P equal the reference filter fed the device's own poses (to
    test_motion_gpu's TOL); the oracle's loop driven with the device's priors gives equal statuses, counts and match vectors and
    poses within 1e-5; the hand-off equals the host restatement bit for bit; every stream is tracked at every frame."""
    import sdslam_amd as sd
    import test_motion_gpu as MG
    import test_sequence_gpu as SQ
    geo = G.GEOMETRIES[name]
    L = MG.MLoop(sd, oracle, geo.cfg, [11, 12], 4, w=geo.w, h=geo.h)
    trk, B = L.trk, L.B
    worst, worst_f = 0.0, 0.0
    try:
        refs = [MG.R.EKF() for _ in range(B)]
        Tref = [s["T"][0] for s in L.seqs]
        for t in range(1, L.T):
            prior, mo_p = L.motion_step(t, 15.0, 1.0, sync=True)
            tw, (fm, _), gl, gp, al = trk.get_tracked(0, B), trk.get_matches(0, B), trk.get_local_map(0, B), trk.get_pose_opt(0, B), trk.get_align(0, B)
            old, mo = trk.get_last(0, B), trk.get_motion(0, B)
            ck, _, cn = trk.cur.download(0, B)
            trk.advance(B, 1)
            new = trk.get_last(0, B)
            for b in range(B):
                n, key = cn[b], (name, t, b)
                # the filter on the device's own poses
                want = refs[b].predict(Tref[b], MG.DT)
                d = max(np.abs(prior[b] - want).max(), np.abs(mo_p["E"][b] - refs[b].E).max())
                assert prior[b].tobytes() == SQ.prior_product(mo_p["E"][b], Tref[b]).tobytes(), key
                refs[b].track(al["T"][b], tracked=gl["status"][b] == 2)
                d = max(d, np.abs(mo["X"][b] - refs[b].X).max(), np.abs(mo["P"][b] - np.diag(refs[b].P)).max())
                worst_f = max(worst_f, d)
                assert d <= MG.TOL and mo["started"][b] == int(refs[b].started()), (key, d)
                # the hand-off on the device's own outputs
                prev = {k: old[k][b] for k in ("valid", "Xw", "desc", "octave", "angle", "obs")}
                want = SQ.host_handoff(ck[b], n, gl["match"][b], gp["outlier"][b], prev, old["ids"][b], L.local[b], L.lids[b])
                SQ.check_last(new, b, want, n, key)
                # the oracle's loop on the device's prior
                r, rl, un, N = L.oracle_step_prior(oracle, t, b, prior[b], 15.0, 1.0)
                assert N == n, key
                assert (tw["status"][b], tw["nmatches"][b], tw["nmatches_map"][b]) == (r["status"], r["nmatches"], r["nmatches_map"]), key
                assert np.array_equal(fm[b, :n], r["match"]) and np.array_equal(gl["match"][b, :n], un), key
                assert (gl["status"][b], gl["n_inliers"][b], gl["n_local"][b]) == (rl["status"], rl["n_inliers"], rl["n_local"]), key
                assert np.array_equal(gp["outlier"][b, :n], rl["outlier"]), key
                d = np.abs(gp["T"][b] - rl["T"]).max()
                worst = max(worst, d)
                assert d <= POSE_TOL, (key, d)
                assert np.abs(al["T"][b] - gp["T"][b]).max() == 0, key
                assert tw["status"][b] == 2 and gl["status"][b] == 2, key
                assert np.abs(gp["T"][b][:3, 3] - L.seqs[b]["T"][t][:3, 3]).max() < 0.02, key
                Tref[b] = al["T"][b]
        assert all(np.abs(f.X).max() > 1e-3 for f in refs)          # the filter picked up a velocity
        print(f"sequential loop {name}: largest device-oracle pose difference {worst:.3e}, largest deviation of prior / E / X / P from the "
              f"reference filter {worst_f:.3e}")
    finally:
        L.close()
