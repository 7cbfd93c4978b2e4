"""GPU: RGB-D map points created on the device (sd_track_stereo_init, sd_track_create_keyframe_points, sd_track_need_keyframe,
sd_track_advance with the created points).

Bars: creation equals the numpy restatement (tests/keyframe_points_ref.py) applied to the device's own downloaded inputs --
created flags, creation order, ids, P and counts equal, Xw bit-equal; the hand-off equals the extended restatement bit for
bit; the decision flags equal NeedNewKeyFrame's restatement on the device's own counts; the errors are pinned."""
import numpy as np
import pytest

import keyframe_points_ref as R
from sdslam_amd import synth

pytestmark = pytest.mark.gpu
K = (synth.FX, synth.FY, synth.CX, synth.CY)
BOUNDS = (0.0, 640.0, 0.0, 480.0)
CFGS = {"p8": (1000, 1.2, 8, 20), "p5": (1000, 2.0, 5, 20)}
W, H = 640, 480
M = 1000
BF = 4.0
F32, U16 = 0, 1
DIST = (0.2624, -0.9531, -0.0054, 0.0026, 1.1633)   # k1 != 0: mvKeys != mvKeysUn
LAST_KEYS = ("valid", "Xw", "desc", "octave", "angle", "obs")


@pytest.fixture(scope="module")
def sd():
    import sdslam_amd
    if sdslam_amd.device_count() < 1:
        pytest.fail("no HIP device: the gpu-marked tests need a real MI355X")
    return sdslam_amd


def _code(sd, fn):
    with pytest.raises(sd.SdError) as e:
        fn()
    return e.value.code


def masked_depth(seqs, u16):
    """[T][B][H][W] depth, quantised (equal depths occur), with invalid regions: every 9th column zero, a NaN band and a
    negative band (f32 only), and slot 2 valid in one corner only (fewer than 101 candidates).  ComputeStereoFromRGBD leaves
    mvDepth = -1 on all of them, so the kernel's own NaN / zero tests are pinned by the restatement's known answers."""
    d = np.stack([s["depth"] for s in seqs], 1)
    d = (np.round(d * 250.0) / 250.0).astype(np.float32)
    d[..., ::9] = 0.0
    if not u16:
        d[:, :, 100:130, :] = np.nan
        d[:, :, 300:320, :] = -1.0
    if d.shape[1] > 2:
        keep = d[:, 2, :150, :200].copy()
        d[:, 2] = 0.0
        d[:, 2, :150, :200] = keep
    return d


class Rig:
    """B RGB-D streams with depth maps in device memory; frame 0 in `ref` with a static map of it as last frame and local map
    (Observations() 0 for every 7th point); the last slot has no usable points, so it is never tracked."""

    def __init__(self, sd, cfg, seeds, T, u16=False, distorted=False, static=True, K=K):
        self.sd, self.B, self.T, self.u16, self.distorted = sd, len(seeds), T, u16, distorted
        self.seqs = [synth.make_sequence(s, T, with_depth=True) for s in seeds]
        self.views = np.stack([s["views"] for s in self.seqs], 1)
        self.depth = masked_depth(self.seqs, u16)
        raw = np.round(np.nan_to_num(self.depth) * 5000.0).astype(np.uint16) if u16 else self.depth
        self.dbuf = sd.DeviceBuffer(raw.nbytes)
        self.dbuf.upload(raw)
        self.ext = [sd.ORBextractor(*cfg, W, H, self.B) for _ in range(2)]
        if distorted:
            for e in self.ext:
                e.set_distortion(*K, *DIST)
        self.trk = sd.Tracker(self.ext[0], self.ext[1], max_points=M, max_batch=self.B, pnp_max_iterations=100)
        self.trk.set_camera(*K, BF, BOUNDS)
        if static:
            rk, rd, rn = self.trk.ref.extract_batch(self.views[0])
            maps = [synth.static_map(rk[b, :rn[b]], rd[b, :rn[b]], self.seqs[b]["T"][0], cfg[1], cfg[2], seed=b) for b in range(self.B)]
            maps[-1][1]["valid"][:] = 0
            maps[-1][0]["cand"][:] = 0
            self.local = [m[0] for m in maps]
            self.lids = [m[2] for m in maps]
            self.trk.set_last(0, [m[1] for m in maps])
            self.trk.set_local(0, self.local)
            self.trk.set_map_ids(0, self.lids, 0)
            self.trk.set_map_ids(0, self.lids, 1)
            T0 = [s["T"][0] for s in self.seqs]
            self.trk.set_poses(0, T0, T0)

    def vel(self, t):
        return [s["T"][t] @ np.linalg.inv(s["T"][t - 1]) for s in self.seqs]

    def stereo(self, t):
        es = 2 if self.u16 else 4
        self.trk.stereo_from_depth_device(self.dbuf.ptr.value + t * self.B * W * H * es, U16 if self.u16 else F32, W, H,
                                          depth_map_factor=5000.0 if self.u16 else 1.0)

    def track(self, t, local_map=True):
        trk = self.trk
        trk.cur.extract_batch(self.views[t])
        self.stereo(t)
        trk.set_prior(0, self.vel(t), relative=True)
        trk.track_with_motion_model(self.B, th=15.0, mono=False, align_mode=0)
        if local_map:
            trk.track_local_map(self.B, th=3.0, min_inliers=30)

    def keys_un(self):
        k, d, n = self.trk.cur.download(0, self.B)
        ku = self.trk.cur.download_undistorted(0, self.B) if self.distorted else k
        return k, ku, d, n

    def close(self):
        self.trk.close()
        for e in self.ext:
            e.close()
        self.dbuf.free()


def local_obs_of(rig, b):
    o = np.zeros(M, np.int32)
    o[:len(rig.local[b]["obs"])] = rig.local[b]["obs"]
    return o


def check_created(got, b, want_idx, P, cand, ku, depth, T, id0, key):
    n = len(want_idx)
    assert (got["mode"][b], got["created"][b], got["P"][b], got["candidates"][b]) == (1, n, P, cand), key
    assert got["kp_index"][b, :n].tolist() == want_idx, key
    assert got["ids"][b, :n].tolist() == list(range(id0, id0 + n)), key
    for r, i in enumerate(want_idx):
        X = R.unproject_stereo(ku[b]["x"][i], ku[b]["y"][i], depth[i], K, T)
        assert np.array_equal(got["Xw"][b, r], X), (key, r, i, got["Xw"][b, r], X)


@pytest.mark.parametrize("name,u16,distorted", [("p8", False, False), ("p8", True, True), ("p5", False, True), ("p5", True, False)])
def test_creation_and_handoff_equal_the_restatement(sd, name, u16, distorted):
    """4 slots x 2 frames after TrackWithMotionModel + TrackLocalMap.  Per frame three creation calls with different th_depth
    (the median depth of slot 0 -- one keypoint's depth exactly; one below every depth; one above), then one with
    use_flags = 1 and flags [1, 0, 1, 1]; the hand-off carries the last call's points.  Slot 2 has fewer than 101 candidates,
    slot 3 is not tracked."""
    rig = Rig(sd, CFGS[name], [101, 102, 103, 104], 3, u16=u16, distorted=distorted)
    trk, B = rig.trk, rig.B
    seen = set()
    try:
        next_id = np.array([1000, 20000, 300000, 4000000], np.int32)
        trk.set_next_map_id(0, next_id)
        for t in range(1, rig.T):
            rig.track(t)
            _, dd = trk.get_stereo(0, B)
            kk, ku, cd, cn = rig.keys_un()
            gl, gp, old, Tc, tw = trk.get_local_map(0, B), trk.get_pose_opt(0, B), trk.get_last(0, B), trk.get_align(0, B)["T"], trk.get_tracked(0, B)
            assert gl["status"][:3].tolist() == [2, 2, 2] and gl["status"][3] != 2, (t, gl["status"])
            pos = np.sort(dd[0, :cn[0]][dd[0, :cn[0]] > 0])
            calls = [(pos[len(pos) // 2], False), (np.float32(0.5), False), (np.float32(9.0), False), (pos[len(pos) // 3], True)]
            flags = np.array([1, 0, 1, 1], np.uint8)
            trk.set_keyframe_flags(0, flags)
            assert trk.get_keyframe_flags(0, B).tolist() == flags.tolist()
            for th, use_flags in calls:
                trk.create_keyframe_points(B, 1, th, use_flags=use_flags, frame_id=t)
                got = trk.get_created(0, B)
                for b in range(B):
                    key = (name, t, b, float(th), use_flags)
                    n = cn[b]
                    d, m, ol = dd[b, :n], gl["match"][b, :n], gp["outlier"][b, :n]
                    if b == 3 or (use_flags and not flags[b]):
                        assert (got["mode"][b], got["created"][b], got["P"][b], got["candidates"][b]) == (0, 0, 0, 0), key
                        assert (got["kp_index"][b] == -1).all(), key
                        continue
                    lobs = local_obs_of(rig, b)
                    want, P, cand = R.create_new_keyframe(d, th, m, M, old["obs"][b], lobs)
                    check_created(got, b, want, P, cand, ku, d, Tc[b], int(next_id[b]), key)
                    next_id[b] += len(want)
                    # which branches of the loop this call took
                    z = np.sort(d[d > 0])
                    n_close = int((z <= th).sum())
                    if cand >= 101:
                        seen.add("a" if n_close >= 100 else "b")
                    else:
                        seen.add("c")
                        assert P == cand, key
                    if P < cand and (z[:P] == th).any():
                        seen.add("d")
                    if len(np.unique(z[:P])) < P:
                        seen.add("e")
                    order = sorted((float(d[i]), i) for i in range(n) if d[i] > 0)
                    inside = {i for _, i in order[:P]}
                    obs_m = np.array([R.point_obs(v, M, old["obs"][b], lobs) if v >= 0 else 1 for v in m])
                    vo = np.nonzero((m >= 0) & (obs_m < 1) & (d > 0))[0]
                    if any(i in inside for i in vo) and any(i not in inside for i in vo):
                        seen.add("f")
                        assert all((i in want) == (i in inside) for i in vo), key
                    kept_out = np.nonzero((m >= 0) & (obs_m >= 1) & ol & (d > 0))[0]
                    if any(i in inside for i in kept_out):
                        seen.add("g")
                        assert not set(kept_out) & set(want), key
                    # keypoints on zero / NaN / negative depth carry no depth (mvDepth -1) and are no candidates
                    rows = np.round(kk[b]["y"][:n]).astype(int)
                    nan_band, neg_band = (rows >= 101) & (rows < 129), (rows >= 301) & (rows < 319)
                    if (d <= 0).any() and (u16 or (nan_band.any() and neg_band.any())):
                        seen.add("h")
                        assert u16 or ((d[nan_band] <= 0).all() and (d[neg_band] <= 0).all()), key
                        assert cand == int((d > 0).sum()) and not any(d[i] <= 0 for i in want), key
                    if any(ol[i] for i in want):
                        seen.add("created_outlier")
            last_call = got
            trk.advance(B, 1)
            new = trk.get_last(0, B)
            for b in range(B):
                n = cn[b]
                prev = {k: old[k][b] for k in LAST_KEYS}
                c = int(last_call["created"][b])
                created = dict(kp_index=last_call["kp_index"][b, :c], Xw=last_call["Xw"][b, :c], ids=last_call["ids"][b, :c])
                want = R.handoff(M, kk[b], n, gl["match"][b], gp["outlier"][b], prev, old["ids"][b], rig.local[b], rig.lids[b], created, cd[b])
                assert new["n_last"][b] == n
                for k in LAST_KEYS + ("ids",):
                    assert np.array_equal(new[k][b], want[k]), (name, t, b, k)
                assert want["angle"][:n].tolist() == ku[b]["angle"][:n].tolist()
        assert {"a", "b", "c", "d", "e", "f", "g", "h", "created_outlier"} <= seen, seen
    finally:
        rig.close()


def test_advance_without_a_creation_call_is_unchanged(sd):
    """No creation call on the extraction: the hand-off is the plain restatement (created = None)."""
    rig = Rig(sd, CFGS["p8"], [111, 112], 3)
    trk, B = rig.trk, rig.B
    try:
        for t in range(1, rig.T):
            rig.track(t)
            if t == 1:
                trk.create_keyframe_points(B, 1, 2.0, frame_id=t)      # an earlier extraction's points must not leak into t = 2
            kk, ku, cd, cn = rig.keys_un()
            gl, gp, old = trk.get_local_map(0, B), trk.get_pose_opt(0, B), trk.get_last(0, B)
            trk.advance(B, 1)
            new = trk.get_last(0, B)
            if t == 1:
                continue
            for b in range(B):
                prev = {k: old[k][b] for k in LAST_KEYS}
                want = R.handoff(M, kk[b], cn[b], gl["match"][b], gp["outlier"][b], prev, old["ids"][b], rig.local[b], rig.lids[b])
                for k in LAST_KEYS + ("ids",):
                    assert np.array_equal(new[k][b], want[k]), (t, b, k)
    finally:
        rig.close()


def test_stereo_init_then_track_from_created_points(sd):
    """stereo_init on frame 0: ids in keypoint order, Tref the identity, Xw bit-equal; slot 3 (a blank image: no keypoints)
    keeps its previous last frame.  Then frames 1..3 track from the created points alone (TrackWithMotionModel, source 0),
    refilled by creation calls driven through set_keyframe_flags, each equal to the restatement."""
    rig = Rig(sd, CFGS["p8"], [121, 122, 123, 124], 4, static=False)
    trk, B = rig.trk, rig.B
    try:
        rig.views[0, 3] = 128
        rk, rd, rn = trk.ref.extract_batch(rig.views[0])                   # a previous last frame for slot 3
        keep = synth.static_map(rk[0, :rn[0]], rd[0, :rn[0]], np.eye(4), seed=1)[1]
        trk.set_last(3, [keep])
        Tk = synth.se3_exp((0.1, 0.0, 0.0), (0.0, 0.1, 0.0))
        trk.set_poses(3, [Tk], [Tk])
        before = trk.get_last(0, B)
        assert _code(sd, lambda: trk.advance(B, 2)) == 1                  # stereo_init has not run
        trk.cur.extract_batch(rig.views[0])
        rig.stereo(0)
        next_id = np.array([0, 5000, 10000, 15000], np.int32)
        trk.set_next_map_id(0, next_id)
        trk.stereo_init(B, 500)
        got = trk.get_created(0, B)
        _, dd = trk.get_stereo(0, B)
        kk, ku, cd, cn = rig.keys_un()
        assert _code(sd, lambda: trk.advance(B, 0)) == 1                  # no tracking call ran
        trk.advance(B, 2)
        new = trk.get_last(0, B)
        trk.set_prior(0, [np.eye(4)] * B, relative=True)                  # Tprior = I * Tref: reads Tref back
        Tref = trk.get_align(0, B)["T"]
        assert cn[3] <= 500 and got["mode"][3] == 0 and got["created"][3] == 0
        for k in before:
            assert np.array_equal(new[k][3], before[k][3]), k
        assert np.array_equal(Tref[3], Tk)
        for b in range(3):
            n = cn[b]
            want = R.stereo_initialization(dd[b, :n], 500)
            c = len(want)
            assert c > (300 if b < 2 else 0) and (got["mode"][b], got["created"][b], got["P"][b], got["candidates"][b]) == (2, c, c, c), b
            assert got["kp_index"][b, :c].tolist() == want and got["ids"][b, :c].tolist() == list(range(next_id[b], next_id[b] + c))
            for r, i in enumerate(want):
                assert np.array_equal(got["Xw"][b, r], R.unproject_stereo(ku[b]["x"][i], ku[b]["y"][i], dd[b, i], K, np.eye(4))), (b, i)
            created = dict(kp_index=want, Xw=got["Xw"][b, :c], ids=got["ids"][b, :c])
            h = R.handoff(M, kk[b], n, None, None, None, None, None, None, created, cd[b])
            assert new["n_last"][b] == n and np.array_equal(Tref[b], np.eye(4))
            for k in LAST_KEYS + ("ids",):
                assert np.array_equal(new[k][b], h[k]), (b, k)
            next_id[b] += c
        # the streams go on from their own points; the true pose of frame t relative to frame 0
        for t in range(1, rig.T):
            trk.cur.extract_batch(rig.views[t])
            rig.stereo(t)
            rel = [s["T"][t] @ np.linalg.inv(s["T"][0]) for s in rig.seqs]
            trk.set_prior(0, rel, relative=False)
            trk.track_with_motion_model(B, th=15.0, mono=False, align_mode=0)
            tw, (fm, _), old, Tc = trk.get_tracked(0, B), trk.get_matches(0, B), trk.get_last(0, B), trk.get_align(0, B)["T"]
            _, dd = trk.get_stereo(0, B)
            kk, ku, cd, cn = rig.keys_un()
            assert tw["status"][:2].tolist() == [2, 2], (t, tw)
            flags = np.array([1, t % 2, 1, 1], np.uint8)
            trk.set_keyframe_flags(0, flags)
            trk.create_keyframe_points(B, 0, 2.0, use_flags=True, frame_id=t)
            got = trk.get_created(0, B)
            trk.advance(B, 0)
            new = trk.get_last(0, B)
            for b in range(B):
                n = cn[b]
                created = None
                if flags[b] and tw["status"][b] == 2:
                    want, P, cand = R.create_new_keyframe(dd[b, :n], np.float32(2.0), fm[b, :n], M, old["obs"][b], np.zeros(M, np.int32))
                    check_created(got, b, want, P, cand, ku, dd[b, :n], Tc[b], int(next_id[b]), (t, b))
                    next_id[b] += len(want)
                    created = dict(kp_index=want, Xw=got["Xw"][b, :len(want)], ids=got["ids"][b, :len(want)])
                    assert len(want) > 0
                else:
                    assert got["created"][b] == 0 and got["mode"][b] == 0
                prev = {k: old[k][b] for k in LAST_KEYS}
                h = R.handoff(M, kk[b], n, fm[b], np.zeros(n, bool), prev, old["ids"][b], None, None, created, cd[b])
                for k in LAST_KEYS + ("ids",):
                    assert np.array_equal(new[k][b], h[k]), (t, b, k)
                if b < 2:
                    assert np.abs(Tc[b][:3, 3] - rel[b][:3, 3]).max() < 0.02, (t, b)
    finally:
        rig.close()


def test_need_keyframe_equals_the_restatement(sd):
    """The decision on the device's own counts and mnMatchesInliers, over a table of per-slot states: every condition, both
    busy-mapper outcomes, and mnLastKeyFrameId written by a creation call and kept by SD_KF_KEEP."""
    rig = Rig(sd, CFGS["p8"], [131, 132, 133, 134], 2)
    trk, B = rig.trk, rig.B
    try:
        rig.track(1)
        assert _code(sd, lambda: trk.need_keyframe(B, 1, 10, 0, 30)) == 1            # close_points has not run
        trk.need_keyframe(B, 0, 10, 0, 30)                                           # not RGB-D: no counts needed
        _, dd = trk.get_stereo(0, B)
        _, _, cn = trk.cur.download(0, B)
        pos = np.sort(dd[0, :cn[0]][dd[0, :cn[0]] > 0])
        outcomes = set()
        for th in (pos[len(pos) // 2], pos[50]):
            trk.close_points(B, 1, th)
            cp, gl = trk.get_close_points(0, B), trk.get_local_map(0, B)
            inl = int(gl["n_inliers"][0])
            assert inl > 40
            table = []
            for nkfs in (1, 5, 40):
                for nref in (inl, int(inl / 0.75) + 1, 4 * inl, 4 * inl + 1, 10):
                    for last_kf, last_reloc in ((0, 0), (95, 0), (99, 90)):
                        for fl in (0, 1, 2, 4, 5):
                            table.append((nkfs, nref, last_kf, last_reloc, fl, 0, 0, 0))
            table = np.array(table, np.int32)
            for rgbd in (1, 0):
                for k in range(0, len(table), B):
                    st = table[k:k + B]
                    if len(st) < B:
                        break
                    trk.set_keyframe_state(0, st)
                    trk.need_keyframe(B, rgbd, 100, 5, 30)
                    got = trk.get_keyframe_flags(0, B)
                    for b in range(B):
                        want = R.need_new_keyframe(gl["status"][b] == 2, int(gl["n_inliers"][b]), int(cp["tracked"][b]),
                                                   int(cp["non_tracked"][b]), st[b], rgbd, 100, 5, 30)
                        assert got[b] == want, (float(th), rgbd, st[b].tolist(), got[b], want)
                        outcomes.add((rgbd, int(got[b])))
            assert got[3] == 0                                                       # slot 3 is not tracked
        assert {(1, 0), (1, 1), (1, 2), (1, 3), (0, 0), (0, 1), (0, 2)} <= outcomes, outcomes
        # a creation call writes mnLastKeyFrameId = frame_id; SD_KF_KEEP leaves it
        idle = np.array([[5, 4 * inl, 0, 0, 1, 0, 0, 0]] * B, np.int32)
        trk.set_keyframe_state(0, idle)
        trk.need_keyframe(B, 1, 100, 5, 30)
        assert trk.get_keyframe_flags(0, B)[:3].tolist() == [1, 1, 1]
        trk.create_keyframe_points(B, 1, 2.0, use_flags=True, frame_id=100)
        assert (trk.get_created(0, B)["mode"][:3] == 1).all()
        idle[:, 2] = trk.KF_KEEP
        trk.set_keyframe_state(0, idle)
        trk.need_keyframe(B, 1, 104, 5, 30)                                          # 104 < 100 + 5: c1b fails now
        assert trk.get_keyframe_flags(0, B).tolist() == [0, 0, 0, 0]
        trk.need_keyframe(B, 1, 105, 5, 30)
        assert trk.get_keyframe_flags(0, B)[:3].tolist() == [1, 1, 1]
    finally:
        rig.close()


def test_creation_errors(sd):
    rig = Rig(sd, CFGS["p8"], [141, 142], 2)
    trk, B = rig.trk, rig.B
    try:
        trk.cur.extract_batch(rig.views[1])
        rig.stereo(1)
        for src in (0, 1):
            assert _code(sd, lambda: trk.create_keyframe_points(B, src, 2.0)) == 1   # no tracking call on this extraction
        assert _code(sd, lambda: trk.need_keyframe(B, 1, 1, 0, 30)) == 1
        trk.set_prior(0, rig.vel(1), relative=True)
        trk.track_with_motion_model(B, th=15.0, mono=False, align_mode=0)
        assert _code(sd, lambda: trk.create_keyframe_points(B, 1, 2.0)) == 1         # TrackLocalMap did not run
        assert _code(sd, lambda: trk.create_keyframe_points(B, 2, 2.0)) == 1         # bad source
        assert _code(sd, lambda: trk.create_keyframe_points(B + 1, 0, 2.0)) == 3
        assert _code(sd, lambda: trk.stereo_init(B + 1)) == 3
        assert _code(sd, lambda: trk.need_keyframe(B + 1, 1, 1, 0, 30)) == 3
        assert _code(sd, lambda: trk.set_keyframe_state(1, np.zeros((B, 8), np.int32))) == 3
        assert _code(sd, lambda: trk.set_keyframe_flags(1, np.zeros(B, np.uint8))) == 3
        assert _code(sd, lambda: trk.set_next_map_id(B, [0])) == 3
        trk.set_current_broadcast(0)
        assert _code(sd, lambda: trk.create_keyframe_points(B, 0, 2.0)) == 1
        assert _code(sd, lambda: trk.stereo_init(B)) == 1
        trk.set_current_broadcast(-1)
        trk.create_keyframe_points(B, 0, 2.0)
        c = trk.get_created(0, B)
        assert c["created"][0] > 1
        assert _code(sd, lambda: trk.get_created(0, B, cap=int(c["created"][0]) - 1)) == 3
        assert _code(sd, lambda: trk.advance(B, 2)) == 1                            # keyframe points, not an initialisation
        trk.advance(B, 0)
    finally:
        rig.close()


POSE_TOL = 1e-5


def _download(sd, ptr, nbytes):
    import ctypes as C
    from sdslam_amd import capi
    out = np.zeros(nbytes, np.uint8)
    capi._check(capi.lib().sd_dev_download(out.ctypes.data_as(C.c_void_p), ptr, nbytes))
    return out


def _device_loop(sd, KL, seqs, views, depth, next_id0, sync):
    """The odometry loop of tests/keyframe_loop.py on the device, frames and f32 depth resident in HBM: stereo_init + advance(2)
    on frame 0, then per frame extraction -> depth -> prior -> TrackWithMotionModel -> TrackLocalMap (empty local map) ->
    close_points -> need_keyframe -> create_keyframe_points(use_flags) -> records -> advance.  The keyframe state is uploaded
    every frame with SD_KF_KEEP for mnLastKeyFrameId.  sync: getters after every stage (returned per frame); otherwise nothing
    but queued calls inside the loop."""
    T, B = views.shape[0], views.shape[1]
    F = W * H
    frames, dmaps, rec = sd.DeviceBuffer(views.nbytes), sd.DeviceBuffer(depth.nbytes), sd.DeviceBuffer(T * B * 160)
    frames.upload(views)
    dmaps.upload(depth)
    ext = [sd.ORBextractor(*KL.CFG, W, H, B) for _ in range(2)]
    trk = sd.Tracker(ext[0], ext[1], max_points=M, max_batch=B, pnp_max_iterations=100)
    log = []
    try:
        trk.set_camera(*K, KL.BF, BOUNDS)
        state = np.array([KL.STATE] * B, np.int32)
        trk.set_next_map_id(0, np.asarray(next_id0, np.int32))
        trk.set_keyframe_state(0, state)
        state[:, 2] = trk.KF_KEEP
        trk.cur.extract_batch_device(frames.ptr.value, B, W, H)
        trk.stereo_from_depth_device(dmaps.ptr.value, F32, W, H)
        trk.stereo_init(B, 500)
        if sync:
            log.append(dict(created=trk.get_created(0, B)))
        trk.advance(B, 2)
        if sync:
            log[-1]["last"] = trk.get_last(0, B)
        for t in range(1, T):
            trk.cur.extract_batch_device(frames.ptr.value + t * B * F, B, W, H)
            trk.stereo_from_depth_device(dmaps.ptr.value + t * B * F * 4, F32, W, H)
            trk.set_prior(0, KL.velocity(seqs, t), relative=True)
            trk.set_keyframe_state(0, state)
            trk.track_with_motion_model(B, th=KL.TH_MM, mono=False, align_mode=0)
            trk.track_local_map(B, th=KL.TH_LM, min_inliers=30)
            trk.close_points(B, 1, KL.TH_DEPTH)
            trk.need_keyframe(B, 1, t, KL.MIN_FRAMES, KL.MAX_FRAMES)
            trk.create_keyframe_points(B, 1, KL.TH_DEPTH, use_flags=True, frame_id=t)
            trk.pack_records(B, 3, rec.ptr.value + t * B * 160)
            if sync:
                log.append(dict(tw=trk.get_tracked(0, B), fm=trk.get_matches(0, B)[0], gl=trk.get_local_map(0, B), gp=trk.get_pose_opt(0, B),
                                close=trk.get_close_points(0, B), flags=trk.get_keyframe_flags(0, B), created=trk.get_created(0, B),
                                n=trk.cur.download(0, B)[2]))
            trk.advance(B, 1)
            if sync:
                log[-1]["last"] = trk.get_last(0, B)
        final = dict(last=trk.get_last(0, B), rec=_download(sd, rec.ptr, T * B * 160)[B * 160:], flags=trk.get_keyframe_flags(0, B))
        c = trk.get_created(0, B)
        final.update({"c_" + k: v for k, v in c.items()})
        return log, final
    finally:
        trk.close()
        for e in ext:
            e.close()
        for d in (frames, dmaps, rec):
            d.free()


def test_closed_loop_equals_the_oracle_loop_and_queued_equals_synchronised(sd, oracle):
    """2 streams x 12 frames from stereo_init, nothing but the streams' own created points (n_local = 0; sd_track_local_map is
    usable with it).  Synchronised run: per frame and slot, statuses, counts, match vectors, close-point counts, keyframe
    flags, created index lists and ids equal the oracle loop's; poses and created Xw within 1e-5; the handed-off last frame
    equal (Xw within 1e-5).  Queued run, no getter inside the loop: records, final last frame, flags and the last creation
    record equal the synchronised run's byte for byte."""
    import keyframe_loop as KL
    seqs, views, depth = KL.sequences()
    ids0 = [0, 100000]
    want = KL.oracle_loop(oracle, seqs, views, depth, ids0)
    log, fin_sync = _device_loop(sd, KL, seqs, views, depth, ids0, sync=True)
    B = views.shape[1]
    keyframes = 0

    def same_created(got, b, w, mode, key):
        c = len(w["created"])
        assert (got["mode"][b], got["created"][b]) == ((mode, c) if c or mode == 2 else (0, 0)), key
        assert got["kp_index"][b, :c].tolist() == list(w["created"]) and got["ids"][b, :c].tolist() == list(w["ids"]), key
        if c:
            assert np.abs(got["Xw"][b, :c] - w["Xw"]).max() <= POSE_TOL, key

    def same_last(got, b, h, key):
        for k in ("valid", "desc", "octave", "angle", "obs", "ids"):
            assert np.array_equal(got[k][b], h[k]), (key, k)
        assert np.abs(got["Xw"][b] - h["Xw"]).max() <= POSE_TOL, key

    for b in range(B):
        same_created(log[0]["created"], b, want[b][0], 2, (0, b))
        same_last(log[0]["last"], b, want[b][0]["last"], (0, b))
        for t in range(1, len(log)):
            g, w, key = log[t], want[b][t], (t, b)
            n = g["n"][b]
            assert (g["tw"]["status"][b], g["tw"]["nmatches"][b], g["tw"]["nmatches_map"][b]) == (w["status_mm"], w["nmatches"], w["nmatches_map"]), key
            assert np.array_equal(g["fm"][b, :n], w["match_mm"]) and np.array_equal(g["gl"]["match"][b, :n], w["match"]), key
            assert (g["gl"]["status"][b], g["gl"]["n_inliers"][b], g["gl"]["n_local"][b]) == (w["status"], w["n_inliers"], 0), key
            assert np.array_equal(g["gp"]["outlier"][b, :n], w["outlier"]), key
            assert np.abs(g["gp"]["T"][b] - w["T"]).max() <= POSE_TOL, (key, np.abs(g["gp"]["T"][b] - w["T"]).max())
            assert (g["close"]["tracked"][b], g["close"]["non_tracked"][b]) == w["close"], key
            assert g["flags"][b] == w["flag"], key
            same_created(g["created"], b, w, 1, key)
            if w["flag"] & 1:
                assert (g["created"]["P"][b], g["created"]["candidates"][b]) == (w["P"], w["candidates"]), key
                keyframes += 1
            same_last(g["last"], b, w["last"], key)
            assert g["gl"]["status"][b] == 2, key
    assert keyframes >= 2 * B
    _, fin_q = _device_loop(sd, KL, seqs, views, depth, ids0, sync=False)
    assert set(fin_q) == set(fin_sync)
    for k in fin_sync:
        if k == "last":
            for kk in fin_sync[k]:
                assert np.array_equal(fin_sync[k][kk], fin_q[k][kk]), kk
        else:
            assert np.array_equal(fin_sync[k], fin_q[k]), k
    recs = fin_q["rec"].view(np.float64).reshape(-1, 20)
    assert (recs[:, 19] == 1).all()
