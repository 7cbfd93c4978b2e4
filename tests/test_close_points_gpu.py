"""GPU: the RGB-D close-point counts of Tracking::NeedNewKeyFrame on the device (sd_track_close_points,
sd_track_get_close_points).

Bars: in a closed RGB-D loop (TrackWithMotionModel [+ TrackLocalMap] + the hand-off, both sources), every frame's counts
equal a numpy restatement of src/Tracking.cc:776-789 after "Clean VO matches" (:250-257) over the getters, and a keypoint
counts as tracked exactly when sd_track_advance keeps its map point.  The errors of the call are pinned."""
import numpy as np
import pytest

from sdslam_amd import synth

pytestmark = pytest.mark.gpu
K = (synth.FX, synth.FY, synth.CX, synth.CY)
BOUNDS = (0.0, 640.0, 0.0, 480.0)
CFG = (1000, 1.2, 8, 20)
W, H = 640, 480
M = 1000
BF = 4.0


@pytest.fixture(scope="module")
def sd():
    import sdslam_amd
    if sdslam_amd.device_count() < 1:
        pytest.fail("no HIP device: the gpu-marked tests need a real MI355X")
    return sdslam_amd


class Rig:
    """B RGB-D streams (one sequence seed each, depth with a hole every 9th column), frame 0 extracted into `ref` as the
    first last frame, a static map of it as last frame and local map, ids set."""

    def __init__(self, sd, seeds, T):
        self.B, self.T = len(seeds), T
        self.seqs = [synth.make_sequence(s, T, with_depth=True) for s in seeds]
        self.views = np.stack([s["views"] for s in self.seqs], 1)          # [T][B][H][W]
        self.depth = np.stack([s["depth"] for s in self.seqs], 1)
        self.depth[..., ::9] = 0.0
        self.ext = [sd.ORBextractor(*CFG, W, H, self.B) for _ in range(2)]
        self.trk = sd.Tracker(self.ext[0], self.ext[1], max_points=M, max_batch=self.B, pnp_max_iterations=100)
        self.trk.set_camera(*K, BF, BOUNDS)
        rk, rd, rn = self.trk.ref.extract_batch(self.views[0])
        maps = [synth.static_map(rk[b, :rn[b]], rd[b, :rn[b]], self.seqs[b]["T"][0], seed=b) for b in range(self.B)]
        self.local_obs = np.zeros((self.B, M), np.int32)
        for b, m in enumerate(maps):
            self.local_obs[b, :len(m[0]["obs"])] = m[0]["obs"]
        self.trk.set_last(0, [m[1] for m in maps])
        self.trk.set_local(0, [m[0] for m in maps])
        self.trk.set_map_ids(0, [m[2] for m in maps], 0)
        self.trk.set_map_ids(0, [m[2] for m in maps], 1)
        T0 = [s["T"][0] for s in self.seqs]
        self.trk.set_poses(0, T0, T0)

    def vel(self, t):
        return [s["T"][t] @ np.linalg.inv(s["T"][t - 1]) for s in self.seqs]

    def close(self):
        self.trk.close()
        for e in self.ext:
            e.close()


def _code(sd, fn):
    with pytest.raises(sd.SdError) as e:
        fn()
    return e.value.code


def test_close_points_equal_restatement_and_handoff(sd):
    """3 streams x 7 frames; every third frame hands off after TrackWithMotionModel (source 0), the others after
    TrackLocalMap (source 1).  th_depth is the median depth of slot 0, i.e. one keypoint's depth exactly (excluded: the
    test is strict).  A second call on 2 slots with another threshold leaves the counts of slots 2.. alone."""
    R = Rig(sd, [91, 92, 93], 7)
    trk, B = R.trk, R.B
    seen = set()
    try:
        for t in range(1, R.T):
            source = 0 if t % 3 == 0 else 1
            trk.cur.extract_batch(R.views[t])
            trk.stereo_from_depth(R.depth[t])
            for src in (0, 1):                                    # nothing has run on this extraction
                assert _code(sd, lambda: trk.close_points(B, src, 1.0)) == 1
            trk.set_prior(0, R.vel(t), relative=True)
            trk.track_with_motion_model(B, th=15.0, mono=False, align_mode=0)
            if source == 1:
                assert _code(sd, lambda: trk.close_points(B, 1, 1.0)) == 1
                trk.track_local_map(B, th=3.0, min_inliers=30)
            _, dd = trk.get_stereo(0, B)
            _, _, cn = trk.cur.download(0, B)
            pos = np.sort(dd[0, :cn[0]][dd[0, :cn[0]] > 0])
            th = pos[len(pos) // 2]
            th2 = np.float32(th * np.float32(0.9))
            trk.close_points(B, source, th)
            got = trk.get_close_points(0, B)
            (fm, _), gl, gp, old = trk.get_matches(0, B), trk.get_local_map(0, B), trk.get_pose_opt(0, B), trk.get_last(0, B)
            trk.close_points(2, source, th2)
            part = trk.get_close_points(0, B)
            trk.advance(B, source)
            new = trk.get_last(0, B)
            match = fm if source == 0 else gl["match"]
            for b in range(B):
                key = (t, b, source)
                n = cn[b]
                d, m, ol = dd[b, :n], match[b, :n], gp["outlier"][b, :n]
                obs = np.where(m >= M, R.local_obs[b][np.clip(m - M, 0, M - 1)], old["obs"][b][np.clip(m, 0, M - 1)])
                kept = (m >= 0) & (obs >= 1)
                if source == 1:
                    kept &= ~ol
                close = (d > 0) & (d < th)
                assert (got["tracked"][b], got["non_tracked"][b]) == ((close & kept).sum(), (close & ~kept).sum()), key
                assert np.array_equal(new["valid"][b, :n] == 1, kept), key        # what sd_track_advance kept
                close2 = (d > 0) & (d < th2)
                want2 = ((close2 & kept).sum(), (close2 & ~kept).sum()) if b < 2 else (got["tracked"][b], got["non_tracked"][b])
                assert (part["tracked"][b], part["non_tracked"][b]) == want2, key
                assert got["tracked"][b] > 0 and got["non_tracked"][b] > 0, key
                if (d == th).any():
                    seen.add("depth == th")
                if (close & (m >= 0) & (obs < 1)).any():
                    seen.add("obs0")
                if source == 1 and (close & (m >= 0) & (obs >= 1) & ol).any():
                    seen.add("outlier")
                if (close & kept & (m >= M)).any():
                    seen.add("local")
                if source == 0 and (close & kept).any():
                    seen.add("source 0")
            for src in (0, 1):                                    # the hand-off ended this extraction's results
                assert _code(sd, lambda: trk.close_points(B, src, th)) == 1
        assert {"depth == th", "obs0", "outlier", "local", "source 0"} <= seen, seen
    finally:
        R.close()


def test_close_points_errors(sd):
    """SD_ERR_CAPACITY for n_frames outside 1..max_batch and a getter range beyond it; SD_ERR_INVALID_ARG for a bad source,
    before the named call ran, for more slots than it ran on, in broadcast mode, and for a NULL output."""
    R = Rig(sd, [94, 95], 2)
    trk, B = R.trk, R.B
    try:
        assert _code(sd, lambda: trk.close_points(B + 1, 0, 1.0)) == 3
        assert _code(sd, lambda: trk.close_points(0, 0, 1.0)) == 3
        trk.cur.extract_batch(R.views[1])
        trk.stereo_from_depth(R.depth[1])
        trk.set_prior(0, R.vel(1), relative=True)
        trk.track_with_motion_model(B, th=15.0, mono=False)
        for src in (-1, 2):
            assert _code(sd, lambda: trk.close_points(B, src, 1.0)) == 1
        trk.set_current_broadcast(0)
        assert _code(sd, lambda: trk.close_points(B, 0, 1.0)) == 1
        trk.set_current_broadcast(-1)
        trk.close_points(B, 0, 2.0)
        got = trk.get_close_points(0, B)
        assert (got["tracked"] + got["non_tracked"] > 0).all()
        assert _code(sd, lambda: trk.get_close_points(1, B)) == 3
        assert trk.L.sd_track_get_close_points(trk.h, 0, 1, None) == 1
        trk.track_with_motion_model(1, th=15.0, mono=False)       # ran on slot 0 only
        assert _code(sd, lambda: trk.close_points(B, 0, 1.0)) == 1
        trk.close_points(1, 0, 1.0)
    finally:
        R.close()
