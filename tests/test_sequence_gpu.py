"""GPU: sequential tracking with the last-frame hand-off on the device (sd_track_advance, sd_track_set_map_ids,
sd_track_set_prior, sd_track_get_last).

B camera streams are tracked frame after frame: the result of frame t (mvpMapPoints, mvbOutlier, pose) becomes the last
frame of frame t+1 without a host round trip.  Bars: the hand-off equals a host restatement of src/Tracking.cc:250-292 applied
to the device's own outputs, bit for bit; the closed loop equals the CPU oracle driven through the same loop (statuses,
counts and match vectors equal, poses within 1e-5); queued and synchronised loops are identical."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

_CHILD = os.environ.get("SD_SEQUENCE_CHILD") == "1"
if _CHILD:
    import torch as _torch_first  # noqa: F401  (before the library: one HIP runtime in the process)

from sdslam_amd import synth  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = (synth.FX, synth.FY, synth.CX, synth.CY)
BOUNDS = (0.0, 640.0, 0.0, 480.0)
CFGS = {"p8": (1000, 1.2, 8, 20), "p5": (1000, 2.0, 5, 20)}
M = 1000
POSE_TOL = 1e-5
SLEEP = 90_000_000


@pytest.fixture(scope="module")
def sd():
    import sdslam_amd
    if sdslam_amd.device_count() < 1:
        pytest.fail("no HIP device: the gpu-marked tests need a real MI355X")
    return sdslam_amd


def prior_product(V, L):
    """V @ L summed k = 0..3 in order, every product and sum rounded on its own (what sd_track_set_prior computes)."""
    P = V[:, 0:1] * L[0:1, :]
    for k in range(1, 4):
        P = P + V[:, k:k + 1] * L[k:k + 1, :]
    return P


def host_handoff(kps, N, match, outlier, last, last_ids, local, local_ids):
    """src/Tracking.cc:250-292 on the host: mvpMapPoints[i] = match[i] (< M: last-frame point, >= M: local point - M), dropped
    where Observations() < 1 ("Clean VO matches") or mvbOutlier; mLastFrame = Frame(mCurrentFrame).  [M]-padded arrays, zeros
    and id -1 where no point is kept; octave / angle of the keypoint for i < N."""
    out = dict(valid=np.zeros(M, np.uint8), Xw=np.zeros((M, 3)), desc=np.zeros((M, 32), np.uint8), octave=np.zeros(M, np.int32),
               angle=np.zeros(M, np.float32), obs=np.zeros(M, np.int32), ids=np.full(M, -1, np.int32))
    out["octave"][:N] = kps["octave"][:N]
    out["angle"][:N] = kps["angle"][:N]
    for i in range(N):
        m = int(match[i])
        if m < 0 or outlier[i]:
            continue
        src, ids, j = (local, local_ids, m - M) if m >= M else (last, last_ids, m)
        if src["obs"][j] < 1:
            continue
        out["valid"][i], out["Xw"][i], out["desc"][i] = 1, src["Xw"][j], src["desc"][j]
        out["obs"][i], out["ids"][i] = src["obs"][j], ids[j]
    return out


def as_last(h, N):
    """The oracle's last-frame dict (arrays of the last frame's N keypoints) from a hand-off result."""
    return {k: np.ascontiguousarray(h[k][:N]) for k in ("valid", "Xw", "desc", "octave", "angle", "obs")}, h["ids"][:N].copy()


def check_last(got, f, want, N, what):
    assert got["n_last"][f] == N, what
    for k in ("valid", "Xw", "desc", "octave", "angle", "obs", "ids"):
        assert np.array_equal(got[k][f], want[k]), (what, k)


class Loop:
    """B streams of one sequence seed each: device tracker and the oracle's restatement of the same loop.  w x h: the frame size
    (synth's camera K behind bounds (0, w, 0, h))."""

    def __init__(self, sd, oracle, cfg, seeds, T, rgbd=False, w=640, h=480):
        self.cfg, self.B, self.T, self.rgbd = cfg, len(seeds), T, rgbd
        self.bounds = (0.0, float(w), 0.0, float(h))
        self.seqs = [synth.make_sequence(s, T, w=w, h=h, with_depth=rgbd) for s in seeds]
        self.views = np.stack([s["views"] for s in self.seqs], 1)          # [T][B][H][W]
        self.ext = [sd.ORBextractor(*cfg, w, h, self.B) for _ in range(2)]
        self.trk = sd.Tracker(self.ext[0], self.ext[1], max_points=M, max_batch=self.B, pnp_max_iterations=100)
        self.bf = 4.0 if rgbd else 0.0
        self.trk.set_camera(*K, self.bf, self.bounds)
        rk, rd, rn = self.trk.ref.extract_batch(self.views[0])
        self.local, self.lids, lasts, self.o_last, self.o_ids = [], [], [], [], []
        self.o_ext = []
        self.o_T = []
        for b in range(self.B):
            oc = oracle.OrbOracle(*cfg)
            ok_, od = oc.extract(self.views[0][b])
            assert np.array_equal(ok_, rk[b, :rn[b]])
            loc, last, ids = synth.static_map(ok_, od, self.seqs[b]["T"][0], cfg[1], cfg[2], seed=b)
            self.local.append(loc)
            self.lids.append(ids)
            lasts.append(last)
            self.o_last.append(last)
            self.o_ids.append(ids.copy())
            self.o_ext.append([oc, oracle.OrbOracle(*cfg)])                   # [ref, cur]
            self.o_T.append(self.seqs[b]["T"][0])
        self.tab = self.o_ext[0][0].tables()
        self.trk.set_last(0, lasts)
        self.trk.set_local(0, self.local)
        self.trk.set_map_ids(0, self.lids, which=0)
        self.trk.set_map_ids(0, self.lids, which=1)
        self.trk.set_poses(0, [s["T"][0] for s in self.seqs], [s["T"][0] for s in self.seqs])

    def vel(self, t):
        return [s["T"][t] @ np.linalg.inv(s["T"][t - 1]) for s in self.seqs]

    def close(self):
        self.trk.close()
        for e in self.ext:
            e.close()

    def device_step(self, t, th_mm, th_lm, source=1):
        trk, B = self.trk, self.B
        trk.cur.extract_batch(self.views[t])
        if self.rgbd:
            trk.stereo_from_depth(np.stack([s["depth"][t] for s in self.seqs]))
        trk.set_prior(0, self.vel(t), relative=True)
        trk.track_with_motion_model(B, th=th_mm, mono=not self.rgbd, align_mode=0)
        if source == 1:
            trk.track_local_map(B, th=th_lm, min_inliers=30)

    def oracle_step(self, oracle, t, b, th_mm, th_lm, u_right=None):
        """TrackWithMotionModel + TrackLocalMap + the hand-off for stream b, on the oracle's own previous results; `cand`
        excludes the points its final frame-to-frame search matched (mnLastFrameSeen)."""
        O = self.o_ext[b]                                                      # [ref, cur]
        ck, cd = O[1].extract(self.views[t][b])
        NL, tab, last = self.cfg[2], self.tab, self.o_last[b]
        mb = np.float32(self.bf) / np.float32(K[0])
        pc = [O[1].level(l) for l in range(NL)]
        pr = [O[0].level(l) for l in range(NL)]
        T_pred = prior_product(self.vel(t)[b], self.o_T[b])
        mono = not self.rgbd
        kw = dict(u_right=u_right, mbf=self.bf, mb=mb) if not mono else {}
        r = oracle.track_with_motion_model(pc, pr, tab, ck, cd, self.bounds, K, self.o_T[b], T_pred, last, th_mm, mono=mono, align_mode=0, **kw)
        seen = r["match"]
        if r["status"] != 0:                                                   # the final search again: its matches before the discard
            retried = bool(r["retried"])
            T_s = T_pred if retried or not r["align"]["ok"] else r["align"]["T"]
            kws = dict(u_right=u_right, mbf=self.bf, mb=mb) if not mono else {}
            _, seen = oracle.search_by_projection(ck, cd, tab["sf"], self.bounds, K, T_s, self.o_T[b], last, th=2 * th_mm if retried else th_mm,
                                                  mono=mono, check_ori=True, **kws)
            assert np.array_equal(np.where(r["match"] >= 0, seen, -1), r["match"])
        seen_ids = set(self.o_ids[b][seen[seen >= 0]].tolist()) - {-1}
        local = dict(self.local[b])
        local["cand"] = np.array([0 if i in seen_ids else 1 for i in self.lids[b]], np.uint8)
        rl = oracle.track_local_map(ck, cd, tab, np.log(np.float32(self.cfg[1])), self.bounds, K, r["T"], r["match"], last, local, th=th_lm,
                                    min_inliers=30, u_right=u_right, mbf=self.bf)
        un = np.where(rl["local_match"] >= 0, rl["local_match"] + M, rl["frame_match"])
        N = len(ck)
        h = host_handoff(ck, N, un, rl["outlier"], last, self.o_ids[b], self.local[b], self.lids[b])
        self.o_last[b], self.o_ids[b] = as_last(h, N)
        self.o_T[b] = rl["T"]
        O.reverse()                                                            # this frame is the next reference
        return r, rl, un, N


@pytest.mark.parametrize("name", ["p8", "p5"])
def test_closed_loop_matches_oracle(sd, oracle, name):
    """4 streams x 12 frames, monocular: TrackWithMotionModel + TrackLocalMap + hand-off per frame against the whole static
    map as local map (so the local map holds every last-frame point: the seen-point exclusion decides).  Per frame: the device
    hand-off equals the host restatement on the device's outputs, and every result equals the oracle's loop."""
    L = Loop(sd, oracle, CFGS[name], [11, 12, 13, 14], 12)
    trk, B = L.trk, L.B
    try:
        statuses, seen_branches = [], set()
        for t in range(1, L.T):
            L.device_step(t, 15.0, 1.0)
            tw, (fm, _), gl, gp, al = trk.get_tracked(0, B), trk.get_matches(0, B), trk.get_local_map(0, B), trk.get_pose_opt(0, B), trk.get_align(0, B)
            old = trk.get_last(0, B)
            ck, _, cn = trk.cur.download(0, B)
            trk.advance(B, 1)
            new = trk.get_last(0, B)
            for b in range(B):
                n = cn[b]
                key = (name, t, b)
                # hand-off exactness on the device's own outputs
                prev = {k: old[k][b] for k in ("valid", "Xw", "desc", "octave", "angle", "obs")}
                want = host_handoff(ck[b], n, gl["match"][b], gp["outlier"][b], prev, old["ids"][b], L.local[b], L.lids[b])
                check_last(new, b, want, n, key)
                # the oracle's loop
                r, rl, un, N = L.oracle_step(oracle, t, b, 15.0, 1.0)
                assert N == n, key
                assert (tw["status"][b], tw["nmatches"][b], tw["nmatches_map"][b]) == (r["status"], r["nmatches"], r["nmatches_map"]), key
                assert np.array_equal(fm[b, :n], r["match"]), key
                assert np.array_equal(gl["match"][b, :n], un), key
                assert (gl["status"][b], gl["n_inliers"][b], gl["n_local"][b]) == (rl["status"], rl["n_inliers"], rl["n_local"]), key
                assert np.array_equal(gp["outlier"][b, :n], rl["outlier"]), key
                assert np.abs(gp["T"][b] - rl["T"]).max() <= POSE_TOL, (key, np.abs(gp["T"][b] - rl["T"]).max())
                assert np.abs(al["T"][b] - gp["T"][b]).max() == 0, key          # the frame's pose (next Tref)
                assert np.abs(gp["T"][b][:3, 3] - L.seqs[b]["T"][t][:3, 3]).max() < 0.02, key
                statuses.append(int(gl["status"][b]))
                # every branch of the hand-off is taken: obs-0 points and outliers dropped, local-map points kept
                m, ol = gl["match"][b, :n], gp["outlier"][b, :n]
                seen_branches.add("local" if ((m >= M) & ~ol & (want["valid"][:n] == 1)).any() else "")
                seen_branches.add("outlier" if ((m >= 0) & ol).any() else "")
                obs_m = np.array([(L.local[b]["obs"][v - M] if v >= M else prev["obs"][v]) if v >= 0 else 1 for v in m])
                seen_branches.add("obs0" if ((m >= 0) & (obs_m < 1)).any() else "")
        assert all(s == 2 for s in statuses), statuses
        assert {"local", "outlier", "obs0"} <= seen_branches, seen_branches
    finally:
        L.close()


def test_closed_loop_rgbd(sd, oracle):
    """RGB-D: stereo_from_depth every frame, bMono = false, TrackLocalMap at th 3; 2 streams x 8 frames against the oracle."""
    L = Loop(sd, oracle, CFGS["p8"], [21, 22], 8, rgbd=True)
    trk, B = L.trk, L.B
    try:
        for t in range(1, L.T):
            L.device_step(t, 15.0, 3.0)
            tw, (fm, _), gl, gp = trk.get_tracked(0, B), trk.get_matches(0, B), trk.get_local_map(0, B), trk.get_pose_opt(0, B)
            ur, _ = trk.get_stereo(0, B)
            _, _, cn = trk.cur.download(0, B)
            trk.advance(B, 1)
            for b in range(B):
                key = (t, b)
                r, rl, un, n = L.oracle_step(oracle, t, b, 15.0, 3.0, u_right=ur[b, :cn[b]])
                assert (ur[b, :n] >= 0).sum() > 200, key
                assert (tw["status"][b], tw["nmatches"][b], tw["nmatches_map"][b]) == (r["status"], r["nmatches"], r["nmatches_map"]), key
                assert np.array_equal(fm[b, :n], r["match"]) and np.array_equal(gl["match"][b, :n], un), key
                assert (gl["status"][b], gl["n_inliers"][b]) == (rl["status"], rl["n_inliers"]), key
                assert np.abs(gp["T"][b] - rl["T"]).max() <= POSE_TOL, key
                assert gl["status"][b] == 2, key
    finally:
        L.close()


def test_handoff_after_motion_model_only(sd, oracle):
    """source 0: the hand-off straight after TrackWithMotionModel (post-discard cur_match, no outlier flags left) equals the
    host restatement on the device's outputs, frame after frame; obs-0 points of the last frame are dropped."""
    L = Loop(sd, oracle, CFGS["p8"], [31, 32, 33], 6)
    trk, B = L.trk, L.B
    try:
        dropped = 0
        for t in range(1, L.T):
            L.device_step(t, 15.0, 1.0, source=0)
            (fm, _), old, tw = trk.get_matches(0, B), trk.get_last(0, B), trk.get_tracked(0, B)
            ck, _, cn = trk.cur.download(0, B)
            with pytest.raises(sd.SdError) as e:              # TrackLocalMap did not run on this extraction
                trk.advance(B, 1)
            assert e.value.code == 1
            trk.advance(B, 0)
            new = trk.get_last(0, B)
            for b in range(B):
                prev = {k: old[k][b] for k in ("valid", "Xw", "desc", "octave", "angle", "obs")}
                want = host_handoff(ck[b], cn[b], fm[b], np.zeros(cn[b], bool), prev, old["ids"][b], None, None)
                check_last(new, b, want, cn[b], (t, b))
                m = fm[b, :cn[b]]
                dropped += int(((m >= 0) & (prev["obs"][np.maximum(m, 0)] < 1)).sum())
                assert tw["status"][b] == 2 and want["valid"].sum() >= 20
        assert dropped > 0
    finally:
        L.close()


def test_seen_point_exclusion_and_no_ids(sd, oracle):
    """The static map holds every point of the last frame.  With ids the device equals the oracle whose `cand` skips the
    points the frame-to-frame search saw; without ids (set_last resets the last-frame ids) it equals the oracle with every
    point a candidate -- today's behaviour."""
    L = Loop(sd, oracle, CFGS["p8"], [41, 42], 2)
    trk, B = L.trk, L.B
    try:
        log_sf = np.log(np.float32(L.cfg[1]))
        res = {}
        for ids in (True, False):
            if not ids:
                trk.set_last(0, L.o_last)                         # the same last frame, ids reset to -1
                assert (trk.get_last(0, B)["ids"] == -1).all()
            trk.set_poses(0, [s["T"][0] for s in L.seqs], [s["T"][0] for s in L.seqs])
            L.device_step(1, 15.0, 1.0)
            (fm, _), gl, tw, gp = trk.get_matches(0, B), trk.get_local_map(0, B), trk.get_tracked(0, B), trk.get_pose_opt(0, B)
            res[ids] = gl
            for b in range(B):
                ck, cd, cn = trk.cur.download(b, 1)
                n = cn[0]
                oc = L.o_ext[b][1]
                ok_, od = oc.extract(L.views[1][b])
                assert np.array_equal(ok_, ck[0, :n])
                pc = [oc.level(l) for l in range(L.cfg[2])]
                pr = [L.o_ext[b][0].level(l) for l in range(L.cfg[2])]
                T_pred = prior_product(L.vel(1)[b], L.seqs[b]["T"][0])
                r = oracle.track_with_motion_model(pc, pr, L.tab, ok_, od, BOUNDS, K, L.seqs[b]["T"][0], T_pred, L.o_last[b], 15.0, align_mode=0)
                assert np.array_equal(fm[b, :n], r["match"])
                local = dict(L.local[b])
                if ids:
                    T_s = T_pred if r["retried"] or not r["align"]["ok"] else r["align"]["T"]
                    _, seen = oracle.search_by_projection(ok_, od, L.tab["sf"], BOUNDS, K, T_s, L.seqs[b]["T"][0], L.o_last[b],
                                                          th=30.0 if r["retried"] else 15.0)
                    local["cand"] = np.isin(L.lids[b], L.o_ids[b][seen[seen >= 0]], invert=True).astype(np.uint8)
                    assert local["cand"].sum() < len(local["cand"]) - 100
                rl = oracle.track_local_map(ok_, od, L.tab, log_sf, BOUNDS, K, r["T"], r["match"], L.o_last[b], local, th=1.0)
                un = np.where(rl["local_match"] >= 0, rl["local_match"] + M, rl["frame_match"])
                assert np.array_equal(gl["match"][b, :n], un), (ids, b)
                assert (gl["status"][b], gl["n_inliers"][b], gl["n_local"][b]) == (rl["status"], rl["n_inliers"], rl["n_local"]), (ids, b)
                assert np.abs(gp["T"][b] - rl["T"]).max() <= POSE_TOL
        assert not np.array_equal(res[True]["match"], res[False]["match"])   # the exclusion changed the result
    finally:
        L.close()


def test_set_prior_bit_exact(sd):
    """set_prior relative: T @ Tref on the device equals the host product summed k = 0..3 in order, bit for bit; absolute
    mode stores T; Tref is left alone."""
    ext = [sd.ORBextractor(1000, 1.2, 8, 20, 640, 480, 8) for _ in range(2)]
    trk = sd.Tracker(ext[0], ext[1], max_points=M, max_batch=8)
    try:
        rng = np.random.Generator(np.random.PCG64(5))
        Tref = [synth.se3_exp(rng.normal(size=3), rng.normal(size=3) * 20) for _ in range(8)]
        V = [synth.se3_exp(rng.normal(size=3) * 0.01, rng.normal(size=3)) for _ in range(8)]
        V[3] = np.eye(4)
        trk.set_poses(0, Tref, [np.eye(4)] * 8)
        trk.set_prior(2, V[2:7], relative=True)
        got = trk.get_align(0, 8)["T"]
        for i in range(8):
            want = prior_product(V[i], Tref[i]) if 2 <= i < 7 else np.eye(4)
            assert np.array_equal(got[i], want), i
        trk.set_prior(0, V[:2], relative=False)
        got = trk.get_align(0, 2)["T"]
        assert np.array_equal(got[0], V[0]) and np.array_equal(got[1], V[1])
        trk.set_prior(0, [np.eye(4)] * 8, relative=True)          # Tref untouched by both calls
        got = trk.get_align(0, 8)["T"]
        for i in range(8):
            assert np.array_equal(got[i], prior_product(np.eye(4), Tref[i])), i
    finally:
        trk.close()
        for e in ext:
            e.close()


def test_advance_errors(sd):
    """SD_ERR_CAPACITY when the keypoint capacity exceeds max_points; SD_ERR_INVALID_ARG before the named call ran since the
    last extraction, for a bad source, and in broadcast mode."""
    ext = [sd.ORBextractor(1000, 1.2, 8, 20, 640, 480, 2) for _ in range(2)]
    small = sd.Tracker(ext[0], ext[1], max_points=500, max_batch=2)
    try:
        with pytest.raises(sd.SdError) as e:
            small.advance(2, 0)
        assert e.value.code == 3
    finally:
        small.close()
    seq = synth.make_sequence(3, 2)
    trk = sd.Tracker(ext[0], ext[1], max_points=M, max_batch=2)
    try:
        trk.set_camera(*K, 0.0, BOUNDS)
        trk.ref.extract_batch(np.stack([seq["views"][0]] * 2))
        trk.cur.extract_batch(np.stack([seq["views"][1]] * 2))
        for src in (0, 1, 2):
            with pytest.raises(sd.SdError) as e:
                trk.advance(2, src)
            assert e.value.code == 1
        trk.set_poses(0, [seq["T"][0]] * 2, [seq["T"][1]] * 2)
        trk.track_with_motion_model(2, th=15.0)
        trk.set_current_broadcast(0)
        with pytest.raises(sd.SdError) as e:
            trk.advance(2, 0)
        assert e.value.code == 1
        trk.set_current_broadcast(-1)
        trk.cur.extract_batch(np.stack([seq["views"][1]] * 2))       # re-extracted: the result is gone
        with pytest.raises(sd.SdError) as e:
            trk.advance(2, 0)
        assert e.value.code == 1
        trk.track_with_motion_model(2, th=15.0)
        c0 = trk.cur
        trk.advance(2, 0)
        assert trk.ref is c0 and trk.cur is not c0
        with pytest.raises(sd.SdError) as e:                          # once per extraction
            trk.advance(2, 0)
        assert e.value.code == 1
    finally:
        trk.close()
        for e_ in ext:
            e_.close()


def _run_loop(L, frame_ptr, rec_ptr, sync):
    """The T-frame loop on device-resident frames: extraction into the current `cur`, prior, TrackWithMotionModel,
    TrackLocalMap, records packed on the device, hand-off.  sync: a host getter after every frame."""
    trk, B = L.trk, L.B
    for t in range(1, L.T):
        trk.cur.extract_batch_device(frame_ptr(t), B, 640, 480)
        trk.set_prior(0, L.vel(t), relative=True)
        trk.track_with_motion_model(B, th=15.0, mono=True, align_mode=0)
        trk.track_local_map(B, th=1.0, min_inliers=30)
        trk.pack_records(B, 3, rec_ptr(t))
        trk.advance(B, 1)
        if sync:
            trk.get_local_map(0, B)
    return trk.get_last(0, B)


def _download(ptr, nbytes):
    import ctypes as C
    from sdslam_amd import capi
    out = np.zeros(nbytes, np.uint8)
    capi._check(capi.lib().sd_dev_download(out.ctypes.data_as(C.c_void_p), ptr, nbytes))
    return out


def test_queued_loop_equals_synchronised_loop(sd, oracle):
    """The whole loop queued without a host synchronisation between frames gives the records and the final last frame of
    the loop that synchronises after every frame."""
    out = []
    for sync in (True, False):
        L = Loop(sd, oracle, CFGS["p8"], [61, 62, 63, 64], 8)
        try:
            B, F = L.B, 640 * 480
            frames = sd.DeviceBuffer(L.T * B * F)
            frames.upload(L.views)
            rec = sd.DeviceBuffer(L.T * B * 20 * 8)
            last = _run_loop(L, lambda t: frames.ptr.value + t * B * F, lambda t: ctypes.c_void_p(rec.ptr.value + t * B * 160).value, sync)
            out.append((_download(rec.ptr, L.T * B * 160)[B * 160:], last))
            frames.free()
            rec.free()
        finally:
            L.close()
    assert np.array_equal(out[0][0], out[1][0])
    for k in out[0][1]:
        assert np.array_equal(out[0][1][k], out[1][1][k]), k
    recs = out[0][0].view(np.float64).reshape(-1, 20)
    assert (recs[:, 19] == 1).all()                                # every frame of every stream tracked


def _in_child(request):
    if _CHILD:
        return True
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [
        "-m", "pytest", f"{request.node.path}::{request.node.name}", "-m", "gpu", "-q", "-p", "no:cacheprovider"]
    env = dict(os.environ, SD_SEQUENCE_CHILD="1", GPU_MAX_HW_QUEUES="16")
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and " passed" in r.stdout, r.stdout[-6000:] + r.stderr[-2000:]
    return False


def test_extraction_into_swapped_extractor_waits_for_held_tracking(sd, oracle, request):
    """Frames 3..6 are queued while a GPU delay on a caller's stream holds the tracking stream back (sd_track_stream_fence
    direction 1): the extractions into the swapped extractors must wait for the held tracking kernels that still read the
    output sets they overwrite.  The delay is still pending when the loop is queued; records and final last frame equal a
    synchronised run.  Runs in a child process with torch loaded first (one HIP runtime, 16 hardware queues), as
    test_stream_order_gpu does."""
    if not _in_child(request):
        return
    import torch
    hip = ctypes.CDLL("libamdhip64.so.7")
    p = ctypes.c_void_p()
    assert hip.hipStreamCreateWithFlags(ctypes.byref(p), ctypes.c_uint(1)) == 0
    S = torch.cuda.ExternalStream(p.value)
    out = []
    for held in (False, True):
        L = Loop(sd, oracle, CFGS["p8"], [71, 72, 73, 74], 8)
        try:
            B = L.B
            frames = torch.from_numpy(np.ascontiguousarray(L.views)).cuda()
            rec = torch.full((L.T, B, 20), -7.0, dtype=torch.float64, device="cuda")
            torch.cuda.synchronize()
            ev = torch.cuda.Event()

            def hold():
                with torch.cuda.stream(S):
                    torch.cuda._sleep(SLEEP)
                    ev.record(S)
                L.trk.stream_fence(S.cuda_stream, 1)
            if not held:
                last = _run_loop(L, lambda t: frames[t].data_ptr(), lambda t: rec[t].data_ptr(), sync=True)
            else:
                trk = L.trk
                for t in range(1, L.T):
                    if t == 3:
                        hold()
                    trk.cur.extract_batch_device(frames[t].data_ptr(), B, 640, 480)
                    trk.set_prior(0, L.vel(t), relative=True)
                    trk.track_with_motion_model(B, th=15.0, mono=True, align_mode=0)
                    trk.track_local_map(B, th=1.0, min_inliers=30)
                    trk.pack_records(B, 3, rec[t].data_ptr())
                    trk.advance(B, 1)
                    if t < 3:
                        trk.get_local_map(0, B)
                    if t == 6:
                        assert not ev.query(), "the delay ended before the held frames were queued: the run proves nothing"
                last = trk.get_last(0, B)
            torch.cuda.synchronize()
            out.append((rec[1:].cpu().numpy(), last))
        finally:
            L.close()
    assert np.array_equal(out[0][0], out[1][0])
    for k in out[0][1]:
        assert np.array_equal(out[0][1][k], out[1][1][k]), k
