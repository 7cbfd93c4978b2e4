"""The RGB-D odometry loop the keyframe-point tests share (helper, no tests): B streams start from StereoInitialization on
frame 0 of a synthetic sequence and then run, per frame, TrackWithMotionModel -> TrackLocalMap with an EMPTY local map ->
NeedNewKeyFrame -> CreateNewKeyFrame -> the hand-off, with nothing but the points they created themselves.
`oracle_loop` is that loop on the CPU oracle + the numpy restatement (tests/keyframe_points_ref.py); the GPU test runs the
same loop on the device and compares frame by frame.

Parameters (chosen so that the oracle loop alone stays tracked and inserts keyframes, checked in
tests/test_keyframe_points_cpu.py): th_depth 2.0 lies inside the surface's 1.6-2.4 m; every 9th depth column and a band of rows
are zero (invalid depth); the keyframe state is constant -- nKFs 5, nRefMatches 700 (c2 holds once fewer than 525 inliers
are tracked, c1c never: 175), mapper idle -- with MinFrames 3, MaxFrames 30: c1b lets a keyframe through at most every third
frame, and the gate moves with mnLastKeyFrameId, which the creation step writes."""
import numpy as np

import keyframe_points_ref as R
from sdslam_amd import synth

K = (synth.FX, synth.FY, synth.CX, synth.CY)
BOUNDS = (0.0, 640.0, 0.0, 480.0)
CFG = (1000, 1.2, 8, 20)
M = 1000
BF = 4.0
TH_DEPTH = np.float32(2.0)
TH_MM, TH_LM = 15.0, 3.0
MIN_FRAMES, MAX_FRAMES = 3, 30
STATE = (5, 700, 0, 0, 1, 0, 0, 0)
SEEDS = (151, 152)
T_FRAMES = 12
EMPTY_LOCAL = dict(cand=np.zeros(0, np.uint8), Xw=np.zeros((0, 3)), normal=np.zeros((0, 3)), min_dist=np.zeros(0, np.float32),
                   max_dist=np.zeros(0, np.float32), mf_max_dist=np.zeros(0, np.float32), desc=np.zeros((0, 32), np.uint8),
                   obs=np.zeros(0, np.int32))


def sequences(seeds=SEEDS, T=T_FRAMES):
    seqs = [synth.make_sequence(s, T, with_depth=True) for s in seeds]
    depth = np.stack([s["depth"] for s in seqs], 1).astype(np.float32)        # [T][B][H][W]
    depth[..., ::9] = 0.0
    depth[:, :, 200:215, :] = 0.0
    views = np.stack([s["views"] for s in seqs], 1)
    return seqs, views, depth


def velocity(seqs, t):
    """The motion model stays an input: the true relative motion of frame t (frame 0 is the identity)."""
    return [s["T"][t] @ np.linalg.inv(s["T"][t - 1]) for s in seqs]


def prior_product(V, L):
    P = V[:, 0:1] * L[0:1, :]
    for k in range(1, 4):
        P = P + V[:, k:k + 1] * L[k:k + 1, :]
    return P


def as_last(h, N):
    return {k: np.ascontiguousarray(h[k][:N]) for k in ("valid", "Xw", "desc", "octave", "angle", "obs")}, h["ids"][:N].copy()


def oracle_loop(oracle, seqs, views, depth, next_id0):
    """Returns per stream a list over frames 0..T-1 of dict(status_mm, nmatches, nmatches_map, match, status, n_inliers,
    outlier, T, close, flag, created, P, candidates, ids, Xw, last)."""
    T, B = views.shape[0], views.shape[1]
    out = []
    for b in range(B):
        ext = [oracle.OrbOracle(*CFG), oracle.OrbOracle(*CFG)]                # [ref, cur]
        tab = ext[0].tables()
        log_sf = np.log(np.float32(CFG[1]))
        mb = np.float32(BF) / np.float32(K[0])
        next_id, last_kf = int(next_id0[b]), 0
        ck, cd = ext[0].extract(views[0][b])
        ur, dd = oracle.stereo_from_rgbd(ck, ck, depth[0][b], BF)
        idx = R.stereo_initialization(dd, 500)
        assert idx is not None
        Xw = np.array([R.unproject_stereo(ck["x"][i], ck["y"][i], dd[i], K, np.eye(4)) for i in idx])
        ids = np.arange(next_id, next_id + len(idx), dtype=np.int32)
        next_id += len(idx)
        h = R.handoff(M, ck, len(ck), None, None, None, None, None, None, dict(kp_index=idx, Xw=Xw, ids=ids), cd)
        last, last_ids = as_last(h, len(ck))
        T_last = np.eye(4)
        rec = [dict(created=idx, ids=ids, Xw=Xw, T=np.eye(4), last=h)]
        for t in range(1, T):
            ck, cd = ext[1].extract(views[t][b])
            N = len(ck)
            ur, dd = oracle.stereo_from_rgbd(ck, ck, depth[t][b], BF)
            T_pred = prior_product(velocity(seqs, t)[b], T_last)
            pc = [ext[1].level(l) for l in range(CFG[2])]
            pr = [ext[0].level(l) for l in range(CFG[2])]
            r = oracle.track_with_motion_model(pc, pr, tab, ck, cd, BOUNDS, K, T_last, T_pred, last, TH_MM, mono=False, align_mode=0,
                                               u_right=ur, mbf=BF, mb=mb)
            rl = oracle.track_local_map(ck, cd, tab, log_sf, BOUNDS, K, r["T"], r["match"], last, EMPTY_LOCAL, th=TH_LM, min_inliers=30,
                                        u_right=ur, mbf=BF)
            m, ol = rl["frame_match"], rl["outlier"]
            tracked = rl["status"] == 2
            obs_m = np.where(m >= 0, last["obs"][np.maximum(m, 0)], 0)
            kept = (m >= 0) & (obs_m >= 1) & ~ol
            close = (dd > 0) & (dd < TH_DEPTH)
            counts = (int((close & kept).sum()), int((close & ~kept).sum()))
            flag = R.need_new_keyframe(tracked, rl["n_inliers"], counts[0], counts[1], STATE[:2] + (last_kf,) + STATE[3:], 1, t,
                                       MIN_FRAMES, MAX_FRAMES)
            created, P, cand, cXw, cids = [], 0, 0, np.zeros((0, 3)), np.zeros(0, np.int32)
            if tracked and flag & 1:
                created, P, cand = R.create_new_keyframe(dd, TH_DEPTH, m, M, last["obs"], np.zeros(M, np.int32))
                cXw = np.array([R.unproject_stereo(ck["x"][i], ck["y"][i], dd[i], K, rl["T"]) for i in created]).reshape(-1, 3)
                cids = np.arange(next_id, next_id + len(created), dtype=np.int32)
                next_id += len(created)
                last_kf = t
            h = R.handoff(M, ck, N, m, ol, last, last_ids, None, None, dict(kp_index=created, Xw=cXw, ids=cids), cd)
            rec.append(dict(status_mm=r["status"], nmatches=r["nmatches"], nmatches_map=r["nmatches_map"], match_mm=r["match"], match=m,
                            status=rl["status"], n_inliers=rl["n_inliers"], outlier=ol, T=rl["T"], close=counts, flag=flag,
                            created=created, P=P, candidates=cand, ids=cids, Xw=cXw, last=h, depth=dd,
                            n_close=int(((dd > 0) & (dd <= TH_DEPTH)).sum()), obs_m=obs_m))
            last, last_ids = as_last(h, N)
            T_last = rl["T"]
            ext.reverse()
        out.append(rec)
    return out
