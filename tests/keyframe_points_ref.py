"""Numpy restatement of the RGB-D map point creation the device performs (helper, no tests): Tracking::CreateNewKeyFrame
(src/Tracking.cc:840-887) as the literal serial loop, Tracking::StereoInitialization (:303-327), Frame::UnprojectStereo
(src/Frame.cc:419-431) in the project's operation order, Tracking::NeedNewKeyFrame (:753-826) and the hand-off
(:250-292) extended by the created points.  Written for this project; nothing here calls the library."""
import numpy as np

F32 = np.float32


def unproject_stereo(u, v, z, K, T):
    """x = (u - cx) * z * invfx, y likewise, in float, left to right, invfx = 1.0f / fx; Xw = Rwc * (x, y, z) + Ow in
    double with Rwc = Rcw^T, Ow = -Rwc * tcw, every row summed left to right, every operation rounded on its own."""
    fx, fy, cx, cy = (F32(k) for k in K)
    invfx, invfy = F32(1.0) / fx, F32(1.0) / fy
    u, v, z = F32(u), F32(v), F32(z)
    x = (u - cx) * z * invfx
    y = (v - cy) * z * invfy
    assert x.dtype == np.float32 and y.dtype == np.float32
    x, y, z = np.float64(x), np.float64(y), np.float64(z)
    T = np.asarray(T, np.float64)
    Rwc, t = T[:3, :3].T, T[:3, 3]
    out = np.zeros(3)
    for r in range(3):
        Ow = -((Rwc[r, 0] * t[0] + Rwc[r, 1] * t[1]) + Rwc[r, 2] * t[2])
        out[r] = ((Rwc[r, 0] * x + Rwc[r, 1] * y) + Rwc[r, 2] * z) + Ow
    return out


def point_obs(m, M, last_obs, local_obs):
    """Observations() of mvpMapPoints[i] = m (m < M: last-frame point, m >= M: local point m - M)."""
    return int(local_obs[m - M]) if m >= M else int(last_obs[m])


def create_new_keyframe(depth, th_depth, match, M, last_obs, local_obs):
    """The RGB-D loop of CreateNewKeyFrame on mvDepth[:N] and mvpMapPoints = match (before the outlier discard of
    :272-275: mvbOutlier is not consulted).  Returns (created keypoint indices in creation order, P = list entries the loop
    visited, number of candidates)."""
    vDepthIdx = []
    for i in range(len(depth)):
        z = depth[i]
        if z > 0:
            vDepthIdx.append((float(z), i))
    created, visited = [], 0
    if vDepthIdx:
        vDepthIdx.sort()
        nPoints = 0
        for j in range(len(vDepthIdx)):
            i = vDepthIdx[j][1]
            bCreateNew = False
            m = int(match[i])
            if m < 0:
                bCreateNew = True
            elif point_obs(m, M, last_obs, local_obs) < 1:
                bCreateNew = True
            if bCreateNew:
                created.append(i)
                nPoints += 1
            else:
                nPoints += 1
            visited = j + 1
            if vDepthIdx[j][0] > th_depth and nPoints > 100:
                break
    return created, visited, len(vDepthIdx)


def prefix_closed_form(depth, th_depth):
    """P as the kernel finds it: the first sorted j with z_j > th_depth and j + 1 > 100, plus one; else the candidates."""
    z = np.sort(np.asarray(depth, np.float32)[np.asarray(depth, np.float32) > 0], kind="stable")
    hit = np.nonzero((z > F32(th_depth)) & (np.arange(len(z)) >= 100))[0]
    return int(hit[0]) + 1 if len(hit) else len(z)


def stereo_initialization(depth, min_keypoints=500):
    """Keypoints that get a point, in creation (= index) order; None when N <= min_keypoints."""
    if not len(depth) > min_keypoints:
        return None
    return [i for i in range(len(depth)) if depth[i] > 0]


def need_new_keyframe(tracked, inliers, n_tracked_close, n_non_tracked_close, state, rgbd, frame_id, min_frames, max_frames):
    """state = (nKFs, nRefMatches, last_kf_id, last_reloc_id, flags): flags bit 0 mapper idle, 1 stopped, 2 queue < 3.
    Returns the flag byte: bit 0 insert, bit 1 wanted but the mapper is busy (InterruptBA)."""
    nKFs, nRefMatches, last_kf, last_reloc, fl = (int(v) for v in state[:5])
    if not tracked:
        return 0
    if fl & 2:
        return 0
    if frame_id < last_reloc + max_frames and nKFs > max_frames:
        return 0
    idle = bool(fl & 1)
    if not rgbd:
        n_tracked_close = n_non_tracked_close = 0
    need_close = n_tracked_close < 100 and n_non_tracked_close > 70
    th = F32(0.75)
    if nKFs < 2:
        th = F32(0.4)
    if not rgbd:
        th = F32(0.9)
    c1a = frame_id >= last_kf + max_frames
    c1b = frame_id >= last_kf + min_frames and idle
    c1c = bool(rgbd) and (float(inliers) < float(nRefMatches) * 0.25 or need_close)          # double
    c2 = (bool(F32(inliers) < F32(nRefMatches) * th) or need_close) and inliers > 15          # float
    if (c1a or c1b or c1c) and c2:
        if idle:
            return 1
        return 2 | (1 if rgbd and fl & 4 else 0)
    return 0


def handoff(M, kps, N, match, outlier, last, last_ids, local, local_ids, created=None, cur_desc=None):
    """src/Tracking.cc:250-292 (host_handoff of test_sequence_gpu.py) extended: a keypoint in created = dict(kp_index, Xw,
    ids) carries its new point -- Xw, the keypoint's descriptor, Observations() 1, the id -- whatever outlier[i] says.
    match None: after StereoInitialization, the created points only."""
    out = dict(valid=np.zeros(M, np.uint8), Xw=np.zeros((M, 3)), desc=np.zeros((M, 32), np.uint8), octave=np.zeros(M, np.int32),
               angle=np.zeros(M, np.float32), obs=np.zeros(M, np.int32), ids=np.full(M, -1, np.int32))
    out["octave"][:N] = kps["octave"][:N]
    out["angle"][:N] = kps["angle"][:N]
    new = {}
    if created is not None:
        new = {int(i): r for r, i in enumerate(created["kp_index"])}
    for i in range(N):
        if i in new:
            r = new[i]
            out["valid"][i], out["Xw"][i], out["desc"][i] = 1, created["Xw"][r], cur_desc[i]
            out["obs"][i], out["ids"][i] = 1, created["ids"][r]
            continue
        if match is None:
            continue
        m = int(match[i])
        if m < 0 or outlier[i]:
            continue
        src, ids, j = (local, local_ids, m - M) if m >= M else (last, last_ids, m)
        if src["obs"][j] < 1:
            continue
        out["valid"][i], out["Xw"][i], out["desc"][i] = 1, src["Xw"][j], src["desc"][j]
        out["obs"][i], out["ids"][i] = src["obs"][j], ids[j]
    return out
