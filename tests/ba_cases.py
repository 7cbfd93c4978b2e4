"""The LocalBundleAdjustment cases of tests/test_local_ba_cpu.py and tests/test_local_ba_gpu.py: problems in the form tests/ba_ref.py
takes (and sd_debug_local_ba with it).  Small scenes: cameras on a line looking down +z, points 3 .. 7 m in front of them, the
synthetic pinhole camera (depths of a few metres, so a pose error of 1e-5 is a few 1e-3 px)."""
import numpy as np

CAM = (458.654, 457.296, 367.215, 248.375)
BF = 47.9
INV_SIGMA2 = (1.0 / 1.2 ** (2 * np.arange(8))).astype(np.float32)


def _rot(w):
    th = np.linalg.norm(w)
    if th < 1e-12:
        return np.eye(3)
    k = w / th
    Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def scene(seed, roles, n_points, obs_per_point, stereo_share=0.0, pix_noise=0.0, pose_noise=0.0, point_noise=0.0, wrong_share=0.0,
          wrong_px=(25.0, 60.0)):
    """roles [n_kf]; every point is seen by obs_per_point cameras (int, or a callable rng -> count) chosen at random"""
    rng = np.random.default_rng(seed)
    roles = np.asarray(roles, np.uint8)
    n_kf = len(roles)
    T_true = np.zeros((n_kf, 4, 4))
    for c in range(n_kf):
        R = _rot(rng.normal(0, 0.05, 3))
        centre = np.array([0.35 * c - 0.175 * (n_kf - 1), rng.normal(0, 0.05), rng.normal(0, 0.05)])
        T_true[c] = np.eye(4)
        T_true[c, :3, :3] = R
        T_true[c, :3, 3] = -R @ centre
    X_true = np.stack([rng.uniform(-2.0, 2.0, n_points), rng.uniform(-1.2, 1.2, n_points), rng.uniform(3.0, 7.0, n_points)], 1)
    fx, fy, cx, cy = CAM
    off, kf, uv, ur, inv = [0], [], [], [], []
    for i in range(n_points):
        k = obs_per_point(rng) if callable(obs_per_point) else obs_per_point
        for c in sorted(rng.choice(n_kf, size=min(k, n_kf), replace=False)):
            pc = T_true[c, :3, :3] @ X_true[i] + T_true[c, :3, 3]
            u, v = fx * pc[0] / pc[2] + cx, fy * pc[1] / pc[2] + cy
            octave = int(rng.integers(0, 4))
            sig = pix_noise * 1.2 ** octave
            du, dv, dr = rng.normal(0, 1, 3) * sig
            if rng.uniform() < wrong_share:
                a, m = rng.uniform(0, 2 * np.pi), rng.uniform(*wrong_px)
                du, dv = du + m * np.cos(a), dv + m * np.sin(a)
            kf.append(c)
            uv.append((u + du, v + dv))
            ur.append(u - BF / pc[2] + dr if rng.uniform() < stereo_share else -1.0)
            inv.append(INV_SIGMA2[octave])
        off.append(len(kf))
    poses = T_true.copy()
    for c in np.flatnonzero(roles == 1):
        d = np.eye(4)
        d[:3, :3] = _rot(rng.normal(0, pose_noise, 3))
        d[:3, 3] = rng.normal(0, pose_noise, 3)
        poses[c] = d @ T_true[c]
    Xw = X_true + rng.normal(0, point_noise, X_true.shape)
    return dict(off=np.array(off, np.int32), kf=np.array(kf, np.int32), uv=np.array(uv, np.float32).reshape(-1, 2),
                ur=np.array(ur, np.float32), inv_sigma2=np.array(inv, np.float32), kf_bad=np.zeros(len(kf), np.uint8),
                point_bad=np.zeros(n_points, np.uint8), poses=poses, roles=roles, Xw=Xw, cam=CAM, bf=BF, T_true=T_true, X_true=X_true)


def _edges_of(p, i):
    return range(int(p["off"][i]), int(p["off"][i + 1]))


def noisy(seed=3, cur_fixed=False):
    """6 local keyframes (one with role 2) + 3 fixed, 150 points, mono and stereo mixed, noisy start, ~10 % planted wrong observations.
    cur_fixed: the LAST camera (the one the resident tests plant as the current keyframe) is the one with role 2."""
    roles = [1, 2, 1, 1, 1, 1, 0, 0, 0] if not cur_fixed else [1, 1, 1, 1, 1, 0, 0, 0, 2]
    return scene(seed, roles, 150, lambda r: int(r.integers(3, 7)), stereo_share=0.4, pix_noise=0.5, pose_noise=0.004, point_noise=0.02,
                 wrong_share=0.10)


def exact():
    """3 local + 2 fixed keyframes, 40 mono points, exact start.  Every quantity is chosen so that the projection is exact in
    double AND in float (identity rotations, translations and points on a 1/64 grid, depths 2, 4 or 8, focal length 512): every
    error is exactly 0, so chi2 = 0, b = 0, x = 0, rho = 0 / 1e-3 == 0 and optimize() returns on its first trial, in both rounds."""
    rng = np.random.default_rng(1)
    n_kf, P = 5, 40
    poses = np.stack([np.eye(4)] * n_kf)
    poses[:, 0, 3] = -(np.arange(n_kf) - 2) * 0.25
    X = np.stack([rng.integers(-64, 65, P) / 64.0, rng.integers(-48, 49, P) / 64.0, rng.choice([2.0, 4.0, 8.0], P)], 1)
    off, kf, uv = [0], [], []
    for i in range(P):
        for c in sorted(rng.choice(n_kf, size=4, replace=False)):
            pc = X[i] + poses[c, :3, 3]
            kf.append(c)
            uv.append((512.0 * pc[0] / pc[2] + 320.0, 512.0 * pc[1] / pc[2] + 240.0))
        off.append(len(kf))
    uv = np.array(uv)
    assert (uv.astype(np.float32) == uv).all()
    E = len(kf)
    return dict(off=np.array(off, np.int32), kf=np.array(kf, np.int32), uv=uv.astype(np.float32), ur=-np.ones(E, np.float32),
                inv_sigma2=np.ones(E, np.float32), kf_bad=np.zeros(E, np.uint8), point_bad=np.zeros(P, np.uint8), poses=poses,
                roles=np.array([1, 1, 1, 0, 0], np.uint8), Xw=X.copy(), cam=(512.0, 512.0, 320.0, 240.0), bf=BF, T_true=poses.copy(),
                X_true=X.copy())


def special_points():
    """On the noisy scene: point 0 with one observation, point 1 with 70 observations (a second wave pass; 70 cameras would not
    fit, so the scene has 72 fixed cameras), point 2 with two contradicting observations (every edge at level 1 after round 1), point 3
    behind one of its cameras, local keyframe 5 without observations, some obs_kf_bad and point_bad entries."""
    roles = [1, 2, 1, 1, 1, 1] + [0] * 72
    rng = np.random.default_rng(11)
    p = scene(5, roles, 120, lambda r: int(r.integers(3, 6)), stereo_share=0.4, pix_noise=0.5, pose_noise=0.003, point_noise=0.02)
    fx, fy, cx, cy = CAM
    lists = [[(int(p["kf"][e]), p["uv"][e].copy(), float(p["ur"][e]), float(p["inv_sigma2"][e])) for e in _edges_of(p, i)] for i in range(120)]

    def project(c, X, noise=0.3):
        pc = p["T_true"][c, :3, :3] @ X + p["T_true"][c, :3, 3]
        return np.array([fx * pc[0] / pc[2] + cx, fy * pc[1] / pc[2] + cy]) + rng.normal(0, noise, 2), pc[2]

    lists = [[o for o in l if o[0] != 5] for l in lists]                  # keyframe 5 sees nothing
    lists[0] = lists[0][:1] if lists[0] else [(0, project(0, p["X_true"][0])[0], -1.0, 1.0)]
    lists[1] = [(c, project(c, p["X_true"][1])[0], -1.0, 1.0) for c in [0, 2] + list(range(6, 74))]      # 70 observations
    # two observations that contradict each other across the epipolar lines (the cameras lie along x): no position explains either
    lists[2] = [(c, project(c, p["X_true"][2])[0] + np.array([0.0, dy]), -1.0, 1.0) for c, dy in ((0, 60.0), (2, -60.0))]
    # point 3: between camera 4 and the others' view: behind camera 4 (its measurement is anything)
    c4 = -p["T_true"][4, :3, :3].T @ p["T_true"][4, :3, 3]
    p["X_true"][3] = c4 + p["T_true"][4, :3, :3].T @ np.array([0.05, 0.02, -0.4])
    p["Xw"][3] = p["X_true"][3] + rng.normal(0, 0.005, 3)
    lists[3] = [(c, project(c, p["X_true"][3])[0], -1.0, 1.0) for c in [0, 2, 3]] + [(4, np.array([300.0, 200.0]), -1.0, 1.0)]
    kf_bad, point_bad = [], np.zeros(120, np.uint8)
    point_bad[[7, 19]] = 1
    off, kf, uv, ur, inv = [0], [], [], [], []
    for i, l in enumerate(lists):
        for j, o in enumerate(l):
            kf.append(o[0]); uv.append(o[1]); ur.append(o[2]); inv.append(o[3])
            kf_bad.append(1 if (i in (9, 10, 30) and j == 1) else 0)
        off.append(len(kf))
    p.update(off=np.array(off, np.int32), kf=np.array(kf, np.int32), uv=np.array(uv, np.float32).reshape(-1, 2), ur=np.array(ur, np.float32),
             inv_sigma2=np.array(inv, np.float32), kf_bad=np.array(kf_bad, np.uint8), point_bad=point_bad)
    return p


def many_points():
    """300 points on 4 keyframes: more points than one workgroup's tile"""
    return scene(7, [1, 1, 1, 2], 300, 3, stereo_share=0.3, pix_noise=0.4, pose_noise=0.003, point_noise=0.02, wrong_share=0.05)


def max_free(extra=0):
    """SD_BA_MAX_FREE_KF free keyframes exactly (8 points each are enough), +extra; two fixed cameras hold the gauge"""
    n = 32 + extra
    return scene(9, [1] * n + [2, 0], 8 * n, 3, stereo_share=0.5, pix_noise=0.3, pose_noise=0.002, point_noise=0.01)


def not_resident():
    p = noisy()
    p["kf"][int(p["off"][40])] = -2
    return p


def bad_index():
    p = noisy()
    p["kf"][int(p["off"][41]) + 1] = -3
    return p


def cases():
    """name -> problem; the certified ones (a full run whose decisions must not depend on the summation order) come first"""
    return dict(exact=exact(), noisy=noisy(), noisy_cur_fixed=noisy(cur_fixed=True), special=special_points(), many_points=many_points(),
                max_free=max_free(), too_many=max_free(1), not_resident=not_resident(), bad_index=bad_index())


RUN_CASES = ("exact", "noisy", "noisy_cur_fixed", "special", "many_points", "max_free")
REFUSED = dict(too_many=2, not_resident=1, bad_index=3)


def permuted(p, seed):
    """The same problem with its points, each point's observations and its cameras in another order, and the maps back:
    (problem, point_perm, edge_perm, cam_perm) with new point i = old point_perm[i] etc.  seed 0: the identity."""
    rng = np.random.default_rng(1000 + seed)
    P, n_kf = len(p["off"]) - 1, len(p["roles"])
    pp = np.arange(P) if seed == 0 else rng.permutation(P)
    cp = np.arange(n_kf) if seed == 0 else rng.permutation(n_kf)
    inv_cp = np.argsort(cp)
    ep, off = [], [0]
    for i in pp:
        e = np.arange(p["off"][i], p["off"][i + 1])
        ep += list(e if seed == 0 else rng.permutation(e))
        off.append(len(ep))
    ep = np.array(ep, np.int64)
    q = dict(p)
    kf_old = p["kf"][ep]
    q.update(off=np.array(off, np.int32), kf=np.where((kf_old >= 0) & (kf_old < n_kf), inv_cp[np.clip(kf_old, 0, n_kf - 1)], kf_old).astype(np.int32),
             uv=p["uv"][ep], ur=p["ur"][ep], inv_sigma2=p["inv_sigma2"][ep], kf_bad=p["kf_bad"][ep], point_bad=p["point_bad"][pp],
             poses=p["poses"][cp], roles=p["roles"][cp], Xw=p["Xw"][pp])
    return q, pp, ep, cp


# The largest deviation of poses and points that tests/test_local_ba_cpu.py::test_noise_floor measures between 9 edge and vertex
# orders of every run case and between the Schur and the dense solver, rounded up.  The GPU tests allow 64 times that (the margin
# the IMU tests give over their floor), and never more than the project's pose criterion of 1e-5.
NOISE_FLOOR = 1.3e-7      # measured 1.3e-7: the stereo projection's `const float invz` makes the errors step by 3e-5 px
GPU_BOUND = min(64 * NOISE_FLOOR, 1e-5)
