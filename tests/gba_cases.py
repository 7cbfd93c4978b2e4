"""The BundleAdjustment cases of tests/test_global_ba_cpu.py and tests/test_global_ba_gpu.py: problems in the form tests/gba_ref.py takes
(and sd_debug_global_ba with it), built on ba_cases.scene.  Roles: 1 free, 2 fixed (mnId == 0), 0 no vertex."""
import numpy as np

import ba_cases
from ba_cases import CAM, BF, INV_SIGMA2, scene, permuted


def exact():
    """ba_cases.exact with its two fixed cameras as fixed vertices: every error is exactly 0, rho = 0 / 1e-3 == 0 on the first trial"""
    p = ba_cases.exact()
    p["roles"] = np.array([1, 1, 1, 2, 2], np.uint8)
    return p


def mono_init():
    """CreateInitialMapMonocular: two keyframes, the first fixed, 150 monocular points seen by both"""
    return scene(21, [2, 1], 150, 2, pix_noise=0.4, pose_noise=0.004, point_noise=0.03)


def noisy():
    """8 free keyframes and a fixed one, 150 points, mono and stereo mixed, ~10 % planted wrong observations"""
    return scene(3, [1] * 8 + [2], 150, lambda r: int(r.integers(3, 7)), stereo_share=0.4, pix_noise=0.5, pose_noise=0.004, point_noise=0.02,
                 wrong_share=0.10)


def stereo_mix():
    return scene(4, [2, 1, 1, 1, 1], 100, 3, stereo_share=0.6, pix_noise=0.4, pose_noise=0.003, point_noise=0.02)


def special_points():
    """On a small noisy scene: point 0 bad, point 1 without an observation, point 2 whose only observation is of a bad keyframe (role 0,
    so only the flag keeps the edge out), point 3 with one observation of a bad keyframe among good ones, free keyframe 4 without an edge."""
    p = scene(5, [1, 2, 1, 1, 1, 0], 60, 3, stereo_share=0.3, pix_noise=0.4, pose_noise=0.003, point_noise=0.02)
    lists = [[(int(p["kf"][e]), p["uv"][e].copy(), float(p["ur"][e]), float(p["inv_sigma2"][e]), 0) for e in range(p["off"][i], p["off"][i + 1])]
             for i in range(60)]
    lists = [[o for o in l if o[0] not in (4, 5)] for l in lists]          # nobody sees 4 or 5
    lists[1] = []
    lists[2] = [(5, np.array([300.0, 200.0], np.float32), -1.0, 1.0, 1)]
    lists[3] = lists[3] + [(5, np.array([310.0, 210.0], np.float32), -1.0, 1.0, 1)]
    p["point_bad"][0] = 1
    off, kf, uv, ur, inv, kb = [0], [], [], [], [], []
    for l in lists:
        for o in l:
            kf.append(o[0]); uv.append(o[1]); ur.append(o[2]); inv.append(o[3]); kb.append(o[4])
        off.append(len(kf))
    p.update(off=np.array(off, np.int32), kf=np.array(kf, np.int32), uv=np.array(uv, np.float32).reshape(-1, 2), ur=np.array(ur, np.float32),
             inv_sigma2=np.array(inv, np.float32), kf_bad=np.array(kb, np.uint8))
    return p


def around_switch(K):
    """K free keyframes and two fixed ones, ~10 points per camera: 32 is the last size the LDS solver takes, 33 and 43 the blocked one's
    (198 and 258 unknowns: four and five panels and a remainder)"""
    return scene(9 + K, [1] * K + [2, 2], 10 * K, 3, stereo_share=0.5, pix_noise=0.3, pose_noise=0.002, point_noise=0.01)


def band(K=64, n_points=600, seed=17):
    """K free keyframes on a line and a fixed one at each end; every point is seen by 3 to 6 NEIGHBOURING cameras, so block (i, j) of
    the reduced system is empty for |i - j| > 5"""
    rng = np.random.default_rng(seed)
    roles = np.array([2] + [1] * K + [2], np.uint8)
    n_kf = len(roles)
    T_true = np.zeros((n_kf, 4, 4))
    centres = np.zeros((n_kf, 3))
    for c in range(n_kf):
        R = ba_cases._rot(rng.normal(0, 0.03, 3))
        centres[c] = [0.3 * c, rng.normal(0, 0.03), rng.normal(0, 0.03)]
        T_true[c] = np.eye(4)
        T_true[c, :3, :3] = R
        T_true[c, :3, 3] = -R @ centres[c]
    fx, fy, cx, cy = CAM
    off, kf, uv, ur, inv, X_true = [0], [], [], [], [], []
    for i in range(n_points):
        k = int(rng.integers(3, 7))
        first = int(rng.integers(0, n_kf - k + 1))
        X = np.array([0.3 * (first + 0.5 * (k - 1)) + rng.uniform(-1.0, 1.0), rng.uniform(-1.0, 1.0), rng.uniform(3.0, 6.0)])
        X_true.append(X)
        for c in range(first, first + k):
            pc = T_true[c, :3, :3] @ X + T_true[c, :3, 3]
            octave = int(rng.integers(0, 4))
            du, dv, dr = rng.normal(0, 1, 3) * 0.3 * 1.2 ** octave
            kf.append(c)
            uv.append((fx * pc[0] / pc[2] + cx + du, fy * pc[1] / pc[2] + cy + dv))
            ur.append(fx * pc[0] / pc[2] + cx - BF / pc[2] + dr if rng.uniform() < 0.4 else -1.0)
            inv.append(INV_SIGMA2[octave])
        off.append(len(kf))
    X_true = np.array(X_true)
    poses = T_true.copy()
    for c in np.flatnonzero(roles == 1):
        d = np.eye(4)
        d[:3, :3] = ba_cases._rot(rng.normal(0, 0.002, 3))
        d[:3, 3] = rng.normal(0, 0.002, 3)
        poses[c] = d @ T_true[c]
    return dict(off=np.array(off, np.int32), kf=np.array(kf, np.int32), uv=np.array(uv, np.float32).reshape(-1, 2), ur=np.array(ur, np.float32),
                inv_sigma2=np.array(inv, np.float32), kf_bad=np.zeros(len(kf), np.uint8), point_bad=np.zeros(n_points, np.uint8), poses=poses,
                roles=roles, Xw=X_true + rng.normal(0, 0.01, X_true.shape), cam=CAM, bf=BF, T_true=T_true, X_true=X_true)


def rejects():
    """36 free keyframes (the blocked solver) from a start with every ninth point 2 m BEHIND the cameras: the third iteration's step is
    rejected four times (rho -534, -116, -5, -12) before lambda has grown enough, so trials q > 0 run: k_ba_schur rebuilds S over
    the factor, panel 0 resets solve_ok, the estimate buffer is restored"""
    p = scene(81, [1] * 36 + [2, 2], 360, 3, stereo_share=0.5, pix_noise=0.3, pose_noise=0.01, point_noise=0.05)
    p["Xw"][::9, 2] = -2.0
    return p


def huber_delta():
    """Large planted outliers pull against inliers (a quarter of the observations 8 .. 30 px off), monocular throughout: many edges
    sit on the linear part of the kernel, where the delta scales their weight"""
    return scene(31, [2, 1, 1, 1], 80, 4, pix_noise=0.3, pose_noise=0.003, point_noise=0.02, wrong_share=0.25, wrong_px=(8.0, 30.0))


def no_vertex():
    p = noisy()
    p["roles"] = p["roles"].copy()
    p["roles"][3] = 0                                  # an observed camera that is not in vpKFs
    return p


def not_resident():
    p = noisy()
    p["kf"][int(p["off"][40])] = -2
    return p


def bad_index():
    p = noisy()
    p["kf"][int(p["off"][41]) + 1] = -3
    return p


def too_many():
    """257 cameras with role 1"""
    return scene(2, [1] * 257 + [2], 20, 3, pix_noise=0.3, pose_noise=0.002, point_noise=0.01)


# name -> (problem builder, n_iterations, robust): the runs both test files make
RUNS = dict(
    exact=(exact, 10, 1),
    mono_init=(mono_init, 20, 1),
    noisy_robust=(noisy, 10, 1),
    noisy_plain=(noisy, 10, 0),
    stereo_mix=(stereo_mix, 10, 0),
    special_points=(special_points, 10, 1),
    k32=(lambda: around_switch(32), 5, 0),
    k33=(lambda: around_switch(33), 5, 0),
    k43=(lambda: around_switch(43), 5, 0),
    band64=(band, 4, 0),
    rejects36=(rejects, 8, 0),
    one_iteration=(noisy, 1, 1),
    twenty_iterations=(stereo_mix, 20, 1),
    huber_delta=(huber_delta, 10, 1),
)
REFUSED = dict(no_vertex=(no_vertex, 4), not_resident=(not_resident, 1), bad_index=(bad_index, 3), too_many=(too_many, 2))

_CACHE = {}


def problem(name):
    if name not in _CACHE:
        _CACHE[name] = (RUNS.get(name) or REFUSED[name])[0]()
    return _CACHE[name]


def spd(n, seed):
    """M M^T + n I with seeded M, and a right-hand side: no pivot is near zero"""
    rng = np.random.default_rng(seed)
    M = rng.normal(0, 1, (n, n))
    return M @ M.T + n * np.eye(n), rng.normal(0, 1, n)


SOLVER_SIZES = (1, 6, 47, 48, 49, 198, 258, 384, 390, 1536)


def zero_pivot(panel):
    """A positive-definite 100 x 100 matrix shifted so that its LDL^T in index order meets an exact 0.0 pivot at index 5 (panel 0) or
    60 (panel 1: columns 48 .. 95).  Small integers throughout, so every Schur complement up to the pivot is exact: A = L D L^T with
    unit lower L of entries in {-1, 0, 1} (a band of width 2) and D of 1 and 2, then A[at, at] -= D[at]."""
    n, at = 100, (5 if panel == 0 else 60)
    rng = np.random.default_rng(40 + panel)
    L = np.eye(n)
    for i in range(1, n):
        L[i, max(0, i - 2):i] = rng.integers(-1, 2, min(2, i))
    d = rng.choice([1.0, 2.0], n)
    A = L @ np.diag(d) @ L.T
    A[at, at] -= d[at]
    return A, rng.integers(-3, 4, n).astype(np.float64), at


# ---- Noise floors, measured by tests/test_global_ba_cpu.py (test_noise_floor_*) and rounded up; neither comes from the code under test.
# (a) the whole problem: the largest pose / point deviation between 9 edge and vertex orders of every run case and between the Schur,
#     the blocked and the dense solver.  The GPU bound is min(64 x floor, 1e-5), the convention of ba_cases.
NOISE_FLOOR = 2.5e-10     # measured 2.44e-10 (special_points, between edge orders)
GPU_BOUND = min(64 * NOISE_FLOOR, 1e-5)
# (b) the solver alone: the largest deviation of x between ldlt_solve, blocked_ldlt_solve and np.linalg.solve over SOLVER_SIZES,
#     relative to max |x|.  The GPU bound is 64 x that floor.
SOLVER_FLOOR = 4.3e-15     # measured 4.275e-15 (n = 1536, blocked_ldlt_solve against ldlt_solve; 3.8e-15 against np.linalg.solve)
SOLVER_BOUND = 64 * SOLVER_FLOOR
