"""numpy restatement of SD_SLAM::Sim3Solver (reference src/Sim3Solver.cc), line by line, with the state that lives across
iterate() calls.  float32 where the reference is float: Converter::toCvMat, cv::eigen (OpenCV 3.2 JacobiImpl_<float>), the
angle-axis vector, the CV_32F output of cv::Rodrigues, invz / x / y and the image coordinates, err1 / err2, ms12i, epsilon.
mvnMaxError is a vector<size_t>: 9.210 * sigma2 is truncated.  Random() takes raw rand() values (src/extra/utils.cc:23-26).

Every scalar operation below is one IEEE operation on np.float32 / np.float64 values in the order DESIGN.md §3 fixes.

A keyframe is a dict: T (4x4 float64, Tcw), Xw [n, 3] float64 (GetWorldPos() by keypoint index), has_mp [n] (map point there
and not bad), octave [n], n (keypoints), and the solver takes K = (fx, fy, cx, cy) and the pyramid's mvLevelSigma2 (float32).
"""
import math

import numpy as np

f32, f64 = np.float32, np.float64
RAND_MAX = 2147483647
INT_MIN = -2147483648
FLT_EPS = f32(np.finfo(np.float32).eps)
DBL_EPS = float(np.finfo(np.float64).eps)


def random_int(r, lo, hi):
    """SD_SLAM::Random(min, max) on the raw rand() value r."""
    d = hi - lo + 1
    return int((float(r) / (float(RAND_MAX) + 1.0)) * d + lo)


def level_sigma2(scale_factor, nlevels):
    """ORBextractor's mvLevelSigma2 (src/ORBextractor.cc:414-421), float."""
    sf = [f32(1.0)]
    for _ in range(1, nlevels):
        sf.append(f32(sf[-1] * f32(scale_factor)))
    return np.array([f32(s * s) for s in sf], np.float32)


def ransac_max_its(N, probability, min_inliers, max_iterations):
    """SetRansacParameters (:122-132).  ceil(NaN) -> int is INT_MIN on x86-64, which min / max turn into 1."""
    if min_inliers == N:
        n_it = 1
    else:
        with np.errstate(all="ignore"):
            eps = float(f32(min_inliers) / f32(N))
        try:
            n_it = math.ceil(math.log(1 - probability) / math.log(1 - math.pow(eps, 3)))
            if not (-2147483648 <= n_it < 2147483648):
                n_it = INT_MIN
        except (ValueError, ZeroDivisionError, OverflowError):
            n_it = INT_MIN
    return max(1, min(n_it, max_iterations))


def _cv_hypot(a, b):
    a, b = f32(abs(a)), f32(abs(b))
    if a > b:
        b = f32(b / a)
        return f32(a * f32(np.sqrt(f32(f32(1) + f32(b * b)))))
    if b > 0:
        a = f32(a / b)
        return f32(b * f32(np.sqrt(f32(f32(1) + f32(a * a)))))
    return f32(0)


def jacobi_eigen(N, stats=None):
    """cv::eigen(N, eval, evec) for a symmetric CV_32F matrix: OpenCV 3.2 JacobiImpl_<float>.  Returns (W descending, V with the
    eigenvectors as rows).  stats["tie"] is set when a pivot search compared two equal non-zero magnitudes."""
    n = N.shape[0]
    A = [[f32(N[i, j]) for j in range(n)] for i in range(n)]
    V = [[f32(1) if i == j else f32(0) for j in range(n)] for i in range(n)]
    W = [A[k][k] for k in range(n)]
    indR, indC = [0] * n, [0] * n

    def note(mv, val):
        if stats is not None and mv == val and val != 0:
            stats["tie"] = True

    def refresh(k):
        if k < n - 1:
            m, mv = k + 1, abs(A[k][k + 1])
            for i in range(k + 2, n):
                val = abs(A[k][i])
                note(mv, val)
                if mv < val:
                    mv, m = val, i
            indR[k] = m
        if k > 0:
            m, mv = 0, abs(A[0][k])
            for i in range(1, k):
                val = abs(A[i][k])
                note(mv, val)
                if mv < val:
                    mv, m = val, i
            indC[k] = m

    for k in range(n):
        refresh(k)
    for _ in range(n * n * 30 if n > 1 else 0):
        k, mv = 0, abs(A[0][indR[0]])
        for i in range(1, n - 1):
            val = abs(A[i][indR[i]])
            note(mv, val)
            if mv < val:
                mv, k = val, i
        l = indR[k]
        for i in range(1, n):
            val = abs(A[indC[i]][i])
            if not (indC[i] == k and i == l):
                note(mv, val)
            if mv < val:
                mv, k, l = val, indC[i], i
        p = A[k][l]
        if abs(p) <= FLT_EPS:
            break
        y = f32(f32(W[l] - W[k]) * f32(0.5))
        t = f32(abs(y) + _cv_hypot(p, y))
        s = _cv_hypot(p, t)
        c = f32(t / s)
        s = f32(p / s)
        t = f32(f32(p / t) * p)
        if y < 0:
            s, t = f32(-s), f32(-t)
        A[k][l] = f32(0)
        W[k] = f32(W[k] - t)
        W[l] = f32(W[l] + t)

        def rot(a0, b0):
            return f32(f32(a0 * c) - f32(b0 * s)), f32(f32(a0 * s) + f32(b0 * c))

        for i in range(0, k):
            A[i][k], A[i][l] = rot(A[i][k], A[i][l])
        for i in range(k + 1, l):
            A[k][i], A[i][l] = rot(A[k][i], A[i][l])
        for i in range(l + 1, n):
            A[k][i], A[l][i] = rot(A[k][i], A[l][i])
        for i in range(n):
            V[k][i], V[l][i] = rot(V[k][i], V[l][i])
        refresh(k)
        refresh(l)
    for k in range(n - 1):
        m = k
        for i in range(k + 1, n):
            if W[m] < W[i]:
                m = i
        if k != m:
            W[m], W[k] = W[k], W[m]
            V[m], V[k] = V[k], V[m]
    return np.array(W, np.float32), np.array(V, np.float32)


def rodrigues(r):
    """cv::Rodrigues on a CV_32F 3-vector into a CV_32F matrix: computed in double, rounded to float."""
    rx, ry, rz = (f64(v) for v in r)
    with np.errstate(all="ignore"):
        theta = f64(np.sqrt(rx * rx + ry * ry + rz * rz))
        if theta < DBL_EPS:
            R = np.eye(3)
        elif not np.isfinite(theta):
            R = np.full((3, 3), np.nan)
        else:
            c, s = f64(math.cos(theta)), f64(math.sin(theta))
            c1, it = f64(1.0) - c, f64(1.0) / theta
            rx, ry, rz = rx * it, ry * it, rz * it
            rrt = [rx * rx, rx * ry, rx * rz, rx * ry, ry * ry, ry * rz, rx * rz, ry * rz, rz * rz]
            rxm = [f64(0), -rz, ry, rz, f64(0), -rx, -ry, rx, f64(0)]
            I = [1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0]
            R = np.array([(c * I[k] + c1 * rrt[k]) + s * rxm[k] for k in range(9)]).reshape(3, 3)
        return R.astype(np.float32)


def compute_sim3(P1, P2, fix_scale, stats=None):
    """ComputeSim3 (:216-318).  P1, P2: 3x3 float64, one drawn point per column.  Returns R (float values in float64), s
    (float32), t, T12, T21."""
    with np.errstate(all="ignore"):
        O1 = np.array([(P1[r, 0] + (P1[r, 1] + P1[r, 2])) / 3.0 for r in range(3)])
        O2 = np.array([(P2[r, 0] + (P2[r, 1] + P2[r, 2])) / 3.0 for r in range(3)])
        Pr1, Pr2 = P1 - O1[:, None], P2 - O2[:, None]
        M = np.array([[(Pr2[i, 0] * Pr1[j, 0] + Pr2[i, 1] * Pr1[j, 1]) + Pr2[i, 2] * Pr1[j, 2] for j in range(3)] for i in range(3)])
        N11 = M[0, 0] + M[1, 1] + M[2, 2]
        N12, N13, N14 = M[1, 2] - M[2, 1], M[2, 0] - M[0, 2], M[0, 1] - M[1, 0]
        N22 = M[0, 0] - M[1, 1] - M[2, 2]
        N23, N24 = M[0, 1] + M[1, 0], M[2, 0] + M[0, 2]
        N33 = -M[0, 0] + M[1, 1] - M[2, 2]
        N34 = M[1, 2] + M[2, 1]
        N44 = -M[0, 0] - M[1, 1] + M[2, 2]
        N = np.array([[N11, N12, N13, N14], [N12, N22, N23, N24], [N13, N23, N33, N34], [N14, N24, N34, N44]]).astype(np.float32)
        _, evec = jacobi_eigen(N, stats)
        q = evec[0]
        nrm2 = f64(0)
        for i in range(1, 4):
            nrm2 = nrm2 + f64(q[i]) * f64(q[i])
        nrm = f64(np.sqrt(nrm2))
        ang = f64(math.atan2(nrm, float(q[0])))
        alpha = f32((f64(2) * ang) * (f64(1.0) / nrm))
        vec = np.array([f32(q[i] * alpha) for i in range(1, 4)], np.float32)
        R = rodrigues(vec).astype(np.float64)
        P3 = np.array([[(R[i, 0] * Pr2[0, j] + R[i, 1] * Pr2[1, j]) + R[i, 2] * Pr2[2, j] for j in range(3)] for i in range(3)])
        if not fix_scale:
            pr = [f64(f32(Pr1[i, j])) * f64(f32(P3[i, j])) for i in range(3) for j in range(3)]
            nom = f64(0)
            nom = nom + (((pr[0] + pr[1]) + pr[2]) + pr[3])
            nom = nom + (((pr[4] + pr[5]) + pr[6]) + pr[7])
            nom = nom + pr[8]
            den = f64(0)
            for i in range(3):
                for j in range(3):
                    den = den + P3[i, j] * P3[i, j]
            s = f32(nom / den)
        else:
            s = f32(1.0)
        sd = f64(s)
        sR = sd * R
        t = np.array([O1[i] - ((sR[i, 0] * O2[0] + sR[i, 1] * O2[1]) + sR[i, 2] * O2[2]) for i in range(3)])
        sRi = (f64(1.0) / sd) * R.T
        ti = np.array([((-sRi[i, 0]) * t[0] + (-sRi[i, 1]) * t[1]) + (-sRi[i, 2]) * t[2] for i in range(3)])
    T12, T21 = np.eye(4), np.eye(4)
    T12[:3, :3], T12[:3, 3] = sR, t
    T21[:3, :3], T21[:3, 3] = sRi, ti
    return R, s, t, T12, T21


def to_image(P, K):
    """FromCameraToImage / the tail of Project on camera-frame points [n, 3]: invz, x, y float; fx * x + cx is a float
    expression whose value the Vector2d holds as a double.  Returns float64 [n, 2]."""
    fx, fy, cx, cy = (f32(v) for v in K)
    with np.errstate(all="ignore"):
        invz = (1.0 / P[:, 2]).astype(np.float32)
        x = (P[:, 0] * invz.astype(np.float64)).astype(np.float32)
        y = (P[:, 1] * invz.astype(np.float64)).astype(np.float32)
        return np.stack([(fx * x + cx).astype(np.float64), (fy * y + cy).astype(np.float64)], axis=1)


def transform(T, X):
    """Rcw * X + tcw for points [n, 3], products summed in column order."""
    return ((T[:3, 0] * X[:, 0:1] + T[:3, 1] * X[:, 1:2]) + T[:3, 2] * X[:, 2:3]) + T[:3, 3]


class Sim3Solver:
    def __init__(self, kf1, kf2, matches12, fix_scale, K, sigma2, rand_values, cache=None):
        # cache: iteration number -> its hypothesis and mask (they depend on nothing else: 3 rand() values per iteration),
        # shared between solvers built on the same inputs
        self.cache = cache
        self.fix_scale = bool(fix_scale)
        self.K = K
        self.mN1 = len(matches12)
        self.rand = np.asarray(rand_values, np.int64)
        self.rpos = 0
        idx1, idx2 = [], []
        for i1 in range(min(self.mN1, kf1["n"])):
            m = int(matches12[i1])
            if m < 0 or m >= kf2["n"]:
                continue
            if not kf1["has_mp"][i1] or not kf2["has_mp"][m]:
                continue
            idx1.append(i1)
            idx2.append(m)
        self.idx1 = np.array(idx1, np.int64)
        i2 = np.array(idx2, np.int64)
        self.max_err1 = np.array([f32(int(9.210 * float(sigma2[kf1["octave"][i]]))) for i in idx1], np.float32)
        self.max_err2 = np.array([f32(int(9.210 * float(sigma2[kf2["octave"][i]]))) for i in idx2], np.float32)
        self.X1 = transform(kf1["T"], kf1["Xw"][self.idx1].reshape(-1, 3))
        self.X2 = transform(kf2["T"], kf2["Xw"][i2].reshape(-1, 3))
        self.P1im1, self.P2im2 = to_image(self.X1, K), to_image(self.X2, K)
        self.N = len(idx1)
        self.iterations = 0
        self.best_inliers = 0
        self.best_mask = np.zeros(self.N, bool)
        self.best_T12 = np.zeros((4, 4))
        self.best_R, self.best_t, self.best_s = np.zeros((3, 3)), np.zeros(3), f32(0)
        # margin bookkeeping (tests/test_sim3_cpu.py (e)): smallest relative distance of an error to its threshold, smallest
        # |z| of a projected point, whether a Jacobi pivot search was tied
        self.stats = dict(err_gap=np.inf, min_z=np.inf, tie=False, hypotheses=0)
        self.set_ransac_parameters()

    def set_ransac_parameters(self, probability=0.99, min_inliers=6, max_iterations=300):
        self.min_inliers = min_inliers
        self.max_its = ransac_max_its(self.N, probability, min_inliers, max_iterations)
        self.iterations = 0

    def _random(self, lo, hi):
        r = int(self.rand[self.rpos])
        self.rpos += 1
        return random_int(r, lo, hi)

    def _project(self, X, T):
        P = transform(T, X)
        self.stats["min_z"] = min(self.stats["min_z"], float(np.abs(P[:, 2]).min()))
        return to_image(P, self.K)

    def _check_inliers(self, T12, T21):
        P2im1, P1im2 = self._project(self.X2, T12), self._project(self.X1, T21)
        d1, d2 = self.P1im1 - P2im1, P1im2 - self.P2im2
        with np.errstate(all="ignore"):
            e1 = (d1[:, 0] * d1[:, 0] + d1[:, 1] * d1[:, 1]).astype(np.float32)
            e2 = (d2[:, 0] * d2[:, 0] + d2[:, 1] * d2[:, 1]).astype(np.float32)
            for e, m in ((e1, self.max_err1), (e2, self.max_err2)):
                ok = np.isfinite(e)
                if ok.any():
                    self.stats["err_gap"] = min(self.stats["err_gap"], float(np.min(np.abs(e[ok].astype(np.float64) - m[ok]) / m[ok])))
            return (e1 < self.max_err1) & (e2 < self.max_err2)

    def iterate(self, n_iterations):
        """-> (T12 4x4 or zeros, bNoMore, vbInliers [mN1], nInliers)"""
        inliers = np.zeros(self.mN1, bool)
        if self.N < self.min_inliers:
            return np.zeros((4, 4)), True, inliers, 0
        cur = 0
        while self.iterations < self.max_its and cur < n_iterations:
            cur += 1
            self.iterations += 1
            if self.cache is not None and self.iterations in self.cache:
                R, s, t, T12, T21, mask = self.cache[self.iterations]
                self.rpos += 3
            else:
                avail = list(range(self.N))
                P1, P2 = np.zeros((3, 3)), np.zeros((3, 3))
                for i in range(3):
                    r = self._random(0, len(avail) - 1)
                    idx = avail[r]
                    P1[:, i], P2[:, i] = self.X1[idx], self.X2[idx]
                    avail[r] = avail[-1]
                    avail.pop()
                R, s, t, T12, T21 = compute_sim3(P1, P2, self.fix_scale, self.stats)
                self.stats["hypotheses"] += 1
                mask = self._check_inliers(T12, T21)
                if self.cache is not None:
                    self.cache[self.iterations] = (R, s, t, T12, T21, mask)
            n = int(mask.sum())
            if n >= self.best_inliers:
                self.best_mask, self.best_inliers = mask, n
                self.best_T12, self.best_R, self.best_t, self.best_s = T12, R, t, s
                if n > self.min_inliers:
                    inliers[self.idx1[mask]] = True
                    return T12.copy(), False, inliers, n
        return np.zeros((4, 4)), self.iterations >= self.max_its, inliers, 0

    def find(self):
        return self.iterate(self.max_its)

    def info8(self, result):
        T, no_more, _, n = result
        return np.array([int(T[3, 3] != 0), n, int(no_more), self.iterations, self.N, self.max_its, self.best_inliers, 0], np.int32)
