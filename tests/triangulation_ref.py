"""numpy restatement of ORBmatcher::SearchForTriangulation (reference src/ORBmatcher.cc:359-475), its CheckDistEpipolarLine
(:128-144) and LocalMapping::ComputeF12 (src/LocalMapping.cc:494-511), with the roundings written out: every float of the
reference is an np.float32 here, every double an np.float64 (np.longdouble in the comparison variant of ComputeF12), and no
product is fused with a sum.

The scan is the reference's sequential double loop with its `continue`s in its order (bestDist / bestIdx2 updated in place),
not the "smallest key" form of the kernel, so a comparison of the two shows that they are one algorithm.  Only what a row's
gates are computed FROM is evaluated for all idx2 at once, elementwise, in the scalar arithmetic of the reference.

`counts`, when given, receives how many (idx1, idx2) pairs each gate rejected, in the order the reference applies them."""
import numpy as np

TH_LOW = 50
HISTO_LENGTH = 30
F32 = np.float32
GATES = ("row_has_point", "cand_has_point", "den_zero", "epipolar", "dist_gt_50", "dist_gt_best", "epipole", "accepted")


def scale_tables(scale_factor=1.2, nlevels=8):
    """mvScaleFactors, mvLevelSigma2 as ORBextractor builds them (float products)."""
    sf = np.ones(nlevels, F32)
    for i in range(1, nlevels):
        sf[i] = F32(sf[i - 1] * F32(scale_factor))
    return sf, (sf * sf).astype(F32)


# ------------------------------------------------------------------------------------------------ ComputeF12, epipole
def _dot3(x, y):
    return (x[0] * y[0] + x[1] * y[1]) + x[2] * y[2]


def _mul33(A, B, dt):
    out = np.zeros((3, 3), dt)
    for r in range(3):
        for c in range(3):
            out[r, c] = _dot3(A[r, :], B[:, c])
    return out


def _inv33(M, dt):
    C = np.zeros((3, 3), dt)
    for i in range(3):
        for j in range(3):
            i1, i2, j1, j2 = (i + 1) % 3, (i + 2) % 3, (j + 1) % 3, (j + 2) % 3
            C[i, j] = M[i1, j1] * M[i2, j2] - M[i1, j2] * M[i2, j1]
    invdet = dt(1.0) / _dot3(M[0, :], C[0, :])
    out = np.zeros((3, 3), dt)
    for i in range(3):
        for j in range(3):
            out[i, j] = C[j, i] * invdet
    return out


def camera_matrix(K, dt=np.float64):
    fx, fy, cx, cy = [dt(F32(v)) for v in K]          # the tracker's camera: float parameters
    return np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1]], dt)


def compute_f12(T1, T2, K, dt=np.float64):
    """F12 = K^-T [t12]x R12 K^-1 with T1 = KF1's Tcw, T2 = KF2's; products as sums k = 0..2 in order, chains left to right,
    3 x 3 inverse by cofactors (the order sdslam_amd/csrc/track_tri.hip documents)."""
    T1, T2 = np.asarray(T1, np.float64).astype(dt), np.asarray(T2, np.float64).astype(dt)
    R1, t1, R2, t2 = T1[:3, :3], T1[:3, 3], T2[:3, :3], T2[:3, 3]
    R12 = _mul33(R1, R2.T.copy(), dt)
    t12 = np.array([_dot3(-R12[r, :], t2) + t1[r] for r in range(3)], dt)
    z = dt(0.0)
    tx = np.array([[z, -t12[2], t12[1]], [t12[2], z, -t12[0]], [-t12[1], t12[0], z]], dt)
    Km = camera_matrix(K, dt)
    return _mul33(_mul33(_mul33(_inv33(Km.T.copy(), dt), tx, dt), R12, dt), _inv33(Km, dt), dt)


def compute_f12_longdouble(T1, T2, K):
    return compute_f12(T1, T2, K, np.longdouble)


def epipole(T1, T2, K):
    """(ex, ey) of :362-368: KF1's camera centre in KF2's image."""
    T1, T2 = np.asarray(T1, np.float64), np.asarray(T2, np.float64)
    R1, t1, R2, t2 = T1[:3, :3], T1[:3, 3], T2[:3, :3], T2[:3, 3]
    Cw = np.array([-_dot3(R1[:, r], t1) for r in range(3)])
    C2 = np.array([_dot3(R2[r, :], Cw) + t2[r] for r in range(3)])
    fx, fy, cx, cy = [np.float64(F32(v)) for v in K]
    with np.errstate(all="ignore"):
        invz = F32(np.float64(1.0) / C2[2])
        ex = F32(fx * C2[0] * np.float64(invz) + cx)
        ey = F32(fy * C2[1] * np.float64(invz) + cy)
    return np.array([ex, ey], F32)


# ------------------------------------------------------------------------------------------------ the matcher
def epipolar_line(x1, y1, F12):
    """(a, b, c, den) of :130-136 for one KF1 keypoint."""
    F = np.asarray(F12, np.float64)
    x1, y1 = np.float64(F32(x1)), np.float64(F32(y1))
    with np.errstate(all="ignore"):
        a = F32(x1 * F[0, 0] + y1 * F[1, 0] + F[2, 0])
        b = F32(x1 * F[0, 1] + y1 * F[1, 1] + F[2, 1])
        c = F32(x1 * F[0, 2] + y1 * F[1, 2] + F[2, 2])
        den = F32(F32(a * a) + F32(b * b))
    return a, b, c, den


def dsqr_of(a, b, c, den, x2, y2):
    """num * num / den of :134-141, float; x2 / y2 scalars or arrays."""
    with np.errstate(all="ignore"):
        num = (a * np.asarray(x2, F32) + b * np.asarray(y2, F32)) + c
        return (num * num) / den


def rot_bin(angle1, angle2):
    rot = F32(F32(angle1) - F32(angle2))
    if rot < 0.0:
        rot = F32(rot + F32(360.0))
    v = F32(rot * (F32(1.0) / F32(HISTO_LENGTH)))
    b = int(np.floor(np.float64(v) + 0.5))            # round(): half away from zero, v >= 0
    return 0 if b == HISTO_LENGTH else b


def three_maxima(sizes):
    max1 = max2 = max3 = 0
    ind1 = ind2 = ind3 = -1
    for i, s in enumerate(sizes):
        if s > max1:
            max3, max2, max1 = max2, max1, s
            ind3, ind2, ind1 = ind2, ind1, i
        elif s > max2:
            max3, max2 = max2, s
            ind3, ind2 = ind2, i
        elif s > max3:
            max3, ind3 = s, i
    if F32(max2) < F32(0.1) * F32(max1):
        ind2 = ind3 = -1
    elif F32(max3) < F32(0.1) * F32(max1):
        ind3 = -1
    return ind1, ind2, ind3


def search_for_triangulation(kps1, desc1, has1, ur1, kps2, desc2, has2, ur2, F12, epi, sf, sigma2, check_ori=False, counts=None):
    """Returns (nmatches, matches12[N1]); kps*: structured arrays with x, y, angle, octave (undistorted keypoints)."""
    N1, N2 = len(kps1), len(kps2)
    m12 = np.full(N1, -1, np.int32)
    cnt = dict.fromkeys(GATES, 0)
    ex, ey = F32(epi[0]), F32(epi[1])
    x2, y2 = kps2["x"].astype(F32), kps2["y"].astype(F32)
    oct2 = kps2["octave"].astype(np.int64)
    thr = np.float64(3.84) * np.asarray(sigma2, F32)[oct2].astype(np.float64) if N2 else np.zeros(0)
    with np.errstate(all="ignore"):
        distex, distey = ex - x2, ey - y2
        near_epipole = ((distex * distex + distey * distey) < F32(100) * np.asarray(sf, F32)[oct2]).tolist() if N2 else []
    stereo2 = (np.asarray(ur2, F32) >= 0).tolist()
    has2_l = [bool(v) for v in has2]
    bits2 = np.unpackbits(np.asarray(desc2, np.uint8).reshape(N2, 32), axis=1) if N2 else np.zeros((0, 256), np.uint8)
    rot_hist = [[] for _ in range(HISTO_LENGTH)]
    nmatches = 0
    for idx1 in range(N1):
        if has1[idx1]:
            cnt["row_has_point"] += N2
            continue
        stereo1 = bool(F32(ur1[idx1]) >= 0)
        a, b, c, den = epipolar_line(kps1["x"][idx1], kps1["y"][idx1], F12)
        dsqr = dsqr_of(a, b, c, den, x2, y2)
        epi_ok = (dsqr.astype(np.float64) < thr).tolist()
        dist = (np.unpackbits(np.asarray(desc1[idx1], np.uint8)) ^ bits2).sum(axis=1).tolist()
        best_dist, best_idx2 = TH_LOW, -1
        for idx2 in range(N2):
            if has2_l[idx2]:
                cnt["cand_has_point"] += 1
                continue
            if den == 0:
                cnt["den_zero"] += 1
                continue
            if not epi_ok[idx2]:
                cnt["epipolar"] += 1
                continue
            d = dist[idx2]
            if d > TH_LOW:
                cnt["dist_gt_50"] += 1
                continue
            if d > best_dist:
                cnt["dist_gt_best"] += 1
                continue
            if not stereo1 and not stereo2[idx2] and near_epipole[idx2]:
                cnt["epipole"] += 1
                continue
            cnt["accepted"] += 1
            best_idx2, best_dist = idx2, d
        if best_idx2 >= 0:
            m12[idx1] = best_idx2
            nmatches += 1
            if check_ori:
                rot_hist[rot_bin(kps1["angle"][idx1], kps2["angle"][best_idx2])].append(idx1)
    if check_ori:
        keep = three_maxima([len(h) for h in rot_hist])
        for i in range(HISTO_LENGTH):
            if i in keep:
                continue
            for idx1 in rot_hist[i]:
                m12[idx1] = -1
                nmatches -= 1
    if counts is not None:
        counts.update(cnt)
    return nmatches, m12


def pairs_of(m12):
    """vMatchedPairs (:465-472)."""
    return [(int(i), int(j)) for i, j in enumerate(m12) if j >= 0]


def create_new_map_points_order(run_neighbour, has1, n_neighbours):
    """CreateNewMapPoints' walk over the neighbours with triangulation taken as always succeeding: neighbour i is searched with the
    idx1 that earlier neighbours turned into points flagged.  run_neighbour(i, flags) -> matches12.  Returns the pair lists."""
    flags = np.array(has1, np.uint8).copy()
    out = []
    for i in range(n_neighbours):
        m = np.asarray(run_neighbour(i, flags.copy()))
        out.append(pairs_of(m))
        flags[np.flatnonzero(m >= 0)] = 1
    return out
