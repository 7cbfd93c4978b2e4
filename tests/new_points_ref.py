"""numpy restatement of LocalMapping::CreateNewMapPoints after the search (reference src/LocalMapping.cc:219-419), of
KeyFrame::UnprojectStereo (src/KeyFrame.cc:572-585), MapPoint::UpdateNormalAndDepth (src/MapPoint.cc:304-343) and of the float
instantiation of OpenCV 3.2's JacobiSVDImpl_ behind cv::SVD::compute, with the roundings written out: every float of the
reference is an np.float32 here, every double an np.float64, no product is fused with a sum, in the operation order the header of
sdslam_amd/csrc/track_newpoints_tri.hip fixes.  hypot is glibc's algorithm restated (not correctly rounded, so not np.hypot's to
choose).  cosParallaxStereo is cos rounded to float of 2 * atan2f: neither is bit-identical to the device's, and it feeds
comparisons only, so `triangulate` reports every stereo row's distance to them (`margins`) and the case builders keep it wide.

Scalar Python throughout: this is the statement of the arithmetic, not a fast path."""
import numpy as np

import triangulation_ref as TR

F32, F64 = np.float32, np.float64
NO_MATCH, ACCEPTED, LOW_PARALLAX, W_ZERO, Z1, Z2, REPROJ1, REPROJ2, DIST_ZERO, SCALE, SLOT_GATED = range(11)
VERDICTS = ("no_match", "accepted", "low_parallax", "w_zero", "z1", "z2", "reproj1", "reproj2", "dist_zero", "scale", "slot_gated")
BR_NONE, BR_SVD, BR_UNPROJECT1, BR_UNPROJECT2 = range(4)
FLT_EPSILON = F32(2.0 ** -23)


# ------------------------------------------------------------------------------------------------ hypot, float Jacobi SVD
def _hypot_kernel(ax, ay):
    h = np.sqrt(ax * ax + ay * ay)
    if h <= F64(2.0) * ay:
        delta = h - ay
        t1 = ax * (F64(2.0) * delta - ax)
        t2 = (delta - F64(2.0) * (ax - ay)) * delta
    else:
        delta = h - ax
        t1 = F64(2.0) * delta * (ax - F64(2.0) * ay)
        t2 = (F64(4.0) * delta - ay) * ay + delta * delta
    return h - (t1 + t2) / (F64(2.0) * h)


def hypot_glibc(x, y):
    """glibc 2.35 hypot (sdslam_amd/csrc/sd_hypot.h), finite arguments."""
    SCALE_, LARGE, TINY, EPS = F64(2.0 ** -600), F64(2.0 ** 511), F64(2.0 ** -459), F64(2.0 ** -54)
    x, y = abs(F64(x)), abs(F64(y))
    ax, ay = (y, x) if x < y else (x, y)
    with np.errstate(all="ignore"):
        if ax > LARGE:
            return ax + ay if ay <= ax * EPS else _hypot_kernel(ax * SCALE_, ay * SCALE_) / SCALE_
        if ay < TINY:
            return ax + ay if ax >= ay / EPS else _hypot_kernel(ax / SCALE_, ay / SCALE_) * SCALE_
        return ax + ay if ax >= ay / EPS else _hypot_kernel(ax, ay)


def jacobi_svd_float(A, stats=None):
    """cv::SVD::compute(A, w, u, vt) for a square CV_32F A: returns (w float64[n] descending, vt float32[n, n]).  JacobiSVDImpl_
    works on At = A^T; matrix and Vt elements float, W, a, b, p, c, s double.  The zero-singular-value tail (U only) is left out."""
    A = np.asarray(A, F32)
    n = A.shape[0]
    At = [[F32(A[k, i]) for k in range(n)] for i in range(n)]
    Vt = [[F32(1.0 if k == i else 0.0) for k in range(n)] for i in range(n)]
    eps = F64(F32(FLT_EPSILON * F32(2)))
    W = []
    with np.errstate(all="ignore"):
        for i in range(n):
            sd = F64(0)
            for k in range(n):
                sd = sd + F64(At[i][k]) * F64(At[i][k])
            W.append(sd)
        sweeps = 0
        for _ in range(max(n, 30)):
            changed = False
            sweeps += 1
            for i in range(n - 1):
                for j in range(i + 1, n):
                    a, b, p = W[i], W[j], F64(0)
                    for k in range(n):
                        p = p + F64(At[i][k]) * F64(At[j][k])
                    if abs(p) <= eps * np.sqrt(a * b):
                        continue
                    p = p * F64(2)
                    beta = a - b
                    gamma = hypot_glibc(p, beta)
                    if beta < 0:
                        delta = (gamma - beta) * F64(0.5)
                        s = np.sqrt(delta / gamma)
                        c = p / (gamma * s * F64(2))
                    else:
                        c = np.sqrt((gamma + beta) / (gamma * F64(2)))
                        s = p / (gamma * c * F64(2))
                    a = b = F64(0)
                    for k in range(n):
                        t0 = F32(c * F64(At[i][k]) + s * F64(At[j][k]))
                        t1 = F32(-s * F64(At[i][k]) + c * F64(At[j][k]))
                        At[i][k], At[j][k] = t0, t1
                        a = a + F64(t0) * F64(t0)
                        b = b + F64(t1) * F64(t1)
                    W[i], W[j] = a, b
                    changed = True
                    for k in range(n):
                        t0 = F32(c * F64(Vt[i][k]) + s * F64(Vt[j][k]))
                        t1 = F32(-s * F64(Vt[i][k]) + c * F64(Vt[j][k]))
                        Vt[i][k], Vt[j][k] = t0, t1
            if not changed:
                break
        for i in range(n):
            sd = F64(0)
            for k in range(n):
                sd = sd + F64(At[i][k]) * F64(At[i][k])
            W[i] = np.sqrt(sd)
    for i in range(n - 1):
        j = i
        for k in range(i + 1, n):
            if W[j] < W[k]:
                j = k
        if i != j:
            W[i], W[j] = W[j], W[i]
            Vt[i], Vt[j] = Vt[j], Vt[i]
    if stats is not None:
        stats["sweeps"] = sweeps
    return np.array(W, F64), np.array(Vt, F32)


# ------------------------------------------------------------------------------------------------ poses
def dot3(x, y):
    return (x[0] * y[0] + x[1] * y[1]) + x[2] * y[2]


class Pose:
    """Rcw, tcw and Ow = -Rwc * tcw of a Tcw."""

    def __init__(self, T):
        T = np.asarray(T, F64)
        self.R = T[:3, :3].copy()
        self.t = T[:3, 3].copy()
        self.Ow = np.array([-dot3(self.R[:, r], self.t) for r in range(3)], F64)

    def rotate_back(self, v):
        return np.array([dot3(self.R[:, r], v) for r in range(3)], F64)

    def to_camera(self, r, X):
        return dot3(self.R[r, :], X) + self.t[r]


def norm3f(d):
    return F32(np.sqrt(dot3(d, d)))


def camera(cam5):
    """fx, fy, cx, cy, mbf (floats) -> dict with invfx / invfy = 1.0f / fx and mb = mbf / fx."""
    fx, fy, cx, cy, bf = [F32(v) for v in cam5]
    return dict(fx=fx, fy=fy, cx=cx, cy=cy, bf=bf, invfx=F32(F32(1) / fx), invfy=F32(F32(1) / fy), mb=F32(bf / fx))


def unproject_stereo(P, kp, z, cam):
    z = F32(z)
    if not z > 0:
        return np.zeros(3, F64)
    x = F32(F32(F32(F32(kp["x"]) - cam["cx"]) * z) * cam["invfx"])
    y = F32(F32(F32(F32(kp["y"]) - cam["cy"]) * z) * cam["invfy"])
    return P.rotate_back(np.array([x, y, z], F64)) + P.Ow


def slot_gated(P1, P2, cam, monocular, median):
    """:225-239."""
    baseline = norm3f(P2.Ow - P1.Ow)
    if monocular:
        median = F32(median)
        with np.errstate(all="ignore"):
            return bool(median >= 0 and F64(F32(baseline / median)) < F64(0.01))
    return bool(baseline < cam["mb"])


# ------------------------------------------------------------------------------------------------ one match
def _reprojection_fails(cam, x, y, z, kp, stereo, ur, sigma2):
    invz = F32(F64(1.0) / F64(z))
    u = F32(F32(F32(cam["fx"] * x) * invz) + cam["cx"])
    v = F32(F32(F32(cam["fy"] * y) * invz) + cam["cy"])
    ex, ey = F32(u - F32(kp["x"])), F32(v - F32(kp["y"]))
    e2 = F32(F32(ex * ex) + F32(ey * ey))
    if not stereo:
        return bool(F64(e2) > F64(5.991) * F64(sigma2))
    er = F32(F32(u - F32(cam["bf"] * invz)) - F32(ur))
    e2 = F32(e2 + F32(er * er))
    return bool(F64(e2) > F64(7.8) * F64(sigma2))


def triangulate_match(kp1u, kp1, ur1, z1, kp2u, kp2, ur2, z2, P1, P2, cam, sf, sigma2, ratio_factor, detail=None):
    """:268-399 for one match -> (verdict, branch, x3D).  detail, when given, receives cos_rays, the stereo cosines, A and w."""
    nlev = len(sf)
    st1, st2 = bool(F32(ur1) >= 0), bool(F32(ur2) >= 0)
    o1, o2 = min(max(int(kp1u["octave"]), 0), nlev - 1), min(max(int(kp2u["octave"]), 0), nlev - 1)
    X = np.zeros(3, F64)
    with np.errstate(all="ignore"):
        xn1 = np.array([F32(F32(F32(kp1u["x"]) - cam["cx"]) * cam["invfx"]), F32(F32(F32(kp1u["y"]) - cam["cy"]) * cam["invfy"]), 1.0], F64)
        xn2 = np.array([F32(F32(F32(kp2u["x"]) - cam["cx"]) * cam["invfx"]), F32(F32(F32(kp2u["y"]) - cam["cy"]) * cam["invfy"]), 1.0], F64)
        ray1, ray2 = P1.rotate_back(xn1), P2.rotate_back(xn2)
        cos_rays = F32(dot3(ray1, ray2) / (np.sqrt(dot3(ray1, ray1)) * np.sqrt(dot3(ray2, ray2))))
        cos_st1 = cos_st2 = F32(cos_rays + F32(1))
        half_mb = F32(cam["mb"] / F32(2))
        if st1:
            cos_st1 = F32(np.cos(F64(F32(F32(2) * np.arctan2(half_mb, F32(z1))))))
        elif st2:
            cos_st2 = F32(np.cos(F64(F32(F32(2) * np.arctan2(half_mb, F32(z2))))))
        cos_st = min(cos_st1, cos_st2)
        if detail is not None:
            detail.update(cos_rays=cos_rays, cos_st1=cos_st1, cos_st2=cos_st2, st1=st1, st2=st2)
        if cos_rays < cos_st and cos_rays > 0 and (st1 or st2 or F64(cos_rays) < F64(0.9998)):
            branch = BR_SVD
            T1, T2 = np.column_stack([P1.R, P1.t]), np.column_stack([P2.R, P2.t])
            A = np.array([xn1[0] * T1[2] - T1[0], xn1[1] * T1[2] - T1[1], xn2[0] * T2[2] - T2[0], xn2[1] * T2[2] - T2[1]], F64).astype(F32)
            w, vt = jacobi_svd_float(A)
            h = vt[3]
            if detail is not None:
                detail.update(A=A, w=w, h=h)
            if h[3] == 0:
                return W_ZERO, branch, X
            X = np.array([F32(h[k] / h[3]) for k in range(3)], F64)
        elif st1 and cos_st1 < cos_st2:
            branch = BR_UNPROJECT1
            X = unproject_stereo(P1, kp1, z1, cam)
        elif st2 and cos_st2 < cos_st1:
            branch = BR_UNPROJECT2
            X = unproject_stereo(P2, kp2, z2, cam)
        else:
            return LOW_PARALLAX, BR_NONE, X
        zc1 = F32(P1.to_camera(2, X))
        if zc1 <= 0:
            return Z1, branch, X
        zc2 = F32(P2.to_camera(2, X))
        if zc2 <= 0:
            return Z2, branch, X
        if _reprojection_fails(cam, F32(P1.to_camera(0, X)), F32(P1.to_camera(1, X)), zc1, kp1u, st1, ur1, sigma2[o1]):
            return REPROJ1, branch, X
        if _reprojection_fails(cam, F32(P2.to_camera(0, X)), F32(P2.to_camera(1, X)), zc2, kp2u, st2, ur2, sigma2[o2]):
            return REPROJ2, branch, X
        dist1, dist2 = norm3f(X - P1.Ow), norm3f(X - P2.Ow)
        if dist1 == 0 or dist2 == 0:
            return DIST_ZERO, branch, X
        ratio_dist, ratio_oct = F32(dist2 / dist1), F32(F32(sf[o1]) / F32(sf[o2]))
        if detail is not None:
            detail.update(ratio_dist=ratio_dist, ratio_oct=ratio_oct)
        if F32(ratio_dist * ratio_factor) < ratio_oct or ratio_dist > F32(ratio_oct * ratio_factor):
            return SCALE, branch, X
    return ACCEPTED, branch, X


def stereo_margin(d):
    """Distance of cosParallaxRays (and of cosParallaxRays + 1, which the other cosine holds) to the stereo cosine in use: a
    device atan2f / cosf a few ulp off cannot flip a comparison while this stays above 1e-5.  None for a mono pair."""
    if not (d["st1"] or d["st2"]):
        return None
    c = F64(d["cos_st1"] if d["st1"] else d["cos_st2"])
    return float(min(abs(F64(d["cos_rays"]) - c), abs(F64(d["cos_rays"]) + 1.0 - c)))


def triangulate(k1u, k1, ur1, z1, k2u, k2, ur2, z2, matches12, T1, T2, cam5, sf, sigma2, scale_factor, monocular=True, median=-1.0,
                margins=None):
    """Every row of one keyframe pair -> verdict uint8[n1], branch uint8[n1], Xw float64[n1, 3] (what k_triangulate writes)."""
    n1 = len(k1u)
    cam, P1, P2 = camera(cam5), Pose(T1), Pose(T2)
    ratio_factor = F32(F32(1.5) * F32(scale_factor))
    verdict, branch, Xw = np.zeros(n1, np.uint8), np.zeros(n1, np.uint8), np.zeros((n1, 3), F64)
    gated = slot_gated(P1, P2, cam, monocular, median)
    for i in range(n1):
        j = int(matches12[i])
        if j < 0:
            continue
        if gated:
            verdict[i] = SLOT_GATED
            continue
        d = {}
        verdict[i], branch[i], Xw[i] = triangulate_match(k1u[i], k1[i], ur1[i], z1[i], k2u[j], k2[j], ur2[j], z2[j], P1, P2, cam, sf,
                                                         sigma2, ratio_factor, d)
        if margins is not None and stereo_margin(d) is not None:
            margins.append(stereo_margin(d))
    return verdict, branch, Xw


# ------------------------------------------------------------------------------------------------ the new points
def point_fields(X, i1, P1, P2, k1u, d1, sf):
    """UpdateNormalAndDepth over the two observations, pRefKF = KF1; the descriptor is KF1's."""
    n1, n2 = X - P1.Ow, X - P2.Ow
    l1, l2 = np.sqrt(dot3(n1, n1)), np.sqrt(dot3(n2, n2))
    normal = (n1 / l1 + n2 / l2) / F64(2)
    nlev = len(sf)
    mx = F32(F32(l1) * F32(sf[min(max(int(k1u[i1]["octave"]), 0), nlev - 1)]))
    return dict(Xw=X.copy(), normal=normal, max_dist=mx, min_dist=F32(mx / F32(sf[nlev - 1])), desc=np.array(d1[i1], np.uint8))


def resolve(verdicts, matches, Xws, T1s, T2s, k1u, d1, sf, next_id, broadcast):
    """k_new_points_resolve: verdicts / matches / Xws per slot; k1u / d1 per slot when paired, of KF1 when broadcast.
    Returns (list of point dicts in (slot, idx1) order, next ids after)."""
    B = len(verdicts)
    next_id = [int(v) for v in next_id]
    taken, pts = set(), []
    for b in range(B):
        ku, dd = (k1u, d1) if broadcast else (k1u[b], d1[b])
        P1, P2 = Pose(T1s[b]), Pose(T2s[b])
        for i in np.flatnonzero(np.asarray(verdicts[b]) == ACCEPTED):
            i = int(i)
            if broadcast and i in taken:
                continue
            taken.add(i)
            c = 0 if broadcast else b
            p = point_fields(np.asarray(Xws[b][i], F64), i, P1, P2, ku, dd, sf)
            p.update(kp1=i, slot=b, idx2=int(matches[b][i]), id=next_id[c])
            next_id[c] += 1
            pts.append(p)
    return pts, next_id


def create_new_map_points(k1u, k1, d1, has1, ur1, z1, neigh, T1, cam5, sf, sigma2, scale_factor, monocular, next_id, log=None):
    """The reference's loop (:219-419), sequential: neighbour i is gated, searched with the flags as the earlier neighbours left
    them, and each accepted match becomes a point at once.  neigh: list of dict(ku, k, d, has, ur, z, T, median).
    Returns the point dicts in creation order."""
    has1 = np.array(has1, np.uint8).copy()
    cam, P1 = camera(cam5), Pose(T1)
    K = tuple(float(v) for v in cam5[:4])
    ratio_factor = F32(F32(1.5) * F32(scale_factor))
    pts, nid = [], int(next_id)
    for b, nb in enumerate(neigh):
        P2 = Pose(nb["T"])
        if slot_gated(P1, P2, cam, monocular, nb["median"]):
            continue
        F12, epi = TR.compute_f12(T1, nb["T"], K), TR.epipole(T1, nb["T"], K)
        _, m12 = TR.search_for_triangulation(k1u, d1, has1, ur1, nb["ku"], nb["d"], nb["has"], nb["ur"], F12, epi, sf, sigma2, False)
        for i, j in TR.pairs_of(m12):
            v, _, X = triangulate_match(k1u[i], k1[i], ur1[i], z1[i], nb["ku"][j], nb["k"][j], nb["ur"][j], nb["z"][j], P1, P2, cam, sf,
                                        sigma2, ratio_factor)
            if log is not None:
                log.append((b, i, j, v))
            if v != ACCEPTED:
                continue
            p = point_fields(X, i, P1, P2, k1u, d1, sf)
            p.update(kp1=i, slot=b, idx2=j, id=nid)
            nid += 1
            has1[i] = 1                     # AddMapPoint(pMP, idx1): later neighbours skip the keypoint
            pts.append(p)
    return pts


def same_points(a, b):
    """Point for point, id for id, bit for bit."""
    if len(a) != len(b):
        return False
    for p, q in zip(a, b):
        if (p["kp1"], p["slot"], p["idx2"], p["id"]) != (q["kp1"], q["slot"], q["idx2"], q["id"]):
            return False
        for k in ("Xw", "normal", "desc"):
            if np.asarray(p[k]).tobytes() != np.asarray(q[k]).tobytes():
                return False
        if F32(p["max_dist"]).tobytes() != F32(q["max_dist"]).tobytes() or F32(p["min_dist"]).tobytes() != F32(q["min_dist"]).tobytes():
            return False
    return True
