"""ORBmatcher::Fuse restated in numpy, both overloads, with the reference's float32 / float64 widths (src/ORBmatcher.cc:477-732,
KeyFrame::GetFeaturesInArea / IsInImage src/KeyFrame.cc:529-570, MapPoint::PredictScale src/MapPoint.cc:355-369), and a toy map
(src/MapPoint.cc's AddObservation / Replace / SetBadFlag, KeyFrame::mvpMapPoints) on which the reference's sequential loops
(LocalMapping::SearchInNeighbors' first loop) and "all searches on the initial state, then an in-order walk" can be compared.
Written from reading the reference; nothing here runs on a GPU."""
import ctypes
import ctypes.util
import math

import numpy as np

F32, F64 = np.float32, np.float64
TH_LOW = 50
GRID_COLS, GRID_ROWS = 64, 48
GATES = ("cand", "depth", "image", "dist", "angle", "empty", "level", "chi2", "th_low", "accepted")


def decompose(T, sim3):
    """Rcw, tcw, Ow the overload projects with.  Sim3 (:625-629): scw is a FLOAT; every product and sum rounded on its own."""
    T = np.asarray(T, F64)
    R, t = T[:3, :3].copy(), T[:3, 3].copy()
    if sim3:
        scw = F64(F32(np.sqrt((R[0, 0] * R[0, 0] + R[0, 1] * R[0, 1]) + R[0, 2] * R[0, 2])))
        R, t = R / scw, t / scw
    Ow = np.array([((-R[0, c]) * t[0] + (-R[1, c]) * t[1]) + (-R[2, c]) * t[2] for c in range(3)], F64)
    return R, t, Ow


def decompose_longdouble(T, sim3):
    """The same in extended precision (scw still rounded to float: that is the reference's definition, not an error)."""
    T = np.asarray(T, np.longdouble)
    R, t = T[:3, :3].copy(), T[:3, 3].copy()
    if sim3:
        scw = np.longdouble(F32(np.sqrt(F64(R[0, 0] * R[0, 0] + R[0, 1] * R[0, 1] + R[0, 2] * R[0, 2]))))
        R, t = R / scw, t / scw
    return R, t, -(R.T @ t)


_LIBM = ctypes.CDLL(ctypes.util.find_library("m"))
_LIBM.logf.restype, _LIBM.logf.argtypes = ctypes.c_float, [ctypes.c_float]


def logf(v):
    """The C library's float log: what the reference calls, and what the library's PredictScale breakpoints are bisected with
    (numpy's own float32 log may differ from it in the last bit)."""
    return F32(_LIBM.logf(float(F32(v))))


def predict_scale(mf_max, dist, scale_factor, nlevels):
    ratio = F32(mf_max) / F32(dist)
    if not ratio > 0:
        return 0                                   # log(0) = -inf -> clamped to level 0
    n = math.ceil(F32(logf(ratio) / logf(scale_factor)))
    return min(max(n, 0), nlevels - 1)


def build_grid(kps, cam9):
    """KeyFrame::mGrid (Frame::AssignFeaturesToGrid, PosInGrid with round()): cell -> keypoint indices, ascending."""
    _, _, _, _, _, min_x, max_x, min_y, max_y = (F32(v) for v in cam9)
    invW, invH = F32(GRID_COLS) / F32(max_x - min_x), F32(GRID_ROWS) / F32(max_y - min_y)
    grid = {}
    for i in range(len(kps)):
        px = _round(F32(F32(kps["x"][i] - min_x) * invW))
        py = _round(F32(F32(kps["y"][i] - min_y) * invH))
        if 0 <= px < GRID_COLS and 0 <= py < GRID_ROWS:
            grid.setdefault((px, py), []).append(i)
    return grid, invW, invH


def _round(v):
    """C round(): half away from zero."""
    v = float(v)
    return int(math.floor(v + 0.5)) if v >= 0 else -int(math.floor(-v + 0.5))


def features_in_area(kps, grid, invW, invH, cam9, x, y, r):
    min_x, min_y = F32(cam9[5]), F32(cam9[7])
    x, y, r = F32(x), F32(y), F32(r)
    x0 = max(0, int(math.floor(F32(F32(x - min_x - r) * invW))))
    if x0 >= GRID_COLS:
        return []
    x1 = min(GRID_COLS - 1, int(math.ceil(F32(F32(x - min_x + r) * invW))))
    if x1 < 0:
        return []
    y0 = max(0, int(math.floor(F32(F32(y - min_y - r) * invH))))
    if y0 >= GRID_ROWS:
        return []
    y1 = min(GRID_ROWS - 1, int(math.ceil(F32(F32(y - min_y + r) * invH))))
    if y1 < 0:
        return []
    out = []
    for ix in range(x0, x1 + 1):
        for iy in range(y0, y1 + 1):
            for j in grid.get((ix, iy), ()):
                if abs(F32(kps["x"][j] - x)) < r and abs(F32(kps["y"][j] - y)) < r:
                    out.append(j)
    return out


def hamming(a, b):
    return int(np.unpackbits(np.bitwise_xor(a, b)).sum())


def fuse_search(kps, desc, uright, pts, T, cam9, sf, inv_sigma2, scale_factor, th=3.0, sim3=False, pose=None, counts=None):
    """best_idx[i], best_dist[i] of every point: the keypoint the reference reaches :597 / :718 with, or -1; bestDist, 256 for
    none.  pose: (Rcw, tcw, Ow) to project with instead of decompose(T, sim3).  counts: per-gate rejections (GATES)."""
    fx, fy, cx, cy, bf, min_x, max_x, min_y, max_y = (F32(v) for v in cam9)
    R, t, Ow = decompose(T, sim3) if pose is None else (np.asarray(p, F64) for p in pose)
    nlevels = len(sf)
    grid, invW, invH = build_grid(kps, cam9)
    n = len(pts["cand"])
    best_idx, best_dist = np.full(n, -1, np.int32), np.full(n, 256, np.int32)
    c = {g: 0 for g in GATES} if counts is None else counts
    for g in GATES:
        c.setdefault(g, 0)
    th = F32(th)
    for i in range(n):
        if not pts["cand"][i]:
            c["cand"] += 1
            continue
        P = np.asarray(pts["Xw"][i], F64)
        pc = [((R[r, 0] * P[0] + R[r, 1] * P[1]) + R[r, 2] * P[2]) + t[r] for r in range(3)]
        if pc[2] < 0.0:
            c["depth"] += 1
            continue
        with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
            invz = F32(F64(1.0) / pc[2])
            x, y = F32(pc[0] * F64(invz)), F32(pc[1] * F64(invz))
            u, v = F32(F32(fx * x) + cx), F32(F32(fy * y) + cy)
        if not (u >= min_x and u < max_x and v >= min_y and v < max_y):
            c["image"] += 1
            continue
        ur = F32(u - F32(bf * invz))
        PO = P - Ow
        dist3D = F32(np.sqrt((PO[0] * PO[0] + PO[1] * PO[1]) + PO[2] * PO[2]))
        if dist3D < F32(pts["min_dist"][i]) or dist3D > F32(pts["max_dist"][i]):
            c["dist"] += 1
            continue
        Pn = np.asarray(pts["normal"][i], F64)
        if (PO[0] * Pn[0] + PO[1] * Pn[1]) + PO[2] * Pn[2] < F64(0.5) * F64(dist3D):
            c["angle"] += 1
            continue
        lvl = predict_scale(pts["mf_max_dist"][i], dist3D, scale_factor, nlevels)
        radius = F32(th * F32(sf[lvl]))
        idxs = features_in_area(kps, grid, invW, invH, cam9, u, v, radius)
        if not idxs:
            c["empty"] += 1
            continue
        bd, bi = 256, -1
        for idx in idxs:
            lv = int(kps["octave"][idx])
            if lv < lvl - 1 or lv > lvl:
                c["level"] += 1
                continue
            if not sim3:
                ex, ey = F32(u - F32(kps["x"][idx])), F32(v - F32(kps["y"][idx]))
                e2 = F32(F32(ex * ex) + F32(ey * ey))
                limit = 5.99
                if F32(uright[idx]) >= 0:
                    er = F32(ur - F32(uright[idx]))
                    e2 = F32(e2 + F32(er * er))
                    limit = 7.8
                if F64(F32(e2 * F32(inv_sigma2[lv]))) > limit:
                    c["chi2"] += 1
                    continue
            d = hamming(pts["desc"][i], desc[idx])
            if d < bd:
                bd, bi = d, idx
        best_dist[i] = bd
        if bd <= TH_LOW:
            best_idx[i] = bi
            c["accepted"] += 1
        elif bi >= 0:
            c["th_low"] += 1
    return best_idx, best_dist


def window_run_counts(kps, pts, T, cam9, sf, scale_factor, th=3.0):
    """Grid entries per window COLUMN (one contiguous run of the device's sorted grid) over the points that reach the window:
    what a group of lanes walks at a time."""
    R, t, Ow = decompose(T, False)
    grid, invW, invH = build_grid(kps, cam9)
    fx, fy, cx, cy, _, min_x, max_x, min_y, max_y = (F32(v) for v in cam9)
    runs = []
    for i in range(len(pts["cand"])):
        P = np.asarray(pts["Xw"][i], F64)
        pc = R @ P + t
        if pc[2] <= 0:
            continue
        u, v = F32(fx * F32(pc[0] / pc[2]) + cx), F32(fy * F32(pc[1] / pc[2]) + cy)
        if not (min_x <= u < max_x and min_y <= v < max_y):
            continue
        d = F32(np.linalg.norm(P - Ow))
        r = F32(F32(th) * F32(sf[predict_scale(pts["mf_max_dist"][i], d, scale_factor, len(sf))]))
        x0, x1 = max(0, math.floor((u - min_x - r) * invW)), min(GRID_COLS - 1, math.ceil((u - min_x + r) * invW))
        y0, y1 = max(0, math.floor((v - min_y - r) * invH)), min(GRID_ROWS - 1, math.ceil((v - min_y + r) * invH))
        for ix in range(x0, x1 + 1):
            runs.append(sum(len(grid.get((ix, iy), ())) for iy in range(y0, y1 + 1)))
    return np.asarray(runs)


# ---------------------------------------------------------------------------------------------------------------- toy map
class MapPoint:
    """What Fuse touches of src/MapPoint.cc: observations, the bad flag, Replace."""

    def __init__(self, name):
        self.name, self.obs, self.bad, self.replaced = name, {}, False, None

    def isBad(self):
        return self.bad

    def Observations(self):
        return len(self.obs)

    def IsInKeyFrame(self, kf):
        return kf in self.obs

    def AddObservation(self, kf, idx):
        if kf not in self.obs:
            self.obs[kf] = idx

    def Replace(self, other):
        """MapPoint::Replace: this point goes bad, its observations move to `other` (or are erased where other is there already)."""
        if other is self:
            return
        obs, self.obs, self.bad, self.replaced = self.obs, {}, True, other
        for kf, idx in obs.items():
            if not other.IsInKeyFrame(kf):
                kf.points[idx] = other
                other.AddObservation(kf, idx)
            else:
                kf.points[idx] = None


class KeyFrame:
    def __init__(self, name, n_kp):
        self.name, self.points = name, [None] * n_kp

    def GetMapPoint(self, idx):
        return self.points[idx]

    def AddMapPoint(self, mp, idx):
        self.points[idx] = mp


def apply_fuse(kf, mp, best_idx):
    """:597-611 for one point whose search returned best_idx >= 0."""
    in_kf = kf.GetMapPoint(best_idx)
    if in_kf is not None:
        if not in_kf.isBad():
            if in_kf.Observations() > mp.Observations():
                mp.Replace(in_kf)
            else:
                in_kf.Replace(mp)
    else:
        mp.AddObservation(kf, best_idx)
        kf.AddMapPoint(mp, best_idx)


def fuse_sequential(kfs, points, search):
    """SearchInNeighbors' first loop, literally: for every target keyframe Fuse(pKF, vpMapPoints), each with its own skip tests
    and its own search(kf, i) -> best_idx at the moment the reference would run it."""
    n_fused = []
    for kf in kfs:
        n = 0
        for i, mp in enumerate(points):
            if mp is None or mp.isBad() or mp.IsInKeyFrame(kf):
                continue
            b = search(kf, i)
            if b >= 0:
                apply_fuse(kf, mp, b)
                n += 1
        n_fused.append(n)
    return n_fused


def fuse_batched_walk(kfs, points, search):
    """All searches on the initial state (cand as uploaded), then the walk: keyframes in order, points in order, the skip tests live."""
    cand = [[mp is not None and not mp.isBad() and not mp.IsInKeyFrame(kf) for mp in points] for kf in kfs]
    best = [[search(kf, i) if cand[k][i] else -1 for i in range(len(points))] for k, kf in enumerate(kfs)]
    n_fused = []
    for k, kf in enumerate(kfs):
        n = 0
        for i, mp in enumerate(points):
            if mp is None or mp.isBad() or mp.IsInKeyFrame(kf):
                continue
            if best[k][i] >= 0:
                apply_fuse(kf, mp, best[k][i])
                n += 1
        n_fused.append(n)
    return n_fused


def fuse_sim3(kf, points, search, replace):
    """The Scw overload's loop (:639-728) on one keyframe: spAlreadyFound is taken once, up front; a keypoint that holds a point
    fills vpReplacePoint instead of replacing."""
    found = {p for p in kf.points if p is not None and not p.isBad()}
    n = 0
    for i, mp in enumerate(points):
        if mp is None or mp.isBad() or mp in found:
            continue
        b = search(kf, i)
        if b < 0:
            continue
        in_kf = kf.GetMapPoint(b)
        if in_kf is not None:
            if not in_kf.isBad():
                replace[i] = in_kf
        else:
            mp.AddObservation(kf, b)
            kf.AddMapPoint(mp, b)
        n += 1
    return n


def map_state(kfs, points):
    """Everything the two procedures may differ in, by name."""
    return ([[None if p is None else p.name for p in kf.points] for kf in kfs],
            [None if p is None else (p.bad, None if p.replaced is None else p.replaced.name,
                                     sorted((kf.name, idx) for kf, idx in p.obs.items())) for p in points])
