"""Crafted cases for sd_debug_fuse (ORBmatcher::Fuse, both overloads): unit cases whose answers are worked out by hand, each
with a twin just on the other side of its gate, and shape cases at the sizes where k_fuse takes another path.  A case is run
through both overloads: the keyframe-pose one with T, the Sim3 one with Scw = [s R | s t] (s = case["scale"]; 2 in the unit
cases, so the float scw and the divisions are exact and the same hand answers hold).

The unit camera is fx = fy = 512, cx = 320, cy = 240, bf = 40, image 640 x 480, identity pose and points at depth 2: then invz,
x, y, u, v and ur = u - 20 are exact in float, and a point that should project to (u, v) does so to the bit."""
import numpy as np

import fuse_ref as FR
from sdslam_amd.capi import KP_DTYPE
from sdslam_amd import synth

F32 = np.float32
NLEVELS, SCALE = 8, 1.2
SF = np.array([F32(1.0)] * NLEVELS, F32)
for _l in range(1, NLEVELS):
    SF[_l] = F32(SF[_l - 1] * F32(SCALE))                  # ORBextractor's mvScaleFactor recurrence
INV_SIGMA2 = (F32(1.0) / (SF * SF)).astype(F32)
CAM_UNIT = np.array([512, 512, 320, 240, 40, 0, 640, 0, 480], F32)
CAM_SYNTH = np.array([synth.FX, synth.FY, synth.CX, synth.CY, 40, 0, 640, 0, 480], F32)
TH_LOW = 50


def flip(desc, bits):
    out = np.array(desc, np.uint8).copy()
    for b in bits:
        out[b // 8] ^= np.uint8(1 << (b % 8))
    return out


def ratio_for(level):
    """mfMaxDistance / dist3D that PredictScale maps to `level`: 1.2^(level - 0.5), clear of every breakpoint."""
    return SCALE ** (level - 0.5)


class Builder:
    """A keyframe at the identity pose (unit camera) and points at depth 2, added one by one."""

    def __init__(self, seed, cam=CAM_UNIT):
        self.cam = cam
        self.rng = np.random.default_rng(seed)
        self.k, self.d, self.u = [], [], []
        self.p = {k: [] for k in ("cand", "Xw", "normal", "min_dist", "max_dist", "mf_max_dist", "desc")}
        self.expect, self.expect_sim3 = {}, {}

    def kp(self, x, y, octave, uright=-1.0):
        self.k.append((x, y, 31.0, 0.0, 1.0, octave, -1))
        self.d.append(self.rng.integers(0, 256, 32).astype(np.uint8))
        self.u.append(uright)
        return len(self.k) - 1

    def pt(self, u, v, level, desc, want, want_sim3=None, z=2.0, normal=None, min_dist=None, max_dist=None, cand=1):
        fx, fy, cx, cy = (float(c) for c in self.cam[:4])
        X = np.array([(u - cx) / fx * z, (v - cy) / fy * z, z])
        dist = float(F32(np.linalg.norm(X * np.sign(z))))
        self.p["cand"].append(cand)
        self.p["Xw"].append(X)
        self.p["normal"].append(X / np.linalg.norm(X) if normal is None else normal)
        self.p["min_dist"].append(0.01 if min_dist is None else min_dist)
        self.p["max_dist"].append(1e3 if max_dist is None else max_dist)
        self.p["mf_max_dist"].append(dist * ratio_for(level))
        self.p["desc"].append(desc)
        i = len(self.p["cand"]) - 1
        self.expect[i] = want
        self.expect_sim3[i] = want if want_sim3 is None else want_sim3
        return i

    def case(self, name, claims, th=3.0):
        kps = np.array(self.k, KP_DTYPE) if self.k else np.zeros(0, KP_DTYPE)
        pts = dict(cand=np.array(self.p["cand"], np.uint8), Xw=np.array(self.p["Xw"], np.float64).reshape(-1, 3),
                   normal=np.array(self.p["normal"], np.float64).reshape(-1, 3), min_dist=np.array(self.p["min_dist"], F32),
                   max_dist=np.array(self.p["max_dist"], F32), mf_max_dist=np.array(self.p["mf_max_dist"], F32),
                   desc=np.array(self.p["desc"], np.uint8).reshape(-1, 32))
        return dict(name=name, kps=kps, desc=np.array(self.d, np.uint8).reshape(-1, 32), uright=np.array(self.u, F32), pts=pts,
                    T=np.eye(4), scale=2.0, cam=self.cam, th=th, kp_cap=None, max_points=None, expect=self.expect,
                    expect_sim3=self.expect_sim3, claims=tuple(claims))


def unit_depth_and_cand():
    b = Builder(1)
    k = b.kp(320, 240, 2)
    b.pt(320, 240, 2, b.d[k], k)
    b.pt(320, 240, 2, b.d[k], -1, z=-2.0)                          # behind the camera
    b.pt(320, 240, 2, b.d[k], -1, cand=0)                          # bad / already in the keyframe at upload time
    return b.case("unit_depth_and_cand", ("depth", "cand"))


def unit_image_edges(cam=None):
    """KeyFrame::IsInImage is >= min && < max: u == 640 and v == 480 are OUTSIDE (Frame::isInFrustum keeps them), 0 is inside.
    Level 7 windows (radius 10.7) reach the nearest keypoints the grid holds (x < 635, y < 475: PosInGrid rounds).
    With a camera (9 floats: K, bf, bounds) the same eight points sit a hair (0.01 px: the projection of such a camera is not
    exact in float, its error is some 1e-4 px) inside and outside each of its four bounds."""
    if cam is not None:
        return _image_edges_at(np.asarray(cam, F32))
    b = Builder(2)
    right, left, bottom, top = b.kp(633, 100, 7), b.kp(3, 100, 7), b.kp(100, 474, 7), b.kp(100, 3, 7)
    outside = b.kp(637, 100, 7)                                    # PosInGrid = 64: AssignFeaturesToGrid skips it
    b.d[outside] = flip(b.d[right], [0, 1])
    b.pt(640.0, 100, 7, b.d[right], -1)
    b.pt(639.5, 100, 7, b.d[outside], right)                       # the closer keypoint, with this very descriptor, is not in the grid
    b.pt(0.0, 100, 7, b.d[left], left)
    b.pt(-0.5, 100, 7, b.d[left], -1)
    b.pt(100, 480.0, 7, b.d[bottom], -1)
    b.pt(100, 479.5, 7, b.d[bottom], bottom)
    b.pt(100, 0.0, 7, b.d[top], top)
    b.pt(100, -0.5, 7, b.d[top], -1)
    c = b.case("unit_image_edges", ("image",))
    c["outside"] = outside
    return c


def _image_edges_at(cam, hair=0.01):
    x0, x1, y0, y1 = (float(c) for c in cam[5:9])
    b = Builder(2, cam)
    right, left, bottom, top = b.kp(x1 - 7.0, 100, 7), b.kp(x0 + 3.0, 100, 7), b.kp(100, y1 - 6.0, 7), b.kp(100, y0 + 3.0, 7)
    b.pt(x1 + hair, 100, 7, b.d[right], -1)
    b.pt(x1 - hair, 100, 7, b.d[right], right)
    b.pt(x0 + hair, 100, 7, b.d[left], left)
    b.pt(x0 - hair, 100, 7, b.d[left], -1)
    b.pt(100, y1 + hair, 7, b.d[bottom], -1)
    b.pt(100, y1 - hair, 7, b.d[bottom], bottom)
    b.pt(100, y0 + hair, 7, b.d[top], top)
    b.pt(100, y0 - hair, 7, b.d[top], -1)
    return b.case("unit_image_edges_at_bounds", ("image",))


def unit_distance_and_angle():
    b = Builder(3)
    k = b.kp(320, 240, 2)
    two, up, down = F32(2.0), np.nextafter(F32(2.0), F32(3.0)), np.nextafter(F32(2.0), F32(1.0))
    b.pt(320, 240, 2, b.d[k], k, min_dist=two)                     # dist3D == minDistance: `<` keeps it
    b.pt(320, 240, 2, b.d[k], -1, min_dist=up)
    b.pt(320, 240, 2, b.d[k], k, max_dist=two)
    b.pt(320, 240, 2, b.d[k], -1, max_dist=down)
    b.pt(320, 240, 2, b.d[k], k, normal=np.array([0, 0, 0.5]))     # PO.Pn == 0.5 * dist3D == 1.0: `<` keeps it
    b.pt(320, 240, 2, b.d[k], -1, normal=np.array([0, 0, np.nextafter(0.5, 0.0)]))
    return b.case("unit_distance_and_angle", ("dist", "angle"))


def unit_levels():
    b = Builder(4)
    k0, k7, k6 = b.kp(50, 50, 0), b.kp(150, 50, 7), b.kp(250, 50, 6)
    b.pt(50, 50, 0, b.d[k0], k0)                                   # predicted level 0: the window [-1, 0]
    b.pt(150, 50, 7, b.d[k7], k7)                                  # predicted level nlevels - 1
    b.pt(250, 50, 7, b.d[k6], k6)
    for j, (octave, ok) in enumerate(((1, False), (2, True), (3, True), (4, False))):   # predicted level 3
        k = b.kp(50 + 100 * j, 200, octave)
        b.pt(50 + 100 * j, 200, 3, b.d[k], k if ok else -1)
    k = b.kp(500, 400, 0)
    b.pt(500, 400, -3, b.d[k], k)                                  # ratio far below 1: clamped to level 0
    k = b.kp(500, 300, 7)
    b.pt(500, 300, 12, b.d[k], k)                                  # far above: clamped to nlevels - 1
    return b.case("unit_levels", ("level",))


def unit_chi_square():
    """Level 0 (invSigma2 = 1), keypoint 2.5 px beside the projection: e2 = 6.25 > 5.99 for a mono keypoint; a stereo one adds
    er^2 and is held to 7.8.  ur = u - bf * invz = u - 20."""
    b = Builder(5)
    rows = ((2.25, -1.0, None, True), (2.5, -1.0, None, False),           # mono: 5.0625 / 6.25 against 5.99
            (2.5, None, 1.0, True), (2.5, None, 1.5, False))             # stereo: 6.25 + 1 / 6.25 + 2.25 against 7.8
    for j, (dx, ur_abs, er, ok) in enumerate(rows):
        u = 100.0 + 60 * j
        k = b.kp(u + dx, 100, 0, uright=ur_abs if er is None else (u - 20.0) + er)
        b.pt(u, 100, 0, b.d[k], k if ok else -1, want_sim3=k)              # the Sim3 overload has no chi-square gate
    k = b.kp(21 + 2.5, 300, 0, uright=0.0)                                 # mvuRight == 0 is stereo: er = (21 - 20) - 0 = 1 -> 7.25
    b.pt(21, 300, 0, b.d[k], k)
    k = b.kp(21 + 2.5, 400, 0, uright=-1.0)                                # the same geometry, mono: 6.25 > 5.99
    b.pt(21, 400, 0, b.d[k], -1, want_sim3=k)
    return b.case("unit_chi_square", ("chi2",))


def unit_th_low_and_ties():
    b = Builder(6)
    k = b.kp(50, 50, 3)
    b.pt(50, 50, 3, flip(b.d[k], range(50)), k)                    # distance 50
    b.pt(50, 50, 3, flip(b.d[k], range(51)), -1)                   # distance 51
    # equal distances in two cells: the cell walked first wins, although its keypoint has the LARGER index (radius 5.18;
    # 2 px off keeps the chi-square at 4 / 1.728^2 = 1.34)
    late = b.kp(98, 100, 3)                                        # cell x = round(9.8) = 10
    early = b.kp(94, 100, 3)                                       # cell x = round(9.4) = 9
    base = b.rng.integers(0, 256, 32).astype(np.uint8)
    b.d[late], b.d[early] = flip(base, [0, 1, 2]), flip(base, [3, 4, 5])
    b.pt(96, 100, 3, base, early)
    # ... and within one cell the smaller index
    first, second = b.kp(298, 300, 3), b.kp(302, 300, 3)           # both in cell x = 30
    base2 = b.rng.integers(0, 256, 32).astype(np.uint8)
    b.d[first], b.d[second] = flip(base2, [10, 11]), flip(base2, [12, 13])
    b.pt(300, 300, 3, base2, first)
    # a strictly smaller distance later in the order still wins
    far, near = b.kp(396, 300, 3), b.kp(404, 300, 3)
    base3 = b.rng.integers(0, 256, 32).astype(np.uint8)
    b.d[far], b.d[near] = flip(base3, [1, 2, 3]), flip(base3, [4])
    b.pt(400, 300, 3, base3, near)
    c = b.case("unit_th_low_and_ties", ("th_low",))
    c["ties"] = dict(early=early, late=late, first=first, second=second)
    return c


def shape_case(name, seed, n_kp, n_pts, kp_cap=None, max_points=None, th=3.0, scale=1.7, crowd=0, stereo=0.3, claims=(), cam=None):
    """Random keyframe (keypoints up to the image border, so some lie outside the grid) at a random pose; the first points see
    keypoints (descriptor distances on both sides of TH_LOW, predicted levels around the keypoint's octave), the rest miss."""
    rng = np.random.default_rng(seed)
    T = synth.se3_exp(rng.uniform(-0.2, 0.2, 3), rng.uniform(-8, 8, 3))
    kps = np.zeros(n_kp, KP_DTYPE)
    kps["x"], kps["y"] = rng.uniform(0, 640, n_kp).astype(F32), rng.uniform(0, 480, n_kp).astype(F32)
    if crowd:                                                       # many keypoints in one grid cell: more than a group's lanes
        kps["x"][:crowd], kps["y"][:crowd] = 200 + rng.uniform(-1, 1, crowd), 200 + rng.uniform(-1, 1, crowd)
    kps["octave"] = rng.choice(NLEVELS, n_kp, p=np.array([24, 20, 16, 13, 10, 8, 5, 4]) / 100.0)
    kps["size"], kps["angle"], kps["response"], kps["class_id"] = 31, rng.uniform(0, 360, n_kp), 1, -1
    desc = rng.integers(0, 256, (n_kp, 32)).astype(np.uint8)
    if crowd:
        for j in range(1, crowd):                                   # near-duplicates: the order decides
            desc[j] = flip(desc[0], rng.integers(0, 256, rng.integers(0, 3)))
    uright = np.where(rng.random(n_kp) < stereo, rng.choice([0.0, 1.0], n_kp) * (kps["x"] - 8.0), -1.0).astype(F32)
    R, t = T[:3, :3], T[:3, 3]
    Ow = -R.T @ t
    cam = CAM_SYNTH if cam is None else np.asarray(cam, F32)
    pts = {k: [] for k in ("cand", "Xw", "normal", "min_dist", "max_dist", "mf_max_dist", "desc")}
    for i in range(n_pts):
        seen = n_kp > 0 and rng.random() < 0.8
        j = int(rng.integers(0, n_kp)) if seen else -1
        if crowd and i < 4:
            j = 0
        ux, vy = (kps["x"][j] + rng.normal(0, 0.7), kps["y"][j] + rng.normal(0, 0.7)) if seen else (rng.uniform(-60, 700), rng.uniform(-60, 540))
        z = rng.uniform(1.0, 5.0) * (-1 if rng.random() < 0.03 else 1)
        Xc = np.array([(ux - cam[2]) / cam[0] * z, (vy - cam[3]) / cam[1] * z, z])
        Xw = R.T @ (Xc - t)
        d = np.linalg.norm(Xw - Ow)
        lvl = (int(kps["octave"][j]) if seen else int(rng.integers(0, NLEVELS))) + int(rng.choice([0, 0, 0, 1, -1, 2]))
        mf = d * SCALE ** (lvl - rng.uniform(0.1, 0.9))
        nrm = (Xw - Ow) / d + rng.normal(size=3) * rng.choice([0.2, 1.5])
        pts["cand"].append(rng.random() > 0.1)
        pts["Xw"].append(Xw)
        pts["normal"].append(nrm / np.linalg.norm(nrm))
        pts["min_dist"].append(0.8 * mf / SCALE ** (NLEVELS - 1) if rng.random() > 0.05 else 1.01 * d)
        pts["max_dist"].append(1.2 * mf if rng.random() > 0.05 else 0.99 * d)
        pts["mf_max_dist"].append(mf)
        pts["desc"].append(flip(desc[j], rng.integers(0, 256, rng.choice([3, 10, 40, 49, 52, 70]))) if seen
                           else rng.integers(0, 256, 32).astype(np.uint8))
    pts = dict(cand=np.array(pts["cand"], np.uint8), Xw=np.array(pts["Xw"], np.float64).reshape(-1, 3),
               normal=np.array(pts["normal"], np.float64).reshape(-1, 3), min_dist=np.array(pts["min_dist"], F32),
               max_dist=np.array(pts["max_dist"], F32), mf_max_dist=np.array(pts["mf_max_dist"], F32),
               desc=np.array(pts["desc"], np.uint8).reshape(-1, 32))
    return dict(name=name, kps=kps, desc=desc, uright=uright, pts=pts, T=T, scale=scale, cam=cam, th=th, kp_cap=kp_cap,
                max_points=max_points, expect=None, expect_sim3=None, claims=tuple(claims))


POINTS_PER_PASS = 64      # k_fuse: 8 waves x 8 groups of 8 lanes


def all_cases():
    return [unit_depth_and_cand(), unit_image_edges(), unit_distance_and_angle(), unit_levels(), unit_chi_square(), unit_th_low_and_ties(),
            shape_case("shape_kp0", 10, 0, 30), shape_case("shape_kp1", 11, 1, 30), shape_case("shape_kp63", 12, 63, 40),
            shape_case("shape_kp64", 13, 64, 40), shape_case("shape_kp65", 14, 65, 40),
            shape_case("shape_pts0", 15, 80, 0), shape_case("shape_pts1", 16, 80, 1),
            shape_case("shape_one_more_than_a_pass", 17, 300, POINTS_PER_PASS + 1, claims=("empty", "dist", "angle", "depth", "image")),
            shape_case("shape_crowded_cell", 18, 120, 40, crowd=20),
            shape_case("shape_all_cells", 19, 200, 12, th=700.0),
            shape_case("shape_odd_capacities", 20, 90, 66, kp_cap=100, max_points=70, claims=("level", "chi2", "th_low", "cand")),
            shape_case("shape_sim3_small_scale", 21, 150, 80, scale=0.37),
            shape_case("shape_2048x2048", 22, 2048, 2048)]


def reference(case, sim3, counts=None):
    T = case["T"].copy()
    if sim3:
        T[:3, :] *= case["scale"]
    return FR.fuse_search(case["kps"], case["desc"], case["uright"], case["pts"], T, case["cam"], SF, INV_SIGMA2, SCALE, case["th"],
                          bool(sim3), counts=counts), T


_CACHE = {}


def cases_with_reference():
    """[(case, {sim3: (best_idx, best_dist, counts, T)})], computed once."""
    if "all" not in _CACHE:
        out = []
        for c in all_cases():
            res = {}
            for sim3 in (0, 1):
                counts = {}
                (bi, bd), T = reference(c, sim3, counts)
                res[sim3] = (bi, bd, counts, T)
            out.append((c, res))
        _CACHE["all"] = out
    return _CACHE["all"]
