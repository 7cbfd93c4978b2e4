"""Seeded cases for sd_debug_search_for_triangulation (tests/test_triangulation_cpu.py checks that each reaches what it claims,
tests/test_triangulation_gpu.py runs them on the device).  Everything is crafted on the host: KF2 descriptors are KF1
descriptors with k flipped bits, placed on or near the epipolar line of a known F12.

Two families.  "shape" cases: random content on an F12 computed from two poses, at the sizes where the kernel takes another
path (more than one wave of rows, a partial tile, the 512-entry tile boundary, one entry in the second tile, more rows than
one pass of the workgroup holds, empty sides, capacities that are no multiple of 64).  "unit" cases: a handful of rows with a
known answer each (`expect`: idx1 -> idx2 or -1), every rejection with a twin just on the other side of its gate.  Unit cases
use F_RECT, the F12 of a pure x translation: the epipolar line of (x1, y1) is y2 = y1 exactly (a = 0, b = 1, c = -y1, den = 1,
dsqr = (y2 - y1)^2), which makes the answers computable by hand."""
import numpy as np

import triangulation_ref as TR
from sdslam_amd.capi import KP_DTYPE
from sdslam_amd import synth

F32 = np.float32
K = (synth.FX, synth.FY, synth.CX, synth.CY)
SF, SIGMA2 = TR.scale_tables(1.2, 8)
F_RECT = np.array([[0, 0, 0], [0, 0, -1], [0, 1, 0]], np.float64)
FAR = np.array([1e6, 1e6], F32)          # an epipole no keypoint is near


def flip(desc, bits):
    """Copy of a 32-byte descriptor with the given bit positions flipped."""
    d = np.array(desc, np.uint8).copy()
    for b in bits:
        d[b >> 3] ^= np.uint8(1 << (b & 7))
    return d


def _kps(n):
    k = np.zeros(n, KP_DTYPE)
    k["size"], k["response"], k["class_id"] = 31.0, 50.0, -1
    return k


def _case(name, k1, d1, h1, u1, k2, d2, h2, u2, F12, epi, expect=None, claims=()):
    return dict(name=name, k1=k1, d1=np.ascontiguousarray(d1, np.uint8).reshape(len(k1), 32), h1=np.asarray(h1, np.uint8),
                u1=np.asarray(u1, F32), k2=k2, d2=np.ascontiguousarray(d2, np.uint8).reshape(len(k2), 32), h2=np.asarray(h2, np.uint8),
                u2=np.asarray(u2, F32), F12=np.asarray(F12, np.float64), epi=np.asarray(epi, F32), sf=SF, sigma2=SIGMA2,
                expect=expect, claims=tuple(claims))


def reference(case, check_ori, counts=None):
    c = case
    return TR.search_for_triangulation(c["k1"], c["d1"], c["h1"], c["u1"], c["k2"], c["d2"], c["h2"], c["u2"], c["F12"], c["epi"],
                                       c["sf"], c["sigma2"], check_ori, counts)


# ------------------------------------------------------------------------------------------------ shape cases
SIDEWAYS = (synth.se3_exp((0.25, 0.02, 0.01), (0.5, -1.0, 0.8)), np.eye(4))     # KF1, KF2 (Tcw); epipole far outside the image
FORWARD = (synth.se3_exp((0.01, -0.005, -0.3), (0.3, 0.2, -0.4)), np.eye(4))    # epipole inside the image


def shape_case(name, seed, n1, n2, motion=SIDEWAYS, flagged=0.5, stereo=0.0, claims=(), K=K):
    rng = np.random.default_rng(seed)
    T1, T2 = motion
    F12, epi = TR.compute_f12(T1, T2, K), TR.epipole(T1, T2, K)
    k1, k2 = _kps(n1), _kps(n2)
    k1["x"], k1["y"] = rng.uniform(20, 620, n1).astype(F32), rng.uniform(20, 460, n1).astype(F32)
    k1["angle"], k1["octave"] = rng.uniform(0, 360, n1).astype(F32), rng.integers(0, 8, n1)
    d1 = rng.integers(0, 256, (n1, 32)).astype(np.uint8)
    d2 = rng.integers(0, 256, (n2, 32)).astype(np.uint8)
    k2["x"], k2["y"] = rng.uniform(20, 620, n2).astype(F32), rng.uniform(20, 460, n2).astype(F32)
    k2["angle"], k2["octave"] = rng.uniform(0, 360, n2).astype(F32), rng.integers(0, 8, n2)
    for j in range(n2 if n1 else 0):
        i = int(rng.integers(n1))
        a, b, c, den = [float(v) for v in TR.epipolar_line(k1["x"][i], k1["y"][i], F12)]
        # a point of the line (in the forward case half of them within a few pixels of the epipole), moved off it by t pixels
        x = float(epi[0]) + rng.uniform(-12, 12) if (motion is FORWARD and j % 2) else rng.uniform(20, 620)
        y = -(a * x + c) / b if abs(b) >= abs(a) else rng.uniform(20, 460)
        if abs(b) < abs(a):
            x = -(b * y + c) / a
        t = rng.uniform(-1, 1) if rng.random() < 0.7 else rng.uniform(-6, 6)
        t *= float(np.sqrt(SIGMA2[k2["octave"][j]]))
        k2["x"][j], k2["y"][j] = x + t * a / np.sqrt(den), y + t * b / np.sqrt(den)
        nflip = int(rng.integers(0, 30)) if rng.random() < 0.8 else int(rng.integers(45, 62))
        d2[j] = flip(d1[i], rng.choice(256, nflip, replace=False))
        k2["angle"][j] = F32((k1["angle"][i] + rng.choice([0.0, 0.0, 0.0, 40.0, 95.0, 200.0, 310.0]) + rng.uniform(-3, 3)) % 360.0)
    h1, h2 = (rng.random(n1) < flagged).astype(np.uint8), (rng.random(n2) < flagged).astype(np.uint8)
    u1 = np.where(rng.random(n1) < stereo, k1["x"] - F32(5), F32(-1)).astype(F32)
    u2 = np.where(rng.random(n2) < stereo, k2["x"] - F32(5), F32(-1)).astype(F32)
    return _case(name, k1, d1, h1, u1, k2, d2, h2, u2, F12, epi, claims=claims)


# ------------------------------------------------------------------------------------------------ unit cases
class _Unit:
    """Rows and candidates on F_RECT; descriptors of unrelated keypoints are ~128 bits apart."""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.rows, self.cands, self.expect = [], [], {}

    def desc(self):
        return self.rng.integers(0, 256, 32).astype(np.uint8)

    def row(self, y, desc, x=100.0, has=0, uright=-1.0, angle=0.0):
        self.rows.append(dict(x=x, y=y, desc=desc, has=has, ur=uright, angle=angle))
        return len(self.rows) - 1

    def cand(self, x, y, desc, octave=0, has=0, uright=-1.0, angle=0.0):
        self.cands.append(dict(x=x, y=y, desc=desc, octave=octave, has=has, ur=uright, angle=angle))
        return len(self.cands) - 1

    def filler(self, n):
        """Candidates that match no row: far from every line used (rows sit at y < 1000)."""
        for _ in range(n):
            self.cand(float(self.rng.uniform(0, 640)), 5000.0, self.desc(), octave=int(self.rng.integers(0, 8)))

    def build(self, name, F12=F_RECT, epi=FAR, claims=()):
        k1, k2 = _kps(len(self.rows)), _kps(len(self.cands))
        for k, items in ((k1, self.rows), (k2, self.cands)):
            k["x"], k["y"] = [F32(i["x"]) for i in items], [F32(i["y"]) for i in items]
            k["angle"] = [F32(i["angle"]) for i in items]
        k2["octave"] = [c["octave"] for c in self.cands]
        return _case(name, k1, np.array([r["desc"] for r in self.rows]), [r["has"] for r in self.rows], [r["ur"] for r in self.rows],
                     k2, np.array([c["desc"] for c in self.cands]), [c["has"] for c in self.cands], [c["ur"] for c in self.cands],
                     F12, epi, expect=dict(self.expect), claims=claims)


def unit_ties():
    u = _Unit(101)
    # row 0: two eligible candidates at the minimum distance 10 -> the larger idx2; a closer one is flagged
    d = u.desc()
    r = u.row(50.0, d)
    u.filler(2)
    u.cand(200.0, 50.0, flip(d, range(0, 10)))
    u.cand(210.0, 50.0, flip(d, range(0, 14)))
    last = u.cand(220.0, 50.0, flip(d, range(20, 30)))
    u.cand(230.0, 50.0, flip(d, range(0, 3)), has=1)
    u.expect[r] = last
    # row 1: the same tie, but the larger index lies 5 px off the line -> the smaller one
    d = u.desc()
    r = u.row(80.0, d)
    first = u.cand(200.0, 80.0, flip(d, range(0, 10)))
    u.cand(220.0, 85.0, flip(d, range(20, 30)))
    u.expect[r] = first
    # row 2 / 3: dist = 50 matches, dist = 51 does not
    d = u.desc()
    r = u.row(110.0, d)
    u.expect[r] = u.cand(300.0, 110.0, flip(d, range(50)))
    d = u.desc()
    r = u.row(140.0, d)
    u.cand(300.0, 140.0, flip(d, range(51)))
    u.expect[r] = -1
    # row 4: holds a map point -> skipped although a perfect candidate exists;  row 5: its best candidate holds one -> second best
    d = u.desc()
    r = u.row(170.0, d, has=1)
    u.cand(300.0, 170.0, d.copy())
    u.expect[r] = -1
    d = u.desc()
    r = u.row(200.0, d)
    u.cand(300.0, 200.0, d.copy(), has=1)
    u.expect[r] = u.cand(310.0, 200.0, flip(d, range(7)))
    u.filler(3)
    return u.build("unit_ties", claims=("cand_has_point", "row_has_point", "epipolar", "dist_gt_50", "dist_gt_best"))


def ulp_pair(octave):
    """(b_lo, y_lo, b_hi, y_hi): a line 0 x + b y + 0 = 0 and a keypoint height whose dsqr = fl(fl(y * y) / fl(b * b)) is the
    largest float below 3.84 * sigma2[octave] (passes) / the smallest float not below it (fails)."""
    T = np.float64(3.84) * np.float64(SIGMA2[octave])
    hi = F32(T) if np.float64(F32(T)) >= T else np.nextafter(F32(T), F32(np.inf))
    lo = np.nextafter(hi, F32(0))
    assert np.float64(lo) < T <= np.float64(hi)
    y0 = F32(np.sqrt(T))
    ys = [y0]
    for _ in range(40):
        ys = [np.nextafter(ys[0], F32(0))] + ys + [np.nextafter(ys[-1], F32(np.inf))]
    found = {}
    for k in range(64):
        b = F32(1.0 + k * 2.0 ** -23)
        den = F32(b * b)
        for y in ys:
            num = F32(b * y)
            dsqr = F32(F32(num * num) / den)
            for tag, want in (("lo", lo), ("hi", hi)):
                if dsqr == want and tag not in found:
                    found[tag] = (k, float(y))
    assert len(found) == 2, (octave, found)
    return found["lo"], found["hi"], float(lo), float(hi)


F_ULP = np.array([[0, 2.0 ** -23, 0], [0, 0, 0], [0, 1, 0]], np.float64)   # a = 0, b = 1 + x1 * 2^-23, c = 0


def unit_ulp():
    """dsqr one float ulp either side of 3.84 * sigma2, octaves 0, 3 and 7; row x1 = k selects b = 1 + k * 2^-23."""
    u = _Unit(102)
    u.filler(2)
    u.ulp = {}
    for octave in (0, 3, 7):
        (k_lo, y_lo), (k_hi, y_hi), lo, hi = ulp_pair(octave)
        d = u.desc()
        r = u.row(0.0, d, x=float(k_lo))
        u.expect[r] = u.cand(300.0, y_lo, flip(d, range(4)), octave=octave)
        d = u.desc()
        r2 = u.row(0.0, d, x=float(k_hi))
        c2 = u.cand(300.0, y_hi, flip(d, range(4)), octave=octave)
        u.expect[r2] = -1
        u.ulp[octave] = (r, u.expect[r], lo, r2, c2, hi)
    c = u.build("unit_ulp", F12=F_ULP, claims=("epipolar",))
    c["ulp"] = u.ulp
    return c


def unit_den(zero):
    """A zero F12 column pair makes a = b = 0: den == 0 rejects every candidate, identical descriptors included."""
    u = _Unit(103)
    for i in range(6):
        d = u.desc()
        r = u.row(40.0 + 10 * i, d)
        c = u.cand(100.0 + i, 40.0 + 10 * i, d.copy())
        u.expect[r] = -1 if zero else c
    F = np.array([[0, 0, 1], [0, 0, 1], [0, 0, 1]], np.float64) if zero else F_RECT
    return u.build("unit_den_zero" if zero else "unit_den_nonzero", F12=F, claims=("den_zero",) if zero else ())


def unit_epipole():
    """Epipole (300, 200): a mono candidate closer than sqrt(100 * mvScaleFactors[octave]) is rejected for a mono row only."""
    u = _Unit(104)
    epi = np.array([300.0, 200.0], F32)

    def pair(cx, octave, row_ur, cand_ur, ok):
        d = u.desc()
        r = u.row(200.0, d, uright=row_ur)
        c = u.cand(cx, 200.0, flip(d, range(5)), octave=octave, uright=cand_ur)
        u.expect[r] = c if ok else -1
    pair(305.0, 0, -1.0, -1.0, False)      # 25 < 100
    pair(305.0, 0, 90.0, -1.0, True)       # the row is stereo
    pair(305.0, 0, -1.0, 290.0, True)      # the candidate is stereo
    pair(305.0, 0, 0.0, -1.0, True)        # mvuRight == 0 is stereo (>= 0)
    pair(310.0, 0, -1.0, -1.0, True)       # 100 < 100 is false
    pair(309.5, 0, -1.0, -1.0, False)      # 90.25 < 100
    pair(311.0, 2, -1.0, -1.0, False)      # 121 < 100 * 1.44
    pair(312.5, 2, -1.0, -1.0, True)       # 156.25
    u.filler(4)
    return u.build("unit_epipole", epi=epi, claims=("epipole",))


def unit_flags(which):
    """all rows flagged / all candidates flagged / none flagged, identical descriptors on the line."""
    u = _Unit(105)
    for i in range(70):
        d = u.desc()
        r = u.row(20.0 + 5 * i, d, has=int(which == "rows"))
        c = u.cand(50.0 + i, 20.0 + 5 * i, flip(d, range(i % 9)), has=int(which == "cands"))
        u.expect[r] = c if which == "none" else -1
    claims = {"rows": ("row_has_point",), "cands": ("cand_has_point",), "none": ()}[which]
    return u.build("unit_flags_" + which, claims=claims)


def unit_far_epipole():
    """C2z tiny but non-zero: |ex| is huge, (ex - x2)^2 overflows to +inf in float and is not < the radius -> nothing rejected."""
    T2 = np.eye(4)
    T1 = np.eye(4)
    T1[:3, 3] = (-0.3, 0.1, -1e-30)          # Cw = (0.3, -0.1, 1e-30) = C2
    epi = TR.epipole(T1, T2, K)
    u = _Unit(106)
    for i in range(8):
        d = u.desc()
        r = u.row(30.0 + 20 * i, d)
        u.expect[r] = u.cand(100.0 + 50 * i, 30.0 + 20 * i, flip(d, range(i)))
    c = u.build("unit_far_epipole", epi=epi)
    c["poses"] = (T1, T2)
    return c


def unit_orientation():
    """Matches in five histogram bins of sizes 6, 5, 4, 2, 1: with check_ori the two smallest bins go."""
    u = _Unit(107)
    u.by_bin = {}
    y = 20.0
    for rot, n in ((0.0, 6), (60.0, 5), (120.0, 4), (180.0, 2), (300.0, 1)):
        for _ in range(n):
            d = u.desc()
            r = u.row(y, d, angle=rot)
            u.expect[r] = u.cand(200.0, y, flip(d, range(3)), angle=0.0)
            u.by_bin.setdefault(int(rot), []).append(r)
            y += 7.0
    c = u.build("unit_orientation")
    c["by_bin"] = u.by_bin
    return c


def all_cases():
    cases = [
        shape_case("shape_70x40", 1, 70, 40, claims=("row_has_point", "cand_has_point", "epipolar", "dist_gt_50")),
        shape_case("shape_5x600", 2, 5, 600, flagged=0.3, claims=("cand_has_point", "epipolar", "dist_gt_50")),
        shape_case("shape_300x513", 3, 300, 513, claims=("row_has_point", "cand_has_point", "epipolar", "dist_gt_50", "dist_gt_best")),
        shape_case("shape_0x50", 4, 0, 50),
        shape_case("shape_50x0", 5, 50, 0),
        shape_case("shape_130x100", 6, 130, 100, stereo=0.4, claims=("epipolar",)),
        shape_case("shape_600x70_unflagged", 7, 600, 70, flagged=0.0, claims=("epipolar", "dist_gt_50")),   # rows beyond one pass of 512
        shape_case("shape_forward_90x200", 8, 90, 200, motion=FORWARD, flagged=0.2, stereo=0.3, claims=("epipole", "epipolar")),
        unit_ties(), unit_ulp(), unit_den(True), unit_den(False), unit_epipole(), unit_flags("rows"), unit_flags("cands"),
        unit_flags("none"), unit_far_epipole(), unit_orientation(),
    ]
    assert len({c["name"] for c in cases}) == len(cases)
    return cases


_CACHE = {}


def cases_with_reference():
    """[(case, {check_ori: (nmatches, matches12, counts)})], computed once per process."""
    if not _CACHE:
        out = []
        for c in all_cases():
            res = {}
            for ori in (0, 1):
                counts = {}
                n, m = reference(c, ori, counts)
                m.setflags(write=False)
                res[ori] = (n, m, counts)
            out.append((c, res))
        _CACHE["all"] = out
    return _CACHE["all"]
