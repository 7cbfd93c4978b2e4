"""Crafted cases for the three tracking matchers -- SearchByProjection(Frame, Frame) (k_match and its split form),
the TrackLocalMap search (k_match_local) and SearchByPoints (k_search_points): unit cases whose answers are worked out by hand,
each with a twin on the other side of its gate, and two shape cases (`crowd`, `sparse`).  The current frame's keypoints and
descriptors are planted with ORBextractor.set_keypoints; tests/test_match_cases_cpu.py proves on the host that every case gives
its hand answer and sits on the boundary it claims, tests/test_match_cases_gpu.py runs them on the device.

The unit camera is the one of tests/fuse_cases.py: fx = fy = 512, cx = 320, cy = 240, image 640 x 480, identity poses and points
at depth 2, so invz = 0.5, u = 256 X + 320 and v = 256 Y + 240 are exact in float for integer and half-integer pixels.  Keypoints
sit where round((x - minX) * invW) is clear of .5 (x mod 10 != 5), never on it.

A projection-search point says which keypoint it takes (`want`) and whether the rotation check cuts it; a case's match vector
and count follow by walking the points in order (a later point overwrites, the count keeps both), as the reference does."""
import numpy as np

from fuse_cases import F32, NLEVELS, SCALE, SF, flip, ratio_for
from sdslam_amd.capi import KP_DTYPE

K = (512.0, 512.0, 320.0, 240.0)
BOUNDS = (0.0, 640.0, 0.0, 480.0)
BF = 40.0
MB = BF / K[0]                                  # 0.078125, exact
TH = 8.0                                        # SearchByProjection(F, F): the level-0 radius is exactly 8
TH_HIGH, TH_LOW = 100, 50
FACTOR = F32(1.0) / F32(30)                     # the reference's histogram factor (1 / HISTO_LENGTH, not 360 / HISTO_LENGTH)
LOG_SF = np.log(F32(SCALE))
# rot with rot * FACTOR (float32) just below / on / just above 3.5: consecutive floats
ROT_BELOW, ROT_ON, ROT_ABOVE = F32(104.99998474121094), F32(104.99999237060547), F32(105.0)
assert np.nextafter(ROT_BELOW, F32(200)) == ROT_ON and np.nextafter(ROT_ON, F32(200)) == ROT_ABOVE


def up(x, steps=1):
    x = F32(x)
    for _ in range(steps):
        x = np.nextafter(x, F32(np.inf))
    return x


def down(x, steps=1):
    x = F32(x)
    for _ in range(steps):
        x = np.nextafter(x, F32(-np.inf))
    return x


def rot_bin(rot):
    """The bin the reference puts a float32 angle difference in (C round(): half away from zero)"""
    rot = F32(rot)
    if rot < 0:
        rot = F32(rot + F32(360.0))
    b = int(np.floor(np.float64(F32(rot * FACTOR)) + 0.5))
    return 0 if b == 30 else b


class Builder:
    """Keypoints of the current frame and points (last-frame map points or local map points) added one by one."""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.k, self.d, self.ur, self.claimed = [], [], [], []
        self.p = []

    def desc(self):
        return self.rng.integers(0, 256, 32).astype(np.uint8)

    def kp(self, x, y, octave, desc=None, angle=0.0, uright=-1.0, claimed=0):
        self.k.append((x, y, 31.0, angle, 1.0, octave, -1))
        self.d.append(self.desc() if desc is None else np.array(desc, np.uint8))
        self.ur.append(uright)
        self.claimed.append(claimed)
        return len(self.k) - 1

    def pt(self, u, v, level, desc, want, angle=0.0, obs=1, valid=1, z=2.0, xn=None, yn=None, dz=0.0, cut=False, normal=None,
           min_dist=None, max_dist=None, predict=None, in_view=None):
        """A point that projects to (u, v) at depth z; xn / yn: its camera-frame X / Y given directly (a float32 value, for
        projections one step outside a bound); dz: added to its world Z (the pose takes it off again).  level: the last-frame
        octave, and the level PredictScale is to give (predict: another mfMaxDistance / dist exponent).  want: keypoint index
        or -1, or {th: ...} for the local-map search; in_view: isInFrustum's answer (default: want >= 0 for some th)."""
        X = np.array([(u - K[2]) / K[0] * z if xn is None else float(xn), (v - K[3]) / K[1] * z if yn is None else float(yn), z])
        dist = F32(np.sqrt((X[0] * X[0] + X[1] * X[1]) + X[2] * X[2]))
        self.p.append(dict(valid=valid, cand=valid, Xw=X + np.array([0.0, 0.0, dz]), desc=np.array(desc, np.uint8), octave=level, angle=angle,
                           obs=obs, normal=X / np.linalg.norm(X) if normal is None else np.asarray(normal, np.float64),
                           min_dist=0.01 if min_dist is None else min_dist, max_dist=1e3 if max_dist is None else max_dist,
                           mf_max_dist=F32(dist * ratio_for(level if predict is None else predict)), want=want, cut=cut, in_view=in_view,
                           dist=dist))
        return len(self.p) - 1

    def pair(self, x, y, octave=0, la=0.0, ka=0.0, cut=False, want=True):
        """A keypoint and a point on top of it with its descriptor"""
        k = self.kp(x, y, octave, angle=ka)
        return k, self.pt(x, y, octave, self.d[k], k if want else -1, angle=la, cut=cut)

    # ---- the arrays
    def frame(self):
        kps = np.array(self.k, KP_DTYPE) if self.k else np.zeros(0, KP_DTYPE)
        return kps, np.array(self.d, np.uint8).reshape(-1, 32), np.array(self.ur, F32)

    def _col(self, key, dtype, tail=()):
        return np.array([q[key] for q in self.p], dtype).reshape((-1,) + tail)

    def _walk(self, th=None):
        match, n = [-1] * len(self.k), 0
        for i, q in enumerate(self.p):
            w = q["want"][th] if isinstance(q["want"], dict) else q["want"]
            if w >= 0:
                match[w] = i
                n += 1
        for i, q in enumerate(self.p):                          # the rotation check afterwards
            w = q["want"][th] if isinstance(q["want"], dict) else q["want"]
            if w >= 0 and q["cut"]:
                match[w] = -1
                n -= 1
        return match, n

    def projection_case(self, name, claims, mono=True, T_cur=None, **extra):
        kps, desc, ur = self.frame()
        last = dict(valid=self._col("valid", np.uint8), Xw=self._col("Xw", np.float64, (3,)), desc=self._col("desc", np.uint8, (32,)),
                    octave=self._col("octave", np.int32), angle=self._col("angle", F32), obs=self._col("obs", np.int32))
        match, n = self._walk()
        return dict(name=name, claims=tuple(claims), kps=kps, desc=desc, uright=ur, last=last, mono=mono,
                    T_cur=np.eye(4) if T_cur is None else T_cur, T_ref=np.eye(4), expect=dict(match=match, n=n), **extra)

    def local_case(self, name, claims, **extra):
        kps, desc, ur = self.frame()
        pts = dict(cand=self._col("cand", np.uint8), Xw=self._col("Xw", np.float64, (3,)), normal=self._col("normal", np.float64, (3,)),
                   min_dist=self._col("min_dist", F32), max_dist=self._col("max_dist", F32), mf_max_dist=self._col("mf_max_dist", F32),
                   desc=self._col("desc", np.uint8, (32,)), obs=self._col("obs", np.int32))
        expect = {}
        for th in LOCAL_THS:
            match, n = self._walk(th)
            inv = [(max(q["want"].values()) if isinstance(q["want"], dict) else q["want"]) >= 0 if q["in_view"] is None else bool(q["in_view"])
                   for q in self.p]
            lvl = [min(max(q["octave"], 0), NLEVELS - 1) if v else 0 for q, v in zip(self.p, inv)]
            expect[th] = dict(match=match, n=n, in_view=inv, level=lvl)
        return dict(name=name, claims=tuple(claims), kps=kps, desc=desc, uright=ur, pts=pts, kp_claimed=np.array(self.claimed, np.uint8),
                    T_cur=np.eye(4), expect=expect, **extra)


# ================================================================================================ SearchByProjection(F, F)
def proj_th_high():
    b = Builder(101)
    k0, k1 = b.kp(52, 52, 0), b.kp(152, 52, 0)
    b.pt(52, 52, 0, flip(b.d[k0], range(100)), k0)                # distance 100 == TH_HIGH: `<=` keeps it
    b.pt(152, 52, 0, flip(b.d[k1], range(101)), -1)
    return b.projection_case("th_high", ("th_high",))


def proj_ties():
    b = Builder(102)
    base = [b.desc() for _ in range(5)]
    # two cells in x: the one walked first wins although its keypoint has the LARGER index
    late, early = b.kp(98, 100, 0, flip(base[0], [0, 1, 2])), b.kp(94, 100, 0, flip(base[0], [3, 4, 5]))     # cells x = 10, 9
    b.pt(96, 100, 0, base[0], early)
    # one cell: the smaller index
    first, second = b.kp(298, 300, 0, flip(base[1], [10, 11])), b.kp(302, 300, 0, flip(base[1], [12, 13]))   # both cell x = 30
    b.pt(300, 300, 0, base[1], first)
    # a strictly smaller distance later in the walk still wins
    far, near = b.kp(394, 300, 0, flip(base[2], [1, 2, 3])), b.kp(406, 300, 0, flip(base[2], [4]))           # cells x = 39, 41
    b.pt(400, 300, 0, base[2], near)
    # one column, two rows: iy ascending inside ix
    low, high = b.kp(500, 106, 0, flip(base[3], [0, 1])), b.kp(500, 94, 0, flip(base[3], [2, 3]))            # cells y = 11, 9
    b.pt(500, 100, 0, base[3], high)
    # ix before iy: (ix 19, iy 21) is walked before (ix 21, iy 19)
    right_up, left_down = b.kp(206, 194, 0, flip(base[4], [0, 1])), b.kp(194, 206, 0, flip(base[4], [2, 3]))
    b.pt(200, 200, 0, base[4], left_down)
    return b.projection_case("ties", ("ties",), ties=dict(late=late, early=early, first=first, second=second, far=far, near=near, low=low,
                                                           high=high, right_up=right_up, left_down=left_down))


def proj_window():
    b = Builder(103)
    for (du, dv), ok in (((8.0, 0.0), False), ((7.5, 0.0), True), ((0.0, 8.0), False), ((0.0, 7.5), True)):     # fabs(d) < 8 is strict
        u, v = 101 + 80 * (len(b.k)), 101
        k = b.kp(u + du, v + dv, 0)
        b.pt(u, v, 0, b.d[k], k if ok else -1)
    r1 = F32(TH) * SF[1]                                          # 9.6000004 in float32
    k = b.kp(r1, 402, 1)                                          # u = 0: kx - u == r1 exactly
    b.pt(0, 402, 1, b.d[k], -1)
    k = b.kp(down(r1), 442, 1)
    b.pt(0, 442, 1, b.d[k], k)
    return b.projection_case("window", ("window",), r1=r1)


def proj_levels():
    b = Builder(104)
    for row, (n_last, octs) in enumerate(((3, (1, 2, 3, 4, 5)), (0, (0, 1, 2)), (NLEVELS - 1, (7, 6, 5)))):
        for col, o in enumerate(octs):
            x, y = 62 + 100 * col, 62 + 130 * row
            k = b.kp(x, y, o)
            b.pt(x, y, n_last, b.d[k], k if abs(o - n_last) <= 1 else -1)
    return b.projection_case("levels", ("levels",))


X0, X640 = -1.25, 1.25          # camera-frame X at depth 2 of u = 0 / u = 640; Y of v = 0 / v = 480: -+0.9375
Y0, Y480 = -0.9375, 0.9375


def proj_bounds():
    b = Builder(105)
    rows = ((3, 102, dict(u=0, v=102), True), (3, 202, dict(u=0, v=202, xn=down(X0)), False),            # u = -2^-15
            (633, 102, dict(u=640, v=102), True), (633, 202, dict(u=640, v=202, xn=up(X640, 2)), False),  # u = 640 + 2^-14: the next float
            (102, 3, dict(u=102, v=0), True), (202, 3, dict(u=202, v=0, yn=down(Y0)), False),
            (302, 474, dict(u=302, v=480), True), (402, 474, dict(u=402, v=480, yn=up(Y480, 2)), False),
            (424, 244, dict(u=420, v=240), True), (324, 244, dict(u=320, v=240, z=-2.0), False))         # invzc < 0
    for x, y, kw, ok in rows:
        k = b.kp(x, y, 0)
        b.pt(level=0, desc=b.d[k], want=k if ok else -1, **kw)
    return b.projection_case("bounds", ("bounds",))


def proj_claims():
    b = Builder(106)
    a = b.kp(62, 62, 0)
    bb = b.kp(66, 62, 0, flip(b.d[a], range(10)))
    b.pt(62, 62, 0, b.d[a], a)                                    # obs > 0 takes a ...
    b.pt(62, 62, 0, flip(b.d[a], [0, 1]), bb)                     # ... so the next one (a: 2, bb: 8) gets its second choice
    c = b.kp(202, 62, 0)
    b.pt(202, 62, 0, b.d[c], c)
    b.pt(202, 62, 0, b.d[c], -1)                                  # its only candidate is taken: nothing
    d = b.kp(342, 62, 0)
    b.pt(342, 62, 0, b.d[d], d, obs=0)                            # obs == 0: overwritten, and nmatches counts both
    b.pt(342, 62, 0, b.d[d], d)
    b.pt(342, 62, 0, b.d[d], -1)
    return b.projection_case("claims", ("claims",))


def _lattice(i):
    return 22 + 40 * (i % 15), 22 + 40 * (i // 15)


def _histogram(b, spec, paired):
    """spec: [(last angle, keypoint angle, count, cut)]: `count` matches with that angle pair each, on a lattice"""
    i = 0
    for la, ka, count, cut in spec:
        for _ in range(count):
            paired(b, *_lattice(i), la, ka, cut)
            i += 1


ROT_SPEC = [(45.0, 45.0, 3, False),          # exactly 0 -> bin 0
            (90.0, 0.0, 3, False),           # bin 3
            (150.0, 0.0, 3, False),          # bin 5
            (ROT_BELOW, 0.0, 1, False),      # 3.4999998 -> bin 3: stays
            (ROT_ON, 0.0, 1, True),          # 3.5 -> bin 4 (round half away from zero)
            (ROT_ABOVE, 0.0, 1, True),       # 3.5000002 -> bin 4
            (10.0, 20.0, 1, True)]           # -10 + 360 = 350 -> bin 12 (without the + 360 it would join bin 0 and stay)
ROT_BINS = {0: 3, 3: 4, 4: 2, 5: 3, 12: 1}

# name -> ([(bin, count)], bins that stay)
MAXIMA = {
    "four_equal": ([(2, 3), (4, 3), (6, 3), (8, 3)], (2, 4, 6)),                    # the three lowest indices stay
    "tenth_kept": ([(1, 20), (3, 2), (5, 2), (7, 1)], (1, 3, 5)),                   # 2 < 0.1f * 20 == 2.0f is false, for max2 and max3
    "tenth_cut_both": ([(1, 20), (3, 1), (5, 1)], (1,)),                            # max2 = 1: cut together with the third
    "tenth_cut_third": ([(1, 20), (3, 2), (5, 1)], (1, 3)),
    "arms": ([(1, 2), (2, 5), (3, 3), (4, 4), (5, 1), (6, 4)], (2, 4, 6)),          # first arm twice, second twice, third once
}


def _maxima_spec(name):
    bins, keep = MAXIMA[name]
    return [(30.0 * bn, 0.0, count, bn not in keep) for bn, count in bins]


def _proj_paired(b, x, y, la, ka, cut):
    b.pair(x, y, 0, la, ka, cut)


def proj_rot_bins():
    b = Builder(107)
    _histogram(b, ROT_SPEC, _proj_paired)
    return b.projection_case("rot_bins", ("rot_bins",), bins=ROT_BINS)


def proj_three_maxima(name):
    b = Builder(108)
    _histogram(b, _maxima_spec(name), _proj_paired)
    return b.projection_case("three_maxima_" + name, ("three_maxima",), bins=dict(MAXIMA[name][0]), keep=MAXIMA[name][1])


def proj_stereo_gate():
    """bf = 40: ur = u - 20; level-0 radius 8"""
    b = Builder(109)
    for i, (ur_of, ok) in enumerate(((lambda ur: ur + 8.0, True), (lambda ur: up(ur + 8.0), False),        # er == radius passes (`>`)
                                     (lambda ur: 0.0, True), (lambda ur: -1.0, True),                      # no right coordinate: not gated
                                     (lambda ur: 5.0, False))):                                            # the twin of the two: gated
        u = 102 + 100 * i if i != 1 else 22                                     # ur = 2, uRight = 10: one float of uRight is one of er
        k = b.kp(u, 102, 0, uright=ur_of(u - 20.0))
        b.pt(u, 102, 0, b.d[k], k if ok else -1)
    return b.projection_case("stereo_gate", ("stereo",), mono=False)


TLC_STEP = 2.0 ** -20


def proj_stereo_direction(name, tlc_z, window):
    """T_ref = identity, so tlc = -tcw; the points' world Z carries tlc.z, and their camera-frame Z is exactly 2.  nLast = 3;
    keypoints on octaves 5, 1, 4, 2 see [3, inf) / [0, 3] / [2, 4] differently."""
    b = Builder(110)
    for i, o in enumerate((5, 1, 4, 2)):
        x = 102 + 140 * i
        k = b.kp(x, 102, o)
        b.pt(x, 102, 3, b.d[k], k if window[0] <= o <= window[1] else -1, dz=tlc_z)
    T = np.eye(4)
    T[2, 3] = -tlc_z
    return b.projection_case("stereo_" + name, ("stereo",), mono=False, T_cur=T, tlc_z=tlc_z)


CROWD_CAPACITY = 1600


def proj_crowd():
    """1500 keypoints inside one level-7 window (radius 28.7), 1400 of them in the grid cell (20, 20), near-duplicate descriptors;
    eight points with observations on the same spot take one keypoint each, so every one depends on what the earlier ones took.
    Their candidate lists overflow the per-frame key list (the single kernel's in LDS, the split form's in HBM) and the late ones
    are evaluated by phase 2.  A shape case: the oracle is the answer."""
    rng = np.random.default_rng(111)
    n, dense = 1500, 1400
    kps = np.zeros(n, KP_DTYPE)
    kps["x"][:dense], kps["y"][:dense] = rng.uniform(196, 204, dense), rng.uniform(196, 204, dense)
    kps["x"][dense:], kps["y"][dense:] = rng.uniform(176, 224, n - dense), rng.uniform(176, 224, n - dense)
    kps["octave"], kps["size"], kps["response"], kps["class_id"] = rng.choice([6, 7], n), 31, 1, -1
    base = rng.integers(0, 256, 32).astype(np.uint8)
    desc = np.stack([flip(base, rng.integers(0, 256, rng.integers(0, 4))) for _ in range(n)])
    m = 8
    X = np.array([(200 - K[2]) / K[0] * 2.0, (200 - K[3]) / K[1] * 2.0, 2.0])
    last = dict(valid=np.ones(m, np.uint8), Xw=np.tile(X, (m, 1)), desc=np.tile(base, (m, 1)), octave=np.full(m, 7, np.int32),
                angle=np.zeros(m, F32), obs=np.ones(m, np.int32))
    return dict(name="crowd", claims=("crowd",), kps=kps, desc=desc, uright=np.full(n, -1, F32), last=last, mono=True, T_cur=np.eye(4),
                T_ref=np.eye(4), expect=None, centre=(200.0, 200.0), radius=F32(TH) * SF[7], levels=(6, 8))


def proj_sparse(n):
    b = Builder(112)
    if n:
        b.pair(322, 242)
    b.pt(102, 102, 0, b.desc(), -1)
    return b.projection_case("sparse_%d" % n, ("sparse",))


def projection_cases():
    return [proj_th_high(), proj_ties(), proj_window(), proj_levels(), proj_bounds(), proj_claims(), proj_rot_bins()] + \
        [proj_three_maxima(k) for k in MAXIMA] + [proj_sparse(0), proj_sparse(1)]


def stereo_cases():
    return [proj_stereo_gate(),
            proj_stereo_direction("forward", MB + TLC_STEP, (3, 99)),          # tlc.z > mb: [nLast, inf)
            proj_stereo_direction("at_mb", MB, (2, 4)),                        # `>` is strict: the plain window
            proj_stereo_direction("below_mb", MB - TLC_STEP, (2, 4)),
            proj_stereo_direction("backward", -(MB + TLC_STEP), (0, 3))]       # -tlc.z > mb: [0, nLast]


# ================================================================================================ the local-map search
LOCAL_THS = (1.0, 3.0)
NNRATIO = 0.8
COS_LIMIT = 0.5
COS_STEP = 2e-6                 # relative distance of the twins around 0.998 (float32 rounding of viewCos: 6e-8)


def local_frustum():
    """Every point of the first block has its own keypoint; the distance / angle twins share one at the image centre and have no
    observations, so each in-view one overwrites the last: in_view says which passed."""
    b = Builder(201)
    k = [b.kp(102 + 140 * i, 102, 2) for i in range(3)]
    b.pt(102, 102, 2, b.d[k[0]], k[0])
    b.pt(242, 102, 2, b.d[k[1]], -1, z=-2.0)                                   # PcZ < 0
    b.pt(382, 102, 2, b.d[k[2]], -1, valid=0)                                  # cand == 0
    c = b.kp(320, 240, 2)
    two = F32(2.0)
    for kw, ok in ((dict(min_dist=two), True), (dict(min_dist=up(two)), False), (dict(max_dist=two), True), (dict(max_dist=down(two)), False),
                   (dict(normal=(0, 0, 0.5)), True), (dict(normal=(0, 0, float(down(0.5)))), False)):       # viewCos == 0.5 stays (`<`)
        b.pt(320, 240, 2, b.d[c], c if ok else -1, obs=0, **kw)
    return b.local_case("frustum", ("depth", "cand", "dist", "angle"))


def local_bounds():
    b = Builder(202)
    rows = ((633, 102, dict(u=640, v=102), True), (633, 242, dict(u=640, v=242, xn=up(X640, 2)), False),
            (3, 102, dict(u=0, v=102), True), (3, 242, dict(u=0, v=242, xn=down(X0)), False),
            (102, 474, dict(u=102, v=480), True), (242, 474, dict(u=242, v=480, yn=up(Y480, 2)), False),
            (102, 3, dict(u=102, v=0), True), (242, 3, dict(u=242, v=0, yn=down(Y0)), False))
    for x, y, kw, ok in rows:                                                   # level 7: radius 2.5 * 3.58 = 8.96
        k = b.kp(x, y, 7)
        b.pt(level=7, desc=b.d[k], want=k if ok else -1, **kw)
    return b.local_case("bounds", ("bounds",))


def local_predict_scale():
    b = Builder(203)
    for i, lvl in enumerate(list(range(NLEVELS)) + [-3, 12]):                   # 1.2^(l - 0.5); far below 1; beyond the top
        x, y = 62 + 140 * (i % 4), 62 + 130 * (i // 4)
        k = b.kp(x, y, min(max(lvl, 0), NLEVELS - 1))
        b.pt(x, y, lvl, b.d[k], k)
    return b.local_case("predict_scale", ("predict_scale",))


def _normal_with_cos(X, c):
    """A unit vector at viewing cosine c to X"""
    d = X / np.linalg.norm(X)
    side = np.cross(d, [0.0, 1.0, 0.0])
    side /= np.linalg.norm(side)
    return c * d + np.sqrt(1.0 - c * c) * side


def local_radius():
    """Level 0.  viewCos on both sides of 0.998 (radius 2.5 vs 4.0, times th); a keypoint 3 px (th = 1: between 2.5 and 4) or 9 px
    (th = 3: between 7.5 and 12) beside the projection decides.  Then the level window [level - 1, level] at level 3."""
    b = Builder(204)
    hi, lo = 0.998 * (1 + COS_STEP), 0.998 * (1 - COS_STEP)
    for i, (off, c, ok1, ok3) in enumerate(((3, hi, False, True), (3, lo, True, True), (9, hi, False, False), (9, lo, False, True))):
        u = 101 + 140 * i
        k = b.kp(u + off, 102, 0)
        X = np.array([(u - K[2]) / K[0] * 2.0, (102 - K[3]) / K[1] * 2.0, 2.0])
        b.pt(u, 102, 0, b.d[k], {1.0: k if ok1 else -1, 3.0: k if ok3 else -1}, normal=_normal_with_cos(X, c), in_view=True)
    for i, o in enumerate((1, 2, 3, 4)):
        x = 62 + 140 * i
        k = b.kp(x, 322, o)
        b.pt(x, 322, 3, b.d[k], k if o in (2, 3) else -1, in_view=True)
    return b.local_case("radius", ("radius", "level_window"), cos=(hi, lo))


def local_th_high():
    b = Builder(205)
    k0, k1 = b.kp(102, 102, 2), b.kp(242, 102, 2)
    b.pt(102, 102, 2, flip(b.d[k0], range(100)), k0)
    b.pt(242, 102, 2, flip(b.d[k1], range(101)), -1, in_view=True)
    return b.local_case("th_high", ("th_high",))


# (distance, octave) of the keypoints in walk order, the index of the one that is taken or None
RATIO_ROWS = (
    (((39, 3), (50, 3)), 0),              # 39 > 0.8f * 50 == 40.0f is false
    (((40, 3), (50, 3)), 0),              # equal: `>` keeps it
    (((41, 3), (50, 3)), None),
    (((41, 3), (50, 2)), 0),              # the second best on another level: no ratio test
    (((40, 2), (30, 3), (40, 3)), 1),     # the displaced second best is the FIRST one, on level 2: no ratio test
    (((40, 2), (36, 3), (40, 3)), 1),     # ... with 36 > 0.8f * 40: a second best on level 3 would reject it
    (((40, 3), (40, 2)), 0),              # equal distances: the later one becomes second best, carrying its level
    (((40, 3), (40, 3)), None),           # ... the same level: 40 > 32
)


def local_ratio():
    """Predicted level 3 (window [2, 3], radius 4.3 / 13); the keypoints of a row sit 1 px apart in one grid cell, so the walk
    takes them in index order."""
    b = Builder(206)
    for i, (cands, take) in enumerate(RATIO_ROWS):
        x, y = 61 + 140 * (i % 4), 62 + 130 * (i // 4)
        base = b.desc()
        ks = [b.kp(x + j, y, o, flip(base, range(d))) for j, (d, o) in enumerate(cands)]
        b.pt(x + 1, y, 3, base, -1 if take is None else ks[take], in_view=True)
    # the equal pair in two grid cells: the cell walked first (x = 6) holds the LARGER index, which is taken; its partner becomes
    # second best on another level.  By index the other one would win.
    base = b.desc()
    late, early = b.kp(66, 322, 3, flip(base, range(40))), b.kp(64, 322, 2, flip(base, range(40)))
    b.pt(65, 322, 3, base, early, in_view=True)
    return b.local_case("ratio", ("ratio",), tie=dict(late=late, early=early))


def local_claimed():
    b = Builder(207)
    a = b.kp(102, 102, 2, claimed=1)
    b.pt(102, 102, 2, b.d[a], -1, in_view=True)                                 # held a point with observations before the call
    c = b.kp(242, 102, 2)
    b.pt(242, 102, 2, b.d[c], c)
    b.pt(242, 102, 2, b.d[c], -1, in_view=True)                                 # matched in this call by a point with observations
    d = b.kp(382, 102, 2)
    b.pt(382, 102, 2, b.d[d], d, obs=0)
    b.pt(382, 102, 2, b.d[d], d)                                                # ... by one without: overwritten
    return b.local_case("claimed", ("claimed",))


def local_stereo():
    """Level 0, bf = 40: mTrackProjXR = u - 20; er == r * sf[0] passes"""
    b = Builder(208)
    k = b.kp(102, 102, 0, uright=82.0 + 2.5)
    b.pt(102, 102, 0, b.d[k], k)
    k = b.kp(21, 242, 0, uright=up(1.0 + 2.5))                                  # small values: one float of uRight is one of er
    b.pt(21, 242, 0, b.d[k], {1.0: -1, 3.0: k}, in_view=True)                   # th = 3: the radius is 7.5
    k = b.kp(20.25, 382, 0, uright=up(0.25 + 7.5))
    b.pt(20.25, 382, 0, b.d[k], -1, in_view=True)
    k = b.kp(522, 102, 0, uright=0.0)
    b.pt(522, 102, 0, b.d[k], k)
    return b.local_case("stereo", ("stereo",))


def local_cases():
    return [local_frustum(), local_bounds(), local_predict_scale(), local_radius(), local_th_high(), local_ratio(), local_claimed(),
            local_stereo()]


# ================================================================================================ SearchByPoints
NNRATIO_POINTS = 0.75
BF_LIST_KS = (1, 2, 3, 4)


class Pairing:
    """currentKF rows and pKF columns; want[row] = column or -1, cut by the rotation check where said"""

    def __init__(self, seed):
        self.rng = np.random.default_rng(seed)
        self.r, self.c, self.want, self.cut = [], [], [], []

    def desc(self):
        return self.rng.integers(0, 256, 32).astype(np.uint8)

    def row(self, desc, want, angle=0.0, has=1, cut=False):
        self.r.append((np.array(desc, np.uint8), angle, has))
        self.want.append(want)
        self.cut.append(cut)
        return len(self.r) - 1

    def col(self, desc, angle=0.0, has=1):
        self.c.append((np.array(desc, np.uint8), angle, has))
        return len(self.c) - 1

    def case(self, name, claims, **extra):
        def side(items):
            k = np.zeros(len(items), KP_DTYPE)
            for i, (_, angle, _) in enumerate(items):
                k[i] = (22 + 40 * (i % 15), 22 + 40 * (i // 15), 31.0, angle, 1.0, 0, -1)
            return k, np.array([d for d, _, _ in items], np.uint8).reshape(-1, 32), np.array([h for _, _, h in items], np.uint8)
        k1, d1, h1 = side(self.r)
        k2, d2, h2 = side(self.c)
        match = [-1 if c else w for w, c in zip(self.want, self.cut)]
        return dict(name=name, claims=tuple(claims), k1=k1, d1=d1, h1=h1, k2=k2, d2=d2, h2=h2,
                    expect={True: dict(match=match, n=sum(m >= 0 for m in match)),
                            False: dict(match=list(self.want), n=sum(w >= 0 for w in self.want))}, **extra)


def points_th_low():
    p = Pairing(301)
    c0, c1 = p.col(p.desc()), p.col(p.desc())
    p.row(flip(p.c[c0][0], range(49)), c0)                        # 49 < TH_LOW
    p.row(flip(p.c[c1][0], range(50)), -1)
    return p.case("th_low", ("th_low",))


def points_ratio():
    """Per row a base descriptor and two columns at the given distances from it"""
    p = Pairing(302)
    for d1, d2, ok in ((30, 40, False), (29, 40, True), (30, 30, False)):        # 30 < 0.75f * 40 == 30.0f is false; a tie never matches
        base = p.desc()
        a = p.col(flip(base, range(d1)))
        p.col(flip(base, range(100, 100 + d2)))
        p.row(base, a if ok else -1)
    return p.case("ratio", ("ratio",))


def points_single():
    p = Pairing(303)
    c = p.col(p.desc())
    p.row(flip(p.c[c][0], range(49)), c)                          # bestDist2 stays 256
    return p.case("single", ("ratio",))


def points_given_away():
    """Columns c0 .. c3 = base with 10 bits of their own flipped, c4 with 20, three unrelated ones.  Rows 0 .. 3 hold 8 of their
    column's bits (distances 2 / 18 / 28); row 4 is the base itself (10 x 4, then 20); row 5 has 50 bits of its own (60 x 4, 70)."""
    p = Pairing(304)
    base = p.desc()
    cols = [p.col(flip(base, range(40 * j, 40 * j + (20 if j == 4 else 10)))) for j in range(5)]
    for _ in range(3):
        p.col(p.desc())
    for j in range(4):
        p.row(flip(base, range(40 * j, 40 * j + 8)), cols[j])
    p.row(base, cols[4])                                          # its four nearest are given away: the fifth, by recomputation
    p.row(flip(base, range(200, 250)), -1)                        # its list ends at 60 >= TH_LOW: nothing, without recomputation
    return p.case("given_away", ("given_away",), base=base)


def points_flags():
    p = Pairing(305)
    c = [p.col(p.desc(), has=h) for h in (1, 0, 1)]
    p.row(p.c[c[0]][0], -1, has=0)                                # the row is off
    p.row(p.c[c[1]][0], -1)                                       # its only good partner is off
    p.row(p.c[c[2]][0], c[2])
    p.row(p.c[c[0]][0], c[0])                                     # the column the first row did not take
    return p.case("flags", ("flags",))


def _points_histogram(name, claims, spec, **extra):
    p = Pairing(306)

    def paired(_, x, y, la, ka, cut):
        d = p.desc()
        c = p.col(d, angle=ka)
        p.row(d, c, angle=la, cut=cut)
    _histogram(None, spec, paired)
    return p.case(name, claims, **extra)


def points_cases():
    return [points_th_low(), points_ratio(), points_single(), points_given_away(), points_flags(),
            _points_histogram("rot_bins", ("rot_bins",), ROT_SPEC, bins=ROT_BINS)] + \
        [_points_histogram("three_maxima_" + k, ("three_maxima",), _maxima_spec(k), bins=dict(MAXIMA[k][0]), keep=MAXIMA[k][1]) for k in MAXIMA]


_CACHE = {}


def all_cases():
    """dict(projection=[...], stereo=[...], local=[...], points=[...], crowd=case), built once"""
    if not _CACHE:
        _CACHE.update(projection=projection_cases(), stereo=stereo_cases(), local=local_cases(), points=points_cases(), crowd=proj_crowd())
    return _CACHE
