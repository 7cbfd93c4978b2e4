"""Hand-built problems for Optimizer::PoseOptimization (k_pose_opt): every edge is planted -- keypoints with
ORBextractor.set_keypoints, map points with Tracker.set_last / set_matches, right coordinates with set_uright -- so that the
gates, the edge lists, the thresholds and the round / Levenberg logic are hit on purpose and not by whatever a rendered scene
happens to give.  tests/test_poseopt_cases_cpu.py proves on the host that every case is what it claims and certifies it under
re-ordering of its edges (`certify`); tests/test_poseopt_cases_gpu.py runs all of them as the frames of one launch.

A case is a dict: name, group, claim, kps (KP_DTYPE), has, Xw [nkp, 3], uright, bf, K, T0, and `expect`, the hand answer where the
group has one (flags by keypoint index, rounds, whether the pose is the input pose).  Everything is seeded and finite.

The camera is the unit camera of tests/match_cases.py (fx = fy = 512, cx = 320, cy = 240, bf = 40).  Scene points are drawn in the
camera frame of a true pose (pixel uniformly in the image, depth 1.5 .. 8 m) and moved to the world; an exact edge's keypoint is the
float32 of its projection.  A residual is planted by moving the keypoint (or its right coordinate) by a fixed number of pixels:
chi2 = invSigma2[octave] * |residual|^2 then sits where the case says, up to the pull the probes exert on a pose pinned by a few
hundred exact edges (a few hundredths of a pixel; the CPU test prints the margins).

The seeds of the `rounds` and `lm` cases were found by a seeded search on the host (200 problems of rounds_problem / lm_problem
each, kept when `certify` passed); what they are claimed to show is re-derived from the oracle's per-round trace by the CPU test."""
import numpy as np

from fuse_cases import F32, INV_SIGMA2, NLEVELS, SF
from sdslam_amd.capi import KP_DTYPE
from sdslam_amd.synth import se3_exp

K = (512.0, 512.0, 320.0, 240.0)
BF = 40.0
CAPACITY = 2048                 # the tracker's keypoint limit: the `full` case matches every keypoint of such a frame
POSE_TOL = 1e-5
MARGIN = 64.0                   # certification: spreads across edge orders stay this factor inside what is asserted
N_ORDERS = 8                    # seeded permutations next to the given order
CHI2_MONO, CHI2_STEREO = F32(5.991), F32(7.815)
T_TRUE = se3_exp((0.3, -0.2, 0.4), (12.0, -20.0, 8.0))           # a world frame away from the identity
NEAR = ((0.02, -0.015, 0.01), (0.5, -0.4, 0.3))                 # the usual start: 2 cm and half a degree off the truth


def start(twist=NEAR, T_true=T_TRUE):
    return se3_exp(*twist) @ T_true


def _to_world(Xc, T):
    return (Xc - T[:3, 3]) @ T[:3, :3]                           # R^T (Xc - t), row vectors


class Scene:
    """nkp keypoints; those in `has` carry a map point that projects onto them under T_true (exactly, or with noise)."""

    def __init__(self, seed, nkp, has=None, stereo=None, noise=0.0, bf=BF, T_true=T_TRUE, octaves=None):
        rng = self.rng = np.random.default_rng(seed)
        self.nkp, self.bf, self.T_true = nkp, bf, T_true
        self.has = np.ones(nkp, bool) if has is None else np.asarray(has, bool).copy()
        self.u, self.v, self.z = rng.uniform(20, 620, nkp), rng.uniform(20, 460, nkp), rng.uniform(1.5, 8.0, nkp)
        self.octave = rng.integers(0, NLEVELS, nkp) if octaves is None else np.broadcast_to(octaves, (nkp,)).copy()
        self.stereo = np.zeros(nkp, bool) if stereo is None else np.broadcast_to(stereo, (nkp,)).copy()
        self.dx, self.dy, self.dr = (noise * SF[self.octave] * rng.standard_normal(nkp) for _ in range(3))
        self.ur_raw = {}                                         # keypoint -> the float32 value to store whatever the geometry says
        self.behind = np.zeros(nkp, bool)

    def put(self, i, u=None, v=None, z=None, octave=None, stereo=None, dx=0.0, dy=0.0, dr=0.0, ur_raw=None, has=True, behind=False):
        """Edge i by hand: projection (u, v) at depth z, residual (dx, dy) on the keypoint and dr on its right coordinate"""
        for name, val in (("u", u), ("v", v), ("z", z), ("octave", octave), ("stereo", stereo)):
            if val is not None:
                getattr(self, name)[i] = val
        self.dx[i], self.dy[i], self.dr[i], self.has[i], self.behind[i] = dx, dy, dr, has, behind
        if ur_raw is not None:
            self.ur_raw[i] = F32(ur_raw)
        return i

    def gross(self, idx, lo=20.0, hi=100.0):
        """Gross outliers: the keypoints of `idx` move by lo .. hi pixels in a random direction"""
        idx = np.asarray(idx, int)
        r, a = self.rng.uniform(lo, hi, len(idx)), self.rng.uniform(0, 2 * np.pi, len(idx))
        self.dx[idx], self.dy[idx] = r * np.cos(a), r * np.sin(a)

    def arrays(self):
        Xc = np.stack([(self.u - K[2]) / K[0] * self.z, (self.v - K[3]) / K[1] * self.z, self.z], 1)
        Xc[self.behind] *= -1.0                                  # the same pixel, z_cam < 0
        Xw = _to_world(Xc, self.T_true)
        kps = np.zeros(self.nkp, KP_DTYPE)
        kps["x"], kps["y"], kps["octave"] = (self.u + self.dx).astype(F32), (self.v + self.dy).astype(F32), self.octave
        kps["size"], kps["response"], kps["class_id"] = 31.0, 1.0, -1
        ur = np.where(self.stereo, self.u - self.bf / self.z + self.dr, -1.0).astype(F32)
        for i, val in self.ur_raw.items():
            ur[i] = val
        return kps, self.has.copy(), Xw, ur

    def case(self, name, group, claim, T0=None, expect=None, **extra):
        kps, has, Xw, ur = self.arrays()
        assert np.isfinite(Xw).all() and np.isfinite(ur).all() and np.isfinite(kps["x"]).all() and np.isfinite(kps["y"]).all()
        return dict(name=name, group=group, claim=claim, kps=kps, has=has, Xw=Xw, uright=ur, bf=self.bf, K=K,
                    T0=start() if T0 is None else T0, expect=expect, **extra)


def _flags(nkp, outliers):
    f = np.zeros(nkp, bool)
    f[list(outliers)] = True
    return f


# ================================================================================================ 1. edge-count gates
def gate_case(n, seed=1101):
    """n edges among 40 keypoints.  Fewer than 3: PoseOptimization returns 0 and touches nothing.  3 .. 9: one round
    (optimizer.edges().size() < 10 breaks).  From 10 on: four.  The 9- and 10-edge cases are twins: the same nine edges, one of them a
    gross outlier, and for the tenth one more clean edge on a keypoint that the 9-edge case leaves without a point."""
    nkp = 40
    slots = [3, 5, 8, 13, 17, 21, 26, 30, 34, 37, 39]            # the edges' keypoints, in the order they are added
    twin = n in (9, 10)
    s = Scene(seed if not twin else 1109, nkp, has=np.zeros(nkp, bool), octaves=0)
    for i in slots[:n]:
        s.has[i] = True
    bad = []
    if n >= 9:
        bad = [slots[4]]
        s.dx[bad[0]], s.dy[bad[0]] = 40.0, -30.0                  # 50 px off at octave 0
    few = n < 3
    expect = dict(outlier=_flags(nkp, [] if few else bad), n=n, rounds=0 if few else (1 if n < 10 else 4), untouched=few,
                  n_inliers=0 if few else n - len(bad))
    return s.case("gate_%d" % n, "gates", "n < 3 untouched / n < 10 one round / else four", expect=expect)


def gate_cases():
    return [gate_case(n) for n in (0, 1, 2, 3, 9, 10, 11)]


# ================================================================================================ 2. edge lists
def _list_case(name, claim, seed, nkp, has, frac_bad=0.15, stereo_every=0):
    has = np.asarray(has, bool)
    stereo = np.zeros(nkp, bool)
    if stereo_every:
        stereo[::stereo_every] = True
    s = Scene(seed, nkp, has=has, stereo=stereo)
    idx = np.flatnonzero(has)
    n_bad = int(len(idx) * frac_bad)
    s.gross(s.rng.choice(idx, n_bad, replace=False)) if n_bad else None
    return s.case(name, "lists", claim)


def _subset(seed, nkp, n):
    has = np.zeros(nkp, bool)
    has[np.random.default_rng(seed).choice(nkp, n, replace=False)] = True
    return has


def list_cases():
    out = []
    for n in (63, 64, 65, 255, 256, 257, 513):                   # one lane's list gains its next slot at 64 k + 1 edges of a wave
        nkp = n + n // 3 + 5
        out.append(_list_case("count_%d" % n, "%d edges scattered over %d keypoints" % (n, nkp), 1200 + n, nkp, _subset(n, nkp, n),
                              stereo_every=3 if n == 257 else 0))
    out.append(_list_case("packed_64", "64 edges on keypoints 0 .. 63, no other keypoint: one full slot per lane", 1211, 64, np.ones(64, bool)))
    out.append(_list_case("packed_65", "65 edges on keypoints 0 .. 64", 1212, 65, np.ones(65, bool)))
    has = np.zeros(600, bool)
    has[:64] = True
    out.append(_list_case("first_window", "all edges in keypoints [0, 64): with four waves three lists are empty", 1213, 600, has))
    has = np.zeros(600, bool)
    has[320:384] = _subset(7, 64, 40)
    out.append(_list_case("one_window", "40 edges, all in keypoints [320, 384): the second pass of the second wave", 1214, 600, has))
    has = np.zeros(700, bool)
    has[[698, 699, 131]] = True
    out.append(_list_case("tail", "edges at keypoints nkp - 1, nkp - 2 and one elsewhere", 1215, 700, has, frac_bad=0.0))
    out.append(_list_case("full", "every keypoint of a full-capacity frame matched", 1216, CAPACITY, np.ones(CAPACITY, bool)))
    has = _subset(8, 769, 500)
    has[768] = True
    out.append(_list_case("mod256", "nkp = 769 = 1 mod 256, the last keypoint matched", 1217, 769, has))
    return out


# ================================================================================================ 3. information / threshold twins
# (name, octave, stereo, (dx, dy, dr), outlier): chi2 = invSigma2[octave] * (dx^2 + dy^2 + dr^2) against 5.991 (mono) / 7.815 (stereo)
PROBES = (
    ("mono_3px_oct0", 0, False, (3.0, 0.0, 0.0), True),           # 9 > 5.991
    ("mono_3px_oct3", 3, False, (3.0, 0.0, 0.0), False),          # 9 / 1.2^6 = 3.01
    ("mono_3px_oct0_y", 0, False, (0.0, -3.0, 0.0), True),
    ("mono_3px_oct3_y", 3, False, (0.0, -3.0, 0.0), False),
    ("stereo_3px_oct0", 0, True, (0.0, 0.0, 3.0), True),          # 9 > 7.815, the residual in uright only
    ("stereo_3px_oct3", 3, True, (0.0, 0.0, 3.0), False),
    ("stereo_3px_oct0_neg", 0, True, (0.0, 0.0, -3.0), True),
    ("stereo_3px_oct3_neg", 3, True, (0.0, 0.0, -3.0), False),
    ("between_mono", 0, False, (-2.6, 0.0, 0.0), True),           # 6.76: over 5.991 as a mono edge ...
    ("between_stereo", 0, True, (-2.6, 0.0, 0.0), False),         # ... under 7.815 as a stereo edge
    ("sum_mono", 0, False, (0.0, 2.2, 0.0), False),               # 4.84 passes 5.991 ...
    ("sum_stereo", 0, True, (0.0, 2.2, -2.0), True),              # ... 4.84 + 4 = 8.84 fails 7.815
)


def info_case():
    nkp, first = 340, 300                                         # 300 exact edges (every third stereo) pin the pose
    stereo = np.zeros(nkp, bool)
    stereo[:first:3] = True
    has = np.zeros(nkp, bool)
    has[:first] = True
    s = Scene(1301, nkp, has=has, stereo=stereo)
    probes, bad = {}, []
    for j, (name, octave, st, (dx, dy, dr), outl) in enumerate(PROBES):
        i = s.put(first + 3 * j, octave=octave, stereo=st, dx=dx, dy=dy, dr=dr)
        probes[name] = i
        if outl:
            bad.append(i)
    n = first + len(PROBES)
    return s.case("info_twins", "info", "3 px at octave 0 / 3; 2.6 px mono / stereo; 2.2 px with and without a 2 px right residual",
                  expect=dict(outlier=_flags(nkp, bad), n=n, rounds=4, untouched=False, n_inliers=n - len(bad)), probes=probes)


# ================================================================================================ 4. uright forms
def uright_case(bf):
    """One 64-keypoint window, every keypoint matched, mono and stereo edges alternating.  !(uright < 0) makes an edge stereo:
    0.0f and -0.0f both do.  A probe with a zero right coordinate whose point projects to ur = 5 is an outlier as a stereo edge (25 >
    7.815; 5 px and not 3, because 60 exact edges give way by a few tenths of a pixel) and would be a perfect inlier as a mono edge; its twin's point projects to ur = 0 (u = bf / z) and is an inlier either
    way.  With bf == 0 the right coordinate of a point is its u."""
    nkp = 64
    stereo = np.arange(nkp) % 2 == 1
    s = Scene(1401 if bf else 1402, nkp, stereo=stereo, bf=bf, octaves=0)
    bad = []
    if bf:
        z = 2.0
        u0 = bf / z                                               # 20: projects to ur = 0
        rows = ((6, -1.0, u0 + 5.0, False), (11, 0.0, u0 + 5.0, True), (20, -0.0, u0 + 5.0, True), (27, 0.0, u0, False),
                (34, -0.0, u0, False), (41, -1.0, u0, False))
        for i, raw, u, outl in rows:
            s.put(i, u=u, z=z, ur_raw=raw)
            bad += [i] if outl else []
    else:
        for i, octave, dr, outl in ((7, 0, 3.0, True), (21, 3, 3.0, False), (35, 0, 0.0, False), (49, 0, -3.0, True)):
            s.put(i, octave=octave, stereo=True, dr=dr)           # ur = u + dr, always positive
            bad += [i] if outl else []
        s.put(12, u=25.0, stereo=False, ur_raw=-1.0)
    return s.case("uright_bf%d" % int(bf), "uright", "-1 / 0.0f / -0.0f / positive uright, bf = %g" % bf,
                  expect=dict(outlier=_flags(nkp, bad), n=nkp, rounds=4, untouched=False, n_inliers=nkp - len(bad)))


def uright_cases():
    return [uright_case(BF), uright_case(0.0)]


# ================================================================================================ 5. rounds
def all_outliers_case(seed=1501):
    """12 keypoints against 12 unrelated points: after round 0 every edge is an outlier, rounds 1 .. 3 have no active edge, optimize()
    does not iterate and the estimate set at the top of the round -- the input pose through a quaternion -- is the result."""
    nkp = 12
    s = Scene(seed, nkp, octaves=0)
    s.u, s.v = s.rng.uniform(20, 620, nkp), s.rng.uniform(20, 460, nkp)
    s.dx, s.dy = s.rng.uniform(-300, 300, nkp), s.rng.uniform(-200, 200, nkp)       # the keypoints: somewhere else
    return s.case("all_outliers", "rounds", "every edge bad after round 0: the input pose's quaternion round trip comes back",
                  expect=dict(outlier=np.ones(nkp, bool), n=nkp, rounds=4, untouched=False, n_inliers=0, round_trip=True))


def rounds_problem(seed, n=60, noise=1.0, n_mid=14, lo=2.0, hi=4.0, twist=((0.08, -0.05, 0.06), (3.0, -2.0, 2.5))):
    """A small noisy problem with `n_mid` edges lo .. hi sigma off: their flags move from round to round"""
    s = Scene(seed, n, noise=noise, stereo=np.arange(n) % 4 == 0)
    mid = s.rng.choice(n, n_mid, replace=False)
    r, a = s.rng.uniform(lo, hi, n_mid) * SF[s.octave[mid]], s.rng.uniform(0, 2 * np.pi, n_mid)
    s.dx[mid], s.dy[mid] = r * np.cos(a), r * np.sin(a)
    return s, start(twist)


# seeds 1600 .. 1799 of rounds_problem were tried (and 200 more with 30 of 40 edges 2 .. 3 sigma off): (b) and (c) are common;
# NO problem was found in which an edge's FINAL flag depends on Huber in the fourth round (d) -- the edges active in that round all had
# chi2 under the threshold one round earlier, so the kernel only touches what sits on the threshold.  `huber_rounds` is the nearest
# thing found: its pose and its iteration counts move when Huber is dropped a round early or kept to the end.
ROUNDS_SEEDS = dict(readmitted=1601, late_outlier=1600, huber_rounds=1621)


def rounds_case(kind):
    s, T0 = rounds_problem(ROUNDS_SEEDS[kind])
    claim = dict(readmitted="an edge flagged in an early round is clear at the end",
                 late_outlier="an edge clear after round 0 is flagged at the end",
                 huber_rounds="pose and counts depend on Huber being on in rounds 0 .. 2 and off in round 3; (b) and (c) in one case")[kind]
    return s.case(kind, "rounds", claim, T0=T0)


def behind_case():
    """One map point behind the camera under T0 and the truth (z_cam = -3): its projection is the mirrored pixel, its keypoint
    sits 150 px from it; flagged from round 0 on"""
    nkp = 200
    s = Scene(1505, nkp)
    i = s.put(77, u=400.0, v=300.0, z=3.0, octave=0, dx=150.0, behind=True)
    return s.case("behind", "rounds", "a point with z_cam < 0 is flagged from round 0", behind=i,
                  expect=dict(outlier=_flags(nkp, [i]), n=nkp, rounds=4, untouched=False, n_inliers=nkp - 1))


def rounds_cases():
    return [all_outliers_case()] + [rounds_case(k) for k in ROUNDS_SEEDS] + [behind_case()]


# ================================================================================================ 6. LM exits
def lm_problem(kind, seed):
    rng = np.random.default_rng(seed)
    if kind == "far":                                             # 20 .. 40 degrees and tens of centimetres off: trials are rejected
        axis = rng.standard_normal(3)
        twist = (rng.uniform(-0.4, 0.4, 3), rng.uniform(20.0, 40.0) * axis / np.linalg.norm(axis))
        s = Scene(seed, 120, noise=0.3, stereo=np.arange(120) % 3 == 0)
        s.gross(s.rng.choice(120, 12, replace=False))
        return s, start(twist)
    if kind == "truth":                                           # exact data, started at the truth
        return Scene(seed, 80, stereo=np.arange(80) % 2 == 0), T_TRUE.copy()
    if kind == "three":                                           # three exact edges: no redundancy, all ten iterations are used
        return Scene(seed, 3, octaves=0), start()
    s = Scene(seed, 150, noise=1.0, stereo=np.arange(150) % 3 == 0)              # "noisy"
    s.gross(s.rng.choice(150, 30, replace=False))
    return s, start()


# (name, kind, seed, exit claimed): seeds 1800 .. 1866 of each kind were tried; all four exits of optimize() were reached
LM_SEEDS = (("far_nbad", "far", 1800, "nbad"), ("far_qmax", "far", 1818, "qmax"), ("far_rho_zero", "far", 1820, "rho_zero"),
            ("truth_nbad", "truth", 1801, "nbad"), ("truth_qmax", "truth", 1800, "qmax"), ("truth_rho_zero", "truth", 1802, "rho_zero"),
            ("noisy_nbad", "noisy", 1801, "nbad"), ("noisy_qmax", "noisy", 1800, "qmax"), ("three_iterations", "three", 1802, "iterations"))


def lm_cases():
    out = []
    for name, kind, seed, exit_ in LM_SEEDS:
        s, T0 = lm_problem(kind, seed)
        out.append(s.case(name, "lm", "%s start; some optimize() call leaves by %s" % (kind, exit_), T0=T0, exit=exit_))
    return out


# ================================================================================================ all of them, and their certification
_CACHE = {}


def all_cases():
    if "cases" not in _CACHE:
        _CACHE["cases"] = gate_cases() + list_cases() + [info_case()] + uright_cases() + rounds_cases() + lm_cases()
        assert len({c["name"] for c in _CACHE["cases"]}) == len(_CACHE["cases"])
    return _CACHE["cases"]


def by_name(name):
    return next(c for c in all_cases() if c["name"] == name)


def solve(oracle, c, order=None, trace=True, **kw):
    """The oracle on case c with its keypoints in `order` (a permutation; g2o adds and sums the edges in keypoint order); per-keypoint
    results come back in the case's own order"""
    if order is None:
        order = np.arange(len(c["kps"]))
    r = oracle.pose_optimization(c["kps"][order], c["has"][order], c["Xw"][order], INV_SIGMA2, c["K"], c["T0"], u_right=c["uright"][order],
                                 bf=c["bf"], trace=trace, **kw)
    back = np.empty_like(order)
    back[order] = np.arange(len(order))
    r["outlier"] = r["outlier"][back]
    if trace:
        r["round_outlier"], r["chi2"] = r["round_outlier"][:, back], r["chi2"][back]
    return r


def counts(r):
    return (int(r["info"][2]), int(r["info"][3]), int(r["info"][4]), tuple(int(x) for x in r["round_its"]),
            tuple(int(x) for x in r["round_trials"]), tuple(r["round_exit"]))


def certify(oracle, c):
    """The case in its own edge order and in N_ORDERS seeded permutations: dict(ref = the given order's traced result, flags_stable,
    pose_spread, chi2_margin = the smallest |chi2 - threshold| / threshold over the edges, chi2_spread = the largest (max - min over
    the orders) / threshold, chi2_ok = every edge's own distance is >= MARGIN x its own spread, count_stable).  Cached."""
    key = ("cert", c["name"])
    if key in _CACHE:
        return _CACHE[key]
    nkp = len(c["kps"])
    rng = np.random.default_rng(9000 + sum(map(ord, c["name"])))
    runs = [solve(oracle, c)] + [solve(oracle, c, rng.permutation(nkp)) for _ in range(N_ORDERS)]
    ref = runs[0]
    has = c["has"]
    thr = np.where(c["uright"] < 0, CHI2_MONO, CHI2_STEREO).astype(np.float64)
    out = dict(ref=ref, flags_stable=all(np.array_equal(r["round_outlier"], ref["round_outlier"]) and np.array_equal(r["outlier"], ref["outlier"])
                                         for r in runs),
               pose_spread=max(np.abs(r["T"] - ref["T"]).max() for r in runs),
               count_stable=all(counts(r) == counts(ref) for r in runs), chi2_margin=np.inf, chi2_spread=0.0, chi2_ok=True)
    if has.any() and ref["info"][2] > 0:
        chi = np.stack([r["chi2"].astype(np.float64) for r in runs])[:, has]
        dist = np.abs(chi - thr[has]).min(0) / thr[has]
        spread = (chi.max(0) - chi.min(0)) / thr[has]
        out.update(chi2_margin=float(dist.min()), chi2_spread=float(spread.max()), chi2_ok=bool((dist >= MARGIN * spread).all()))
    _CACHE[key] = out
    return out


def notices(oracle, c, counterfactual):
    """Would a device that got `counterfactual` wrong (oracle.COUNTERFACTUALS) fail this case's assertions?  Its flags or counts
    differ from the certified ones, its pose is more than 2 POSE_TOL away (it cannot be within POSE_TOL of both), or -- for a
    count-stable case only -- its iterations / trials differ."""
    cert = certify(oracle, c)
    ref, r = cert["ref"], solve(oracle, c, counterfactual=counterfactual)
    return bool(not np.array_equal(r["outlier"], ref["outlier"]) or r["info"][:3].tolist() != ref["info"][:3].tolist() or
                np.abs(r["T"] - ref["T"]).max() > 2 * POSE_TOL or (cert["count_stable"] and counts(r) != counts(ref)))


def quaternion_round_trip(T):
    """Converter::toSE3Quat then SE3Quat::to_homogeneous_matrix on a pose whose rotation has a positive trace"""
    m = np.asarray(T, np.float64)[:3, :3]
    t = np.sqrt(m[0, 0] + m[1, 1] + m[2, 2] + 1.0)
    q = np.array([(m[2, 1] - m[1, 2]) * (0.5 / t), (m[0, 2] - m[2, 0]) * (0.5 / t), (m[1, 0] - m[0, 1]) * (0.5 / t), 0.5 * t])
    q /= np.sqrt(q @ q)
    x, y, z, w = q
    out = np.eye(4)
    out[:3, :3] = [[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                   [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                   [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]]
    out[:3, 3] = np.asarray(T)[:3, 3]
    return out


def device_inputs(c):
    """What the case is on the device: (kps, desc, last-frame dict for set_last, match row).  The map points are stored in a
    seeded order of their own, so a keypoint's match index is not its rank among the edges."""
    idx = np.flatnonzero(c["has"])
    n = len(idx)
    slot = np.random.default_rng(77).permutation(n)                # edge k -> map point slot[k]
    Xw = np.zeros((n, 3))
    Xw[slot] = c["Xw"][idx]
    match = np.full(len(c["kps"]), -1, np.int32)
    match[idx] = slot
    last = dict(valid=np.ones(n, np.uint8), Xw=Xw, desc=np.zeros((n, 32), np.uint8), octave=np.zeros(n, np.int32), angle=np.zeros(n, F32),
                obs=np.ones(n, np.int32))
    return c["kps"], np.zeros((len(c["kps"]), 32), np.uint8), last, match
