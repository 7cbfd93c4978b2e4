"""Crafted keyframe pairs for sd_debug_triangulate (tests/test_new_points_cpu.py checks that each reaches what it claims,
tests/test_new_points_gpu.py runs them on the device), built on the host from planted 3-D points: a row is a point projected
into both keyframes, matches12[i] = i unless a case says otherwise.

Rows on either side of a threshold come from `step_pair`: one float input of the row (a keypoint coordinate, a depth) is bisected
over its bit patterns until two ADJACENT floats give different verdicts, so the pair sits one float step apart across the gate.
Stereo rows keep the margin of new_points_ref.stereo_margin above 1e-5 (asserted where they are built)."""
import numpy as np

import new_points_ref as NR
import triangulation_ref as TR
from sdslam_amd.capi import KP_DTYPE
from sdslam_amd import synth

F32, F64 = np.float32, np.float64
SCALE_FACTOR, NLEVELS = 1.2, 8
SF, SIGMA2 = TR.scale_tables(SCALE_FACTOR, NLEVELS)
CAM5 = np.array([synth.FX, synth.FY, synth.CX, synth.CY, 40.0], F32)       # mbf = 40: mb = bf / fx
T1 = synth.se3_exp((0.02, -0.01, 0.01), (0.5, -1.0, 0.8))
T2 = synth.se3_exp((-0.25, 0.02, 0.01), (0.0, 0.0, 0.0)) @ T1              # KF2 0.25 to the side of KF1
MARGIN = 1e-5


class _camera:
    """with _camera(cam5): the builders below read the module's CAM5 when they run; a case built under another camera is built
    inside this block (None: today's camera)."""

    def __init__(self, cam5):
        self.cam5 = cam5

    def __enter__(self):
        global CAM5
        self.saved = CAM5
        if self.cam5 is not None:
            CAM5 = np.asarray(self.cam5, F32)

    def __exit__(self, *exc):
        global CAM5
        CAM5 = self.saved
        return False


def project(T, X):
    """(u, v, z) of a world point, float64 (the cases round it to float keypoints)."""
    c = np.asarray(T, F64)[:3, :3] @ np.asarray(X, F64) + np.asarray(T, F64)[:3, 3]
    fx, fy, cx, cy = [F64(v) for v in CAM5[:4]]
    return fx * c[0] / c[2] + cx, fy * c[1] / c[2] + cy, c[2]


def world_point(T, u, v, z):
    fx, fy, cx, cy = [F64(v_) for v_ in CAM5[:4]]
    T = np.asarray(T, F64)
    return T[:3, :3].T @ (np.array([(u - cx) * z / fx, (v - cy) * z / fy, z]) - T[:3, 3])


class Pair:
    """Rows of one keyframe pair.  Each row: both keypoints (undistorted and raw), octaves, mvuRight / mvDepth of both sides."""

    def __init__(self, name, Ta=T1, Tb=T2, monocular=True, median=-1.0):
        self.name, self.T1, self.T2, self.monocular, self.median = name, np.asarray(Ta, F64), np.asarray(Tb, F64), monocular, median
        self.rows, self.extra2, self.claims = [], [], {}

    def row(self, X=None, uv1=None, uv2=None, oct1=0, oct2=0, ur1=-1.0, z1=-1.0, ur2=-1.0, z2=-1.0, raw1=None, raw2=None, claim=None,
            match=True):
        if X is not None:
            p1, p2 = project(self.T1, X), project(self.T2, X)
            uv1 = uv1 if uv1 is not None else p1[:2]
            uv2 = uv2 if uv2 is not None else p2[:2]
            if ur1 == "exact":
                ur1, z1 = p1[0] - F64(CAM5[4]) / p1[2], p1[2]
            if ur2 == "exact":
                ur2, z2 = p2[0] - F64(CAM5[4]) / p2[2], p2[2]
        self.rows.append(dict(uv1=uv1, uv2=uv2, oct1=oct1, oct2=oct2, ur1=ur1, z1=z1, ur2=ur2, z2=z2, raw1=raw1 or uv1, raw2=raw2 or uv2,
                              match=match))
        if claim is not None:
            self.claims[len(self.rows) - 1] = claim
        return len(self.rows) - 1

    def build(self):
        n = len(self.rows)

        def kps(key, okey):
            k = np.zeros(n, KP_DTYPE)
            k["size"], k["response"], k["class_id"] = 31.0, 50.0, -1
            k["x"], k["y"] = [F32(r[key][0]) for r in self.rows], [F32(r[key][1]) for r in self.rows]
            k["octave"] = [r[okey] for r in self.rows]
            return k
        col = lambda key: np.array([r[key] for r in self.rows], F32)
        m = np.array([i if r["match"] else -1 for i, r in enumerate(self.rows)], np.int32)
        return dict(name=self.name, k1u=kps("uv1", "oct1"), k1=kps("raw1", "oct1"), k2u=kps("uv2", "oct2"), k2=kps("raw2", "oct2"),
                    ur1=col("ur1"), z1=col("z1"), ur2=col("ur2"), z2=col("z2"), m=m, T1=self.T1, T2=self.T2, cam5=CAM5, sf=SF,
                    sigma2=SIGMA2, scale_factor=SCALE_FACTOR, monocular=self.monocular, median=self.median, claims=dict(self.claims))


def reference(c, margins=None):
    return NR.triangulate(c["k1u"], c["k1"], c["ur1"], c["z1"], c["k2u"], c["k2"], c["ur2"], c["z2"], c["m"], c["T1"], c["T2"], c["cam5"],
                          c["sf"], c["sigma2"], c["scale_factor"], c["monocular"], c["median"], margins)


def verdict_of(make_row, p, Tb=T2, monocular=True):
    """Verdict and branch of the single row make_row(pair, p) adds to a pair (T1, Tb)."""
    pr = Pair("probe", T1, Tb, monocular)
    make_row(pr, F32(p))
    v, b, _ = reference(pr.build())
    return int(v[0]), int(b[0])


def step_pair(make_row, lo, hi):
    """Adjacent floats (p_lo, p_hi) between lo and hi with verdict_of(p_lo) == verdict_of(lo) != verdict_of(p_hi)."""
    lo, hi = F32(lo), F32(hi)
    v_lo, v_hi = verdict_of(make_row, lo)[0], verdict_of(make_row, hi)[0]
    assert v_lo != v_hi, (float(lo), float(hi), v_lo, v_hi)
    a, b = int(lo.view(np.int32)), int(hi.view(np.int32))
    assert (a >= 0) == (b >= 0)
    while abs(b - a) > 1:
        mid = (a + b) // 2
        if verdict_of(make_row, np.int32(mid).view(F32))[0] == v_lo:
            a = mid
        else:
            b = mid
    p_lo, p_hi = np.int32(a).view(F32), np.int32(b).view(F32)
    v_hi = verdict_of(make_row, p_hi)[0]                    # the gate next to `lo`, whichever `hi` itself ends at
    assert verdict_of(make_row, p_lo)[0] == v_lo != v_hi
    return p_lo, p_hi, v_lo, v_hi


# ------------------------------------------------------------------------------------------------ the cases
X0 = world_point(T1, 300.0, 200.0, 3.0)                  # a well-conditioned point: parallax 0.25 / 3


def thresholds_case(cam5=None):
    with _camera(cam5):
        return _thresholds_case()


def _thresholds_case():
    """Every gate of the mono path with a twin one float step away, and the plain rows of every verdict."""
    pr = Pair("thresholds")
    pr.row(X0, claim=(NR.ACCEPTED, NR.BR_SVD))
    pr.row(X0, match=False, claim=(NR.NO_MATCH, NR.BR_NONE))
    pr.row(world_point(T1, 320.0, 240.0, 400.0), claim=(NR.LOW_PARALLAX, NR.BR_NONE))
    u2 = project(T2, X0)
    pr.row(uv1=project(T1, X0)[:2], uv2=(u2[0] + 120.0, u2[1]), claim=(NR.Z1, NR.BR_SVD))       # disparity of the wrong sign: behind both
    pr.row(X0, uv1=(project(T1, X0)[0], project(T1, X0)[1] + 9.0), claim=(NR.REPROJ1, NR.BR_SVD))
    pr.row(X0, oct1=0, oct2=5, claim=(NR.SCALE, NR.BR_SVD))
    pr.row(X0, oct1=5, oct2=0, claim=(NR.SCALE, NR.BR_SVD))
    movers = {
        # 0.9998: KF2's keypoint slides along its (horizontal) epipolar line towards the zero-parallax position
        "parallax": (lambda p, x: p.row(X0, uv2=(x, project(T2, X0)[1])), project(T2, X0)[0], project(T2, world_point(T1, 300.0, 200.0, 60.0))[0]),
        # 5.991 * sigma2 in KF1 / KF2: one keypoint moves off the epipolar plane
        "reproj1": (lambda p, y: p.row(X0, uv1=(project(T1, X0)[0], y)), project(T1, X0)[1], project(T1, X0)[1] + 9.0),
        "reproj2": (lambda p, y: p.row(X0, uv2=(project(T2, X0)[0], y), oct1=2, oct2=0), project(T2, X0)[1], project(T2, X0)[1] + 12.0),
        # ratioDist against ratioOctave * ratioFactor: the point moves along KF1's ray, towards KF2's side
        "scale": (lambda p, z: p.row(world_point(T1, 320.0, 240.0, z), oct1=0, oct2=1), 3.0, 0.15),
    }
    steps = {}
    for name, (mk, lo, hi) in movers.items():
        p_lo, p_hi, v_lo, v_hi = step_pair(mk, lo, hi)
        mk(pr, p_lo)
        pr.claims[len(pr.rows) - 1] = (v_lo, None)
        mk(pr, p_hi)
        pr.claims[len(pr.rows) - 1] = (v_hi, None)
        steps[name] = (v_lo, v_hi)
    c = pr.build()
    c["steps"] = steps
    return c


def stereo_case(cam5=None):
    with _camera(cam5):
        return _stereo_case()


def _stereo_case():
    """Both unproject branches, the stereo reprojection forms (KF2's with KF1's mbf), mvuRight == 0, mvDepth <= 0, and the
    `if (bStereo1) ... else if (bStereo2)` asymmetry: with both sides stereo only KF1's cosine is computed."""
    Tf = synth.se3_exp((0.0, 0.0, -0.3), (0.0, 0.0, 0.0)) @ T1                  # KF2 0.3 ahead of KF1 (> mb: the slot is not gated)
    pr = Pair("stereo", T1, Tf, monocular=False)
    far = world_point(T1, 325.0, 243.0, 5.0)               # next to the direction of motion: less parallax than the stereo pair's
    X0 = world_point(T1, 600.0, 400.0, 1.0)                # far from it: more
    pr.row(far, ur1="exact", claim=(NR.ACCEPTED, NR.BR_UNPROJECT1))
    pr.row(far, ur2="exact", claim=(NR.ACCEPTED, NR.BR_UNPROJECT2))
    pr.row(far, ur1="exact", ur2="exact", claim=(NR.ACCEPTED, NR.BR_UNPROJECT1))
    pr.row(X0, ur1="exact", claim=(NR.ACCEPTED, NR.BR_SVD))                     # wide parallax: triangulated although stereo
    pr.row(X0, ur2="exact", claim=(NR.ACCEPTED, NR.BR_SVD))
    p1, p2 = project(T1, X0), project(Tf, X0)
    pr.row(X0, ur1=p1[0] - 40.0 / p1[2] + 6.0, z1=p1[2], claim=(NR.REPROJ1, NR.BR_SVD))       # only the right coordinate is off
    pr.row(X0, ur2=p2[0] - 40.0 / p2[2] + 6.0, z2=p2[2], claim=(NR.REPROJ2, NR.BR_SVD))
    pr.row(X0, ur1=0.0, z1=p1[2], claim=(NR.REPROJ1, NR.BR_SVD))                # mvuRight == 0 is stereo: 7.8 and the right error
    # mvDepth <= 0: atan2 >= pi / 2, so cos <= -1 + and x3D = 0, which lies in front of KF1 only (tcw z = 0.01 and -0.29)
    pr.row(far, ur1=0.0, z1=0.0, claim=(NR.Z2, NR.BR_UNPROJECT1))
    pr.row(far, ur2=project(Tf, far)[0] - 1.0, z2=-1.0, claim=(NR.Z2, NR.BR_UNPROJECT2))
    raw = (project(T1, far)[0] + 3.0, project(T1, far)[1] - 2.0)                # UnprojectStereo reads the DISTORTED keypoint
    pr.row(far, ur1="exact", raw1=raw, oct1=3, oct2=3, claim=(NR.ACCEPTED, NR.BR_UNPROJECT1))
    # the stereo cosine against cosParallaxRays, one float step of mvDepth apart: unproject <-> triangulate
    mk = lambda p, z: p.row(X0, ur1=p1[0] - 40.0 / p1[2], z1=z)
    lo, hi = F32(p1[2]), F32(0.05)

    def branch_flip(a, b):
        ia, ib = int(F32(a).view(np.int32)), int(F32(b).view(np.int32))
        ba = verdict_of(mk, a, Tf, False)[1]
        while abs(ib - ia) > 1:
            mid = (ia + ib) // 2
            if verdict_of(mk, np.int32(mid).view(F32), Tf, False)[1] == ba:
                ia = mid
            else:
                ib = mid
        return np.int32(ia).view(F32), np.int32(ib).view(F32)
    z_svd, z_unp = branch_flip(lo, hi)
    # the flip itself sits inside the margin by construction: keep the two rows 1 % of the depth either side of it
    mk(pr, F32(z_svd * F32(1.01)))
    pr.claims[len(pr.rows) - 1] = (None, NR.BR_SVD)
    mk(pr, F32(z_unp * F32(0.99)))
    pr.claims[len(pr.rows) - 1] = (None, NR.BR_UNPROJECT1)
    return pr.build()


def degenerate_case():
    """A with a zero column.  Column 3 (both cameras at the origin): x3D = (0, 0, 0, 1), a rank-deficient A that ends at z1 <= 0.
    Column 2 (third column of both rotations zero, which no rigid pose has; the debug entry takes any matrix): x3D[3] == 0."""
    out = []
    Ta = np.eye(4)
    Tb = synth.se3_exp((0.0, 0.0, 0.0), (0.0, 12.0, 0.0))
    pr = Pair("rank_deficient", Ta, Tb)
    pr.row(uv1=(300.0, 200.0), uv2=(350.0, 260.0), claim=(NR.Z1, NR.BR_SVD))
    out.append(pr.build())
    Ta, Tb = np.eye(4), np.eye(4)
    Ta[2, 2] = Tb[2, 2] = 0.0
    Tb[0, 3] = -0.25
    pr = Pair("w_zero", Ta, Tb)
    pr.row(uv1=(400.0, 300.0), uv2=(450.0, 280.0), claim=(NR.W_ZERO, NR.BR_SVD))
    out.append(pr.build())
    return out


def gate_cases():
    """The neighbour gate: mono on baseline / median against 0.01 (one float step of the median apart, and switched off),
    otherwise baseline against mb."""
    out = []
    P1, P2 = NR.Pose(T1), NR.Pose(T2)
    baseline = NR.norm3f(P2.Ow - P1.Ow)
    med = F32(baseline / F32(0.01))
    cands = [med]
    for _ in range(4):
        cands = [np.nextafter(cands[0], F32(0))] + cands + [np.nextafter(cands[-1], F32(np.inf))]
    gated = [bool(F64(F32(baseline / m)) < F64(0.01)) for m in cands]
    k = gated.index(True)
    assert 0 < k and not gated[k - 1]
    for name, median, mono, want in (("gate_mono_open", cands[k - 1], True, NR.ACCEPTED), ("gate_mono_shut", cands[k], True, NR.SLOT_GATED),
                                     ("gate_mono_off", -1.0, True, NR.ACCEPTED), ("gate_stereo_open", 1e9, False, NR.ACCEPTED)):
        pr = Pair(name, monocular=mono, median=float(median))
        pr.row(X0, claim=(want, None))
        pr.row(X0, match=False, claim=(NR.NO_MATCH, NR.BR_NONE))
        out.append(pr.build())
    Tn = synth.se3_exp((-0.05, 0.0, 0.0), (0.0, 0.0, 0.0)) @ T1            # baseline 0.05 < mb = 40 / fx
    assert 0.05 < float(CAM5[4] / CAM5[0])
    pr = Pair("gate_stereo_shut", T1, Tn, monocular=False)
    pr.row(X0, claim=(NR.SLOT_GATED, NR.BR_NONE))
    out.append(pr.build())
    pr = Pair("own_centre", np.eye(4), synth.se3_exp((-0.25, 0.0, 0.0), (0.0, 0.0, 0.0)))
    # KF1 at the origin sees its own centre through a stereo keypoint of depth 0: x3D = 0 = Ow1, but z1 <= 0 comes first
    pr.row(uv1=(320.0, 240.0), uv2=(300.0, 240.0), ur1=0.0, z1=0.0, claim=(NR.Z1, NR.BR_UNPROJECT1))
    out.append(pr.build())
    return out


def late_gate_cases():
    """z2 <= 0 and dist == 0, which need z1 > 0 first.  Z2: KF2 stands beyond the point on KF1's ray, looking the same way (the
    rays are parallel, so KF1's depth decides: UnprojectStereo(idx1)).  DIST_ZERO: x3D = Ow1 with z1 > 0 takes a Tcw no rigid
    motion gives (Rcw = diag(1, 1, 0), tcw = (0, 0, 1): Ow = 0 and z = 1 for every point); the debug entry takes any matrix."""
    out = []
    Ta = np.eye(4)
    Tb = np.eye(4)
    X = world_point(Ta, 400.0, 300.0, 2.0)
    Tb[:3, 3] = -2.0 * X                                    # Ow2 = 2 X
    pr = Pair("z2", Ta, Tb, monocular=False)
    pr.row(uv1=(400.0, 300.0), uv2=(400.0, 300.0), ur1=400.0 - 40.0 / 2.0, z1=2.0, claim=(NR.Z2, NR.BR_UNPROJECT1))
    out.append(pr.build())
    Ta, Tb = np.diag([1.0, 1.0, 0.0, 1.0]), np.diag([1.0, 1.0, 0.0, 1.0])
    Ta[2, 3] = Tb[2, 3] = 1.0
    Tb[0, 3] = 0.25
    cx, cy, fx = float(CAM5[2]), float(CAM5[3]), float(CAM5[0])
    pr = Pair("dist_zero", Ta, Tb, monocular=False)
    pr.row(uv1=(cx + 3.0, cy), uv2=(cx + 0.25 * fx, cy), oct1=7, oct2=7, ur1=cx - 40.0, z1=0.0, claim=(NR.DIST_ZERO, NR.BR_UNPROJECT1))
    out.append(pr.build())
    return out


def count_case(n, seed, cam5=None):
    with _camera(cam5):
        return _count_case(n, seed)


def _count_case(n, seed):
    """n matched rows among 2 n + 3 keypoints (match counts 0, 1, 64, 65: none, one lane, a full wave, a wave and one lane)."""
    rng = np.random.default_rng(seed)
    pr = Pair("count_%d" % n)
    total = 2 * n + 3
    matched = set(rng.choice(total, n, replace=False).tolist())
    for i in range(total):
        X = world_point(T1, rng.uniform(40, 600), rng.uniform(40, 440), rng.uniform(1.5, 8.0))
        uv2 = project(T2, X)[:2] + rng.normal(0, 0.6, 2)
        pr.row(X, uv2=uv2, oct1=int(rng.integers(0, 8)), oct2=int(rng.integers(0, 8)), match=i in matched)
    c = pr.build()
    perm = rng.permutation(total)                           # matches12 is no identity: KF2 is shuffled
    inv = np.argsort(perm)
    for key in ("k2u", "k2", "ur2", "z2"):
        c[key] = c[key][perm]
    c["m"] = np.where(c["m"] >= 0, inv[np.maximum(c["m"], 0)], -1).astype(np.int32)
    return c


def all_cases():
    cases = [thresholds_case(), stereo_case()] + degenerate_case() + gate_cases() + late_gate_cases() + [count_case(n, 10 + n) for n in (0, 1, 64, 65)]
    assert len({c["name"] for c in cases}) == len(cases)
    return cases


_CACHE = {}


def cases_with_reference():
    """[(case, (verdict, branch, Xw), margins)], computed once per process and left unchanged."""
    if not _CACHE:
        out = []
        for c in all_cases():
            margins = []
            res = reference(c, margins)
            for a in res:
                a.setflags(write=False)
            out.append((c, res, margins))
        _CACHE["all"] = out
    return _CACHE["all"]


# ------------------------------------------------------------------------------------------------ the batched scene's stereo mix
def true_depth(T, x, y, depth=2.0):
    """mvDepth an RGB-D sensor would give the keypoints (x, y) of a view of synth's surface rendered from pose T."""
    T = np.asarray(T, F64)
    R, t = T[:3, :3], T[:3, 3]
    rays = np.stack([(np.asarray(x, F64) - synth.CX) / synth.FX, (np.asarray(y, F64) - synth.CY) / synth.FY, np.ones(len(x))], -1)
    Xw = synth.intersect_surface(-R.T @ t, rays @ R, depth)
    return (Xw @ R.T + t)[:, 2]


def batched_mix(k1, k2, T_cur, T_ref, K, bf, seed=6):
    """mvuRight / mvDepth rows [B, cap] for the six views of test_triangulation_gpu.py (k1 / k2: their keypoints, cur / ref
    side, padded to one capacity).  Per keypoint, by a draw that does not depend on the capacity: 10 % carry the surface's depth
    and disparity (accepted stereo points, either unproject branch or triangulated), 10 % a depth of 0.05 with a disparity of
    bf / 2 (stereo cosine 0.25: unproject, then rejected), on cur frames 1 and 2 (the sideways pairs, where no ray pair is
    nearly parallel) 10 % the right disparity with a depth of 400 (stereo cosine 1.0f: triangulated, stereo reprojection form),
    the rest mono; ref frame 2 has mvuRight == 0 rows.  Next to the forward pair's epipole in cur frame 0 a stereo depth of 0.2
    still reprojects within the chi-square bound in KF2 (it stands 0.25 behind) and fails the scale test: no consistent pair of
    these views does, since octaves differ by at most one level and the distance ratio stays near 1.1.
    The seed is one whose draw keeps every matched stereo row's margin above 1e-5 (tests/test_new_points_cpu.py asserts it)."""
    B, cap = k1.shape
    draw = np.random.default_rng(seed).random((2, B, 2048))[:, :, :cap]
    out = {}
    for side, (k, Ts) in enumerate(((k1, T_cur), (k2, T_ref))):
        u, z = np.full((B, cap), -1, F32), np.full((B, cap), -1, F32)
        for f in range(B):
            d, x = draw[side, f], k["x"][f]
            zt = true_depth(Ts[f], x, k["y"][f]).astype(F32)
            disp = (x - F32(bf) / zt).astype(F32)
            real, near = d < 0.1, (d >= 0.1) & (d < 0.2)
            z[f, real], u[f, real] = zt[real], disp[real]
            z[f, near], u[f, near] = F32(0.05), (x - F32(bf) / F32(2.0))[near]
            if side == 0 and f > 0:
                far = (d >= 0.2) & (d < 0.3)
                z[f, far], u[f, far] = F32(400.0), disp[far]
        out["u%d" % (side + 1)], out["z%d" % (side + 1)] = u, z
    out["u2"][2, draw[1, 2] > 0.95] = 0.0
    e1, e2 = TR.epipole(T_ref[0], T_cur[0], K), TR.epipole(T_cur[0], T_ref[0], K)
    near1 = np.hypot(k1["x"][0] - e1[0], k1["y"][0] - e1[1]) < 10.0
    near2 = np.hypot(k2["x"][0] - e2[0], k2["y"][0] - e2[1]) < 15.0
    out["z1"][0, near1] = 0.2
    out["u1"][0, near1] = k1["x"][0, near1] - F32(bf) / F32(0.2)
    out["u2"][0, near2] = -1.0
    return out
