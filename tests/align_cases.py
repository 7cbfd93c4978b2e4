"""Hand-built problems for ImageAlign::ComputePose (k_align), helper, no tests: small frames rendered by cameras.make_scene, points
placed by hand on the scene surface at chosen pixels, so that the branches k_align adds on top of the reference are reached on
purpose: the take-out of H terms of points that have a Jacobian but no measurement at the trial pose, the sticky visibility flags
with their stale patch rows, the +0.0f chi2 terms, n_meas == 0 with its sticky stop_, the gates of modes 2 and 3, the exits of
Optimize, and point counts on the boundaries of the chi2 chain (16 points), a wave (64) and the gather (320 indices).

tests/test_align_cases_cpu.py proves from the oracle's trace (oracle.align(..., trace=True)) that every case does what its `claim`
says and certifies it; tests/test_align_cases_gpu.py runs all cases of a mode and frame size as the frames of one launch.

A case is a dict: name, group, claim, size (w, h), ref, cur (uint8 images), Xw [n, 3], valid [n], n_last (what the device is told
the arrays' length is; flags at or above it are set in some cases and must be ignored), T_ref, T0, mode.  The frames are 320 x 240
behind the (300, 1.2, 8, 20) extractor (level 4 is 154 x 116) and, for the sticky case alone, STICKY_SIZE (110 x 240).  The camera is
K = (250, 250, w / 2, h / 2); T_ref is the identity, as cameras.make_scene renders it.

Seeds and offsets below were found by seeded searches on the host (the search functions are kept: `search_exits`); what each case
is claimed to show is re-derived from the trace by the CPU test, so a change of the renderer or the oracle that moves a case off
its claim fails there and not silently."""
import numpy as np

import cameras as CM
from sdslam_amd.synth import intersect_surface, se3_exp

W, H = 320, 240
CFG = (300, 1.2, 8, 20)
POSE_TOL = 1e-5                   # the device bound of tests/test_track_gpu.py
CERT_TOL = 1e-7                   # certification: poses across H orders and point orders agree 100 times below it
N_ORDERS = 5
MARGIN = 1e-5                     # every comparison a decision reads is off equality by this much, relative
# The largest pose difference tests/test_align_cases_cpu.py::test_noise_floor measures over all cases between the reference's and
# the device's order of forming H and over N_ORDERS point orders, rounded up.
NOISE_FLOOR = 2e-11               # measured 1.6e-11 (count_3: three points leave H badly conditioned); 1e-13 and less elsewhere


def camera(size=(W, H)):
    w, h = size
    return CM.Camera("align%dx%d" % (w, h), tuple(CM.f32(v) for v in (250.0, 250.0, 0.5 * w, 0.5 * h)), None, (0.0, float(w), 0.0, float(h)))


MOTION = ((0.02, -0.01, 0.015), (0.4, -0.3, 0.5))                  # cameras.MOTIONS[0]
NEAR = se3_exp((0.003, -0.002, 0.001), (0.05, 0.02, -0.04))       # cameras.START: the usual perturbed start


def scene(seed, upsilon=MOTION[0], omega=MOTION[1], size=(W, H)):
    return CM.make_scene(seed, camera(size), upsilon, omega, w=size[0], h=size[1])


def on_surface(uv, T=None, size=(W, H)):
    """The scene-surface points seen at pixels uv [n, 2] of a camera at pose T (identity: the reference view)"""
    T = np.eye(4) if T is None else np.asarray(T, np.float64)
    fx, fy, cx, cy = camera(size).K
    uv = np.asarray(uv, np.float64).reshape(-1, 2)
    rays = np.stack([(uv[:, 0] - cx) / fx, (uv[:, 1] - cy) / fy, np.ones(len(uv))], -1)
    R, t = T[:3, :3], T[:3, 3]
    return intersect_surface(-R.T @ t, rays @ R, 2.0)


def grid(nx, ny, size=(W, H), margin=40.0, jitter=0):
    """nx x ny reference pixels inside the frame, `margin` from its border (visible on every aligned level)"""
    w, h = size
    gx, gy = np.meshgrid(np.linspace(margin, w - margin, nx), np.linspace(margin, h - margin, ny))
    uv = np.stack([gx.ravel(), gy.ravel()], 1)
    if jitter:
        uv = uv + np.random.default_rng(jitter).uniform(-6, 6, uv.shape)
    return uv


def case(name, group, claim, sc, Xw, T0, mode=0, valid=None, n_last=None, size=(W, H), **extra):
    Xw = np.ascontiguousarray(Xw, np.float64)
    valid = np.ones(len(Xw), np.uint8) if valid is None else np.asarray(valid, np.uint8)
    assert len(valid) == len(Xw) and np.isfinite(Xw).all()
    return dict(name=name, group=group, claim=claim, size=size, ref=sc["ref"], cur=sc["cur"], Xw=Xw, valid=valid,
                n_last=len(Xw) if n_last is None else n_last, T_ref=sc["T_ref"], T0=np.asarray(T0, np.float64), mode=mode, **extra)


def taken(c):
    """The world points ImageAlign takes: the first 100 / 300 valid ones below n_last, in index order"""
    v = c["valid"][:c["n_last"]] != 0
    return c["Xw"][:c["n_last"]][v][:100 if c["mode"] in (2, 3) else 300]


# ---- the oracle on a case ----------------------------------------------------------------------------------------------------
_PYR = {}


def pyramid(O, img):
    """(levels, tables) of the oracle's extractor on `img` (cached by content)"""
    key = (img.shape, img.tobytes())
    if key not in _PYR:
        o = O.OrbOracle(*CFG)
        o.extract(img)
        _PYR[key] = ([o.level(l) for l in range(CFG[2])], o.tables())
    return _PYR[key]


def solve(O, c, order=None, trace=True, Xw=None, **kw):
    """The oracle on case c; `order` permutes the taken points (the chi2 chain and both H orders sum in point order); per-point
    flags come back in the case's own order"""
    pc, tab = pyramid(O, c["cur"])
    pr, _ = pyramid(O, c["ref"])
    X = taken(c) if Xw is None else Xw
    if order is not None:
        X = X[order]
    r = O.align(pc, pr, tab["inv_sf"], tab["sf"], X, c["T_ref"], c["T0"], camera(c["size"]).K, mode=c["mode"], trace=trace, **kw)
    if trace and order is not None:
        back = np.empty_like(order)
        back[order] = np.arange(len(order))
        for lv in r["trace"]:
            for it in lv["its"]:
                for k in ("has_jac", "visible", "measured"):
                    it[k] = it[k][back]
    return r


def level_shape(O, c, level):
    return pyramid(O, c["ref"])[0][level].shape            # (rows, cols)


def level_scale(O, c, level):
    """The scale ImageAlign multiplies with on `level`: inv_sf[level], in mode 3 (float)(1.0 / sf[level])"""
    tab = pyramid(O, c["ref"])[1]
    return np.float32(1.0 / np.float64(tab["sf"][level])) if c["mode"] == 3 else np.float32(tab["inv_sf"][level])


def decisions(r):
    return (r["ok"], tuple(int(i) for i in r["iters"]), tuple((lv["level"], lv["exit"], tuple(it["decision"] for it in lv["its"])) for lv in r["trace"]))


# ================================================================================================ helpers of the builders
def project(X, T, size=(W, H)):
    """Level-0 pixel (u, v) and camera z of world points at pose T, in double"""
    fx, fy, cx, cy = camera(size).K
    Xc = np.asarray(X, np.float64) @ T[:3, :3].T + T[:3, 3]
    return fx * Xc[:, 0] / Xc[:, 2] + cx, fy * Xc[:, 1] / Xc[:, 2] + cy, Xc[:, 2]


def first_trial_pose(r, level):
    """The trial pose of the first iteration of `level` in a traced result (None if the level did not run)"""
    for lv in r["trace"]:
        if lv["level"] == level:
            return lv["its"][0]["pose"]
    return None


def accepted(it):
    return it["decision"] in ("accept", "small", "converged")


def taken_out(r):
    """[(level, iteration, number of points with a Jacobian and no measurement, number with a Jacobian, accepted)]"""
    return [(lv["level"], k, int((it["has_jac"] & ~it["measured"]).sum()), int(it["has_jac"].sum()), accepted(it))
            for lv in r["trace"] for k, it in enumerate(lv["its"])]


# ================================================================================================ 1. same image
def same_image_case():
    sc = dict(scene(30))
    sc["cur"] = sc["ref"]
    return case("same_image", "exits", "cur == ref at T0 == T_ref: every level converges (error_ <= 1e-10) after one iteration, chi2 == 0, error == 0",
                sc, on_surface(grid(8, 5)), np.eye(4))


# ================================================================================================ 2. exits of Optimize
def exit_problem(seed):
    """A 40-point problem whose scene, start and points are drawn from `seed`"""
    rng = np.random.default_rng(seed)
    sc = scene(30 + seed % 4)
    start = se3_exp(rng.uniform(-0.03, 0.03, 3), rng.uniform(-0.6, 0.6, 3))
    uv = np.stack([rng.uniform(30, W - 30, 40), rng.uniform(30, H - 30, 40)], 1)
    return sc, on_surface(uv), start @ sc["T_cur"]


def search_exits(O, seeds=range(200)):
    """{(level, exit): [seeds]} over exit_problem(seed), certified ones only; the key (level, 'iterations') is the 30-iteration exit"""
    out = {}
    for s in seeds:
        sc, X, T0 = exit_problem(s)
        c = case("exit_%d" % s, "exits", "", sc, X, T0)
        if not certify(O, c, cache=False)["ok"]:
            continue
        for lv in solve(O, c)["trace"]:
            out.setdefault((lv["level"], lv["exit"]), []).append(s)
    return out


# seeds 0 .. 199 of exit_problem were searched: every level ends by rollback_chi2 and by small in some certified problem (and by
# converged in same_image); NO seed ran a level through all 30 iterations -- the longest level took 10 -- so that exit is not forced.
EXIT_SEEDS = {(4, "rollback_chi2"): 0, (3, "rollback_chi2"): 0, (2, "rollback_chi2"): 0, (4, "small"): 2, (3, "small"): 2, (2, "small"): 2}


def exit_cases():
    out, seen = [], set()
    for (level, ex), s in sorted(EXIT_SEEDS.items()):
        if s in seen:
            continue
        seen.add(s)
        sc, X, T0 = exit_problem(s)
        out.append(case("exit_seed%d" % s, "exits", "a level ends by " + ", ".join("%s at level %d" % (e, l) for (l, e), t in sorted(EXIT_SEEDS.items()) if t == s),
                        sc, X, T0, exits=[(l, e) for (l, e), t in EXIT_SEEDS.items() if t == s]))
    return out


# ================================================================================================ 3. current-frame clips
ZOOM = dict(upsilon=(0.0, 0.0, -0.1), omega=(0.1, -0.1, 0.2))      # the camera moves 10 cm towards the surface: the current view is 5 % larger
SIDES = ("left", "top", "right", "bottom")


def _border_pixels(O, c0, level, frac=0.5):
    """Level-0 pixels of the CURRENT view just inside (measured) and just outside (clipped) the clip of `level` on each side:
    [(side, measured, (u, v))]; floor(u s) == 3 / 2 at the low sides, floor(u s) + 3 == cols - 1 / cols at the high sides, `frac` of a
    level pixel from flipping; the other coordinate differs per level and side so that no two patches overlap"""
    rows, cols = level_shape(O, c0, level)
    s = float(level_scale(O, c0, level))
    w, h = c0["size"]
    k = (4 - level) * 0.12
    out = []
    for side in SIDES:
        for measured in (True, False):
            if side in ("left", "top"):
                t = ((3 if measured else 2) + frac) / s
            else:
                n = cols if side in ("left", "right") else rows
                t = ((n - 4 if measured else n - 3) + frac) / s
            m = (0.3 + k + (0.06 if measured else 0.0))
            out.append((side, measured, (t, m * h) if side in ("left", "right") else (m * w, t)))
    return out


def clip_cur_first_case(O):
    """16 interior points and, per aligned level and side, a pair placed through the FIRST trial pose of that level: one just measured,
    one just clipped in the current level while visible in the reference level (the view is 5 % larger, so the reference projection
    lies further inside).  The trial poses of levels 3 and 2 are the outcome of the levels before: the pairs are placed level by level
    from the traced poses and the whole case is solved again, until the poses stop moving (four rounds)."""
    sc = scene(31, **ZOOM)
    base = on_surface(grid(4, 4, margin=70.0))
    T0 = NEAR @ sc["T_cur"]
    pairs, meta = {}, {}
    for _ in range(4):
        levels = [l for l in (4, 3, 2) if l in pairs]
        roles = [None] * len(base) + [(l, side, m) for l in levels for side, m, _ in meta[l]]
        c = case("clip_cur_first", "clips", "per level and side a pair: has a Jacobian and is just clipped / just measured at the level's first trial pose",
                 sc, np.concatenate([base] + [pairs[l] for l in levels]), T0, roles=roles)
        r = solve(O, c)
        for l in (4, 3, 2):
            P = T0 if l == 4 else first_trial_pose(r, l)
            if P is None:
                break
            meta[l] = _border_pixels(O, c, l)
            pairs[l] = on_surface([uv for _, _, uv in meta[l]], P)
    return c


def clip_cur_later_case(O):
    """The current view is the reference shifted 2.4 level-4 pixels to the left, and the start lies 1.2 level-4 pixels to the right of
    the reference.  Twelve points just inside the left clip of the reference level 4 are measured at the start and leave the level
    while the pose converges; twelve just inside its right clip start clipped and enter."""
    sc = scene(32, upsilon=(-0.04, 0.0, 0.0), omega=(0.0, 0.0, 0.0))
    T0 = se3_exp((0.06, 0.0, 0.0), (0, 0, 0)) @ sc["T_cur"]
    c0 = case("x", "clips", "", sc, on_surface(grid(4, 4, margin=70.0)), T0)
    rows, cols = level_shape(O, c0, 4)
    s = float(level_scale(O, c0, 4))
    uv = [(t / s, (0.1 + 0.066 * k) * H) for k, t in enumerate(np.linspace(3.1, 5.3, 12))] + \
         [(t / s, (0.13 + 0.066 * k) * H) for k, t in enumerate(np.linspace(cols - 4.1, cols - 3.1, 12))]
    X = np.concatenate([on_surface(grid(4, 4, margin=70.0)), on_surface(uv)])
    return case("clip_cur_later", "clips", "a point measured at iteration k is unmeasured at k + 1, k + 1 accepted; another re-enters", sc, X, T0)


def clip_share_case(kind):
    """n_out of 40 points sit in the band along the four borders that the reference sees and the 5 % larger current view does not"""
    n_out = dict(few=2, half=20, most=32)[kind]
    sc = scene(33, **ZOOM)
    per = [n_out // 4 + (1 if k < n_out % 4 else 0) for k in range(4)]
    uv = []
    for side, n in zip(SIDES, per):
        for k in range(n):
            a = (k + 1.0) / (n + 1.0)
            uv.append(dict(left=(8.0, 20 + a * (H - 40)), right=(W - 9.0, 20 + a * (H - 40)), top=(30 + a * (W - 60), 8.0), bottom=(30 + a * (W - 60), H - 9.0))[side])
    inner = grid(8, 5, margin=60.0)[:40 - n_out] if n_out < 32 else grid(4, 2, margin=80.0)
    X = np.concatenate([on_surface(uv), on_surface(inner)])
    return case("clip_share_" + kind, "clips", "%d of 40 points with a Jacobian are unmeasured on an accepted iteration" % n_out, sc, X, NEAR @ sc["T_cur"], n_out=n_out)


# ================================================================================================ 4. sticky visibility
def sticky_sizes(max_w=400):
    """Frame widths at height 240 that the extraction plan accepts and at which (cols_c - 3) sf_c > (cols_f - 3) sf_f for a coarser
    level c and the next finer level f = c - 1 leaves room for a point: [(w, c, u_lo, u_hi)] with floor(u s_c) + 3 < cols_c and
    floor(u s_f) + 3 >= cols_f for u in [u_lo, u_hi]"""
    from sdslam_amd import capi
    sc = {l: np.float64(np.float32(1.0) / np.float32(1.2) ** l) for l in (4, 3, 2)}
    out = []
    for w in range(64, max_w):
        try:
            lv = capi.plan_info(*CFG, w, H)["levels"]
        except Exception:       # noqa: BLE001 -- the plan refuses the size
            continue
        us = np.arange(w - 30, w, 0.01)
        for c in (4, 3):
            ok = (np.floor((us * sc[c]).astype(np.float32)) + 3 < lv[c, 0]) & (np.floor((us * sc[c - 1]).astype(np.float32)) + 3 >= lv[c - 1, 0])
            if ok.any():
                out.append((w, c, float(us[ok].min()), float(us[ok].max())))
    return out


# sticky_sizes()[0] is (110, 3, 105.14, 105.40): level 3 is 64 wide and reaches u = 105.40, level 2 is 76 wide and reaches 105.13.  The
# stale level is then the LAST level, so what it adds to chi2 is in the result.  (The first width with a level-4 / level-3 window
# is 132; there the stale terms end with level 3 and only its accept / small decisions could show them.)
STICKY_SIZE = (110, 240)
STICKY_LEVEL = 3                  # the last level that sees the sticky points
STICKY_U = 105.27
N_STICKY = 12


def sticky_case():
    """N_STICKY points at u = 105.27 of the 110-wide frame: visible at level 3, clipped by PrecomputePatches at level 2 (no Jacobian)
    and, because the view moved 3 px to the left, still measured there against the patch rows of level 3"""
    sc = scene(34, upsilon=STICKY_MOTION, omega=(0.0, 0.0, 0.0), size=STICKY_SIZE)
    uv = [(STICKY_U, v) for v in np.linspace(24.0, 216.0, N_STICKY)]
    X = np.concatenate([on_surface(uv, size=STICKY_SIZE), on_surface(grid(4, 7, size=STICKY_SIZE, margin=24.0), size=STICKY_SIZE)])
    return case("sticky_stale_patch", "sticky", "the first N_STICKY points: visible at level 3, clipped by PrecomputePatches at level 2, still measured there (zero Jacobian)",
                sc, X, se3_exp((0.002, -0.001, 0.001), (0.03, 0.02, -0.02)) @ sc["T_cur"], size=STICKY_SIZE)


STICKY_MOTION = (-0.03, 0.0, 0.0)


def late_visible_case():
    """Points at u = 5.7 (and v = 5.7): floor(5.7 s4) = 2 clips them at level 4, floor(5.7 s3) = 3 shows them from level 3 on"""
    sc = scene(35, upsilon=(0.02, 0.02, 0.0), omega=(0.0, 0.0, 0.0))
    uv = [(5.7, 50.0), (5.7, 120.0), (5.7, 190.0), (80.0, 5.7), (160.0, 5.7), (240.0, 5.7)]
    X = np.concatenate([on_surface(uv), on_surface(grid(6, 5))])
    return case("late_visible", "sticky", "points 0 .. 5 are clipped at level 4 on the low side and visible from level 3 on", sc, X, NEAR @ sc["T_cur"])


# ================================================================================================ 5. behind the camera
def behind_ref_case():
    sc = scene(36)
    X = on_surface(grid(8, 5))
    X[::5] *= -1.0                                         # the same pixel, 1 / z < 0 at T_ref
    return case("behind_ref", "behind", "every fifth point has 1 / z < 0 at T_ref and is never visible", sc, X, NEAR @ sc["T_cur"], behind=np.arange(40) % 5 == 0)


NEAR_Z = 0.15                                              # depth of the floating points of the behind_cur and no_measurement cases


def _floating(uv, z=NEAR_Z):
    fx, fy, cx, cy = camera().K
    uv = np.asarray(uv, np.float64)
    return np.stack([(uv[:, 0] - cx) / fx * z, (uv[:, 1] - cy) / fy * z, np.full(len(uv), z)], 1)


def behind_cur_case():
    """Four points float 16 cm in front of the reference camera; the start is 40 cm ahead of the truth, so they are behind the
    camera at the trial poses (z between -0.2 and -0.3: from that start the pose does not find its way back, and a start 30 cm ahead
    walks the points through z = 0 within a few millimetres)"""
    sc = scene(37)
    X = np.concatenate([_floating(grid(2, 2, margin=100.0), 0.16), on_surface(grid(6, 6))])
    return case("behind_cur", "behind", "points 0 .. 3 are visible in the reference and behind the camera at the trial pose", sc, X,
                se3_exp((0.0, 0.0, -0.4), (0, 0, 0)) @ sc["T_cur"])


def no_measurement_cases():
    """n_meas == 0 at the first iteration of level 4.  Modes 0 and 2: every point has a Jacobian and no measurement at the start (all
    behind the camera there / all off the image), so H is taken out entirely.  Mode 3 starts at T_ref whatever T0 says, where a point
    with a Jacobian is always measured: there the points are behind / off the image in the reference too."""
    sc = scene(38)
    out = []
    for mode in (0, 2, 3):
        uv = grid(6, 5)
        if mode == 3:
            Xb, Xo = -on_surface(uv), on_surface(uv) + np.array([5.0, 0.0, 0.0])
            Tb = To = NEAR @ sc["T_cur"]
        else:
            Xb, Tb = _floating(uv), se3_exp((0.0, 0.0, -0.3), (0, 0, 0)) @ sc["T_cur"]
            Xo, To = on_surface(uv), se3_exp((3.0, 0.0, 0.0), (0, 0, 0)) @ sc["T_cur"]
        out.append(case("no_measurement_behind_m%d" % mode, "no_measurement", "n_meas == 0 at the first iteration of level 4: every point behind the camera",
                        sc, Xb, Tb, mode=mode, has_jac=mode != 3))
        out.append(case("no_measurement_off_image_m%d" % mode, "no_measurement", "n_meas == 0 at the first iteration of level 4: every point off the image",
                        sc, Xo, To, mode=mode, has_jac=mode != 3))
    # stop_ is sticky: the points of late_visible alone -- invisible at level 4, visible and measurable from level 3 on
    uv = [(5.7, v) for v in np.linspace(30, 210, 15)] + [(u, 5.7) for u in np.linspace(30, 290, 15)]
    out.append(case("no_measurement_level4_only", "no_measurement", "n_meas == 0 at level 4 only: levels 3 and 2 could measure every point, stop_ ends them",
                    scene(35, upsilon=(0.02, 0.02, 0.0), omega=(0.0, 0.0, 0.0)), on_surface(uv), NEAR @ scene(35, upsilon=(0.02, 0.02, 0.0), omega=(0.0, 0.0, 0.0))["T_cur"],
                    has_jac=False))
    return out


# ================================================================================================ 6. gates of modes 2 and 3
def gate_problem(mode, seed):
    rng = np.random.default_rng(1000 + seed)
    uv = np.stack([rng.uniform(30, W - 30, 40), rng.uniform(30, H - 30, 40)], 1)
    if mode == 2:
        sc = scene(40 + seed % 3)
        return sc, on_surface(uv), se3_exp(rng.uniform(-0.08, 0.08, 3), rng.uniform(-1.5, 1.5, 3)) @ sc["T_cur"]
    a = rng.uniform(0.2, 12.0)
    sc = scene(40 + seed % 3, upsilon=tuple(a * np.array(MOTION[0])), omega=tuple(a * np.array(MOTION[1])))
    return sc, on_surface(uv), sc["T_cur"]


# seeds 0 .. 149 of gate_problem were searched per mode; the values sit 140 % / 45 % above and 90 % / 20 % below their thresholds
GATE_SEEDS = {(2, "below"): 1, (2, "above"): 0, (3, "below"): 1, (3, "above"): 0}


def gate_cases():
    out = []
    for (mode, side), s in sorted(GATE_SEEDS.items()):
        sc, X, T0 = gate_problem(mode, s)
        out.append(case("gate_m%d_%s" % (mode, side), "gates", "mode %d: error_ after level 4 is %s %s" % (mode, side, "0.01" if mode == 2 else "0.03"),
                        sc, X, T0, mode=mode, side=side))
    return out


# ================================================================================================ 7. counts
def _scatter(n, seed):
    rng = np.random.default_rng(seed)
    return on_surface(np.stack([rng.uniform(24, W - 24, n), rng.uniform(24, H - 24, n)], 1))


def count_cases():
    sc = scene(39)
    T0 = NEAR @ sc["T_cur"]
    out = []
    for n in (3, 15, 16, 17, 64, 65):                      # the chi2 chain works in chunks of 16 points, a wave holds 64
        out.append(case("count_%d" % n, "counts", "%d points" % n, sc, _scatter(n, 500 + n), T0))
    for mode in (2, 3):
        for n in (100, 101):                               # the 101st valid point is not taken
            out.append(case("count_%d_m%d" % (n, mode), "counts", "%d valid points in mode %d, which takes 100" % (n, mode), sc, _scatter(n, 600 + n),
                            T0, mode=mode, n_valid=n))
    for mode in (0, 1):
        for n in (300, 301):
            # 690 rows of which 680 are announced: the gather walks three chunks of 320 indices.  count_300: exactly 300 flags, the last
            # one in the third chunk.  count_301: the 300th flag at index 470, mid-way through the second chunk, the 301st at 471, and
            # ten more flags in the same chunk and in the third -- none of them may be taken.
            X = _scatter(690, 700 + n)
            valid = np.zeros(690, np.uint8)
            if n == 300:
                idx = np.sort(np.random.default_rng(71).choice(660, 299, replace=False))
                valid[idx], valid[670] = 1, 1
            else:
                idx = np.sort(np.random.default_rng(72).choice(470, 299, replace=False))
                valid[idx] = 1
                valid[[470, 471, 480, 500, 620, 639, 640, 641, 660, 679]] = 1
            valid[680:] = 1                                # at or above n_last: ignored
            out.append(case("count_%d_m%d" % (n, mode), "counts", "%d and more valid flags in 680 rows, mode %d takes 300" % (n, mode), sc, X, T0, mode=mode,
                            valid=valid, n_last=680, n_valid=int(valid[:680].sum())))
    X = _scatter(120, 801)
    out.append(case("tail_flags", "counts", "50 rows announced, 70 valid rows behind them: 50 points", sc, X, T0, n_last=50, n_valid=50))
    return out


# ================================================================================================ all of them, and their certification
_CACHE = {}


def all_cases(O):
    if "cases" not in _CACHE:
        cs = [same_image_case()] + exit_cases() + [clip_cur_first_case(O), clip_cur_later_case(O)] + [clip_share_case(k) for k in ("few", "half", "most")] + \
            [sticky_case(), late_visible_case(), behind_ref_case(), behind_cur_case()] + no_measurement_cases() + gate_cases() + count_cases()
        assert len({c["name"] for c in cs}) == len(cs)
        _CACHE["cases"] = cs
    return _CACHE["cases"]


def by_name(O, name):
    return next(c for c in all_cases(O) if c["name"] == name)


def comparisons(r, mode):
    """Every comparison the decisions of a traced run read, as (what, value, threshold): new_chi2 against chi2_ and 0.99 chi2_ from
    the second iteration of a level on, error_ against 1e-10 after an accepted step, the gate value against 0.01 / 0.03.  Iterations
    that stop_ ends compare nothing that could flip."""
    out = []
    for lv in r["trace"]:
        for k, it in enumerate(lv["its"]):
            if it["decision"] == "rollback_stop":
                continue
            if k > 0:
                out.append(("chi2 L%d it%d" % (lv["level"], k), it["new_chi2"], it["chi2_before"]))
                if accepted(it):
                    out.append(("0.99 chi2 L%d it%d" % (lv["level"], k), it["new_chi2"], 0.99 * it["chi2_before"]))
            if accepted(it):
                out.append(("error L%d it%d" % (lv["level"], k), it["error"], 1e-10))
        if lv["gate"] is not None:
            out.append(("gate L%d" % lv["level"], lv["gate"], 0.01 if mode == 2 else 0.03))
    return out


def margin(r, mode):
    """The smallest relative distance from equality over comparisons(r); exact zeros on both sides of nothing (value 0 against a
    positive threshold is a distance of 1)"""
    m = np.inf
    for what, v, t in comparisons(r, mode):
        m = min(m, abs(v - t) / max(abs(v), abs(t)))
    return m


def certify(O, c, cache=True):
    """The case in the reference's and the device's order of forming H, and under N_ORDERS seeded permutations of its taken points in
    both: dict(ref = the traced result in the case's own order, same = all decisions, iters and ok equal, spread = the largest pose
    difference, margin = the smallest relative distance from equality of any comparison in any run, ok).  Cached."""
    key = ("cert", c["name"])
    if cache and key in _CACHE:
        return _CACHE[key]
    n = len(taken(c))
    rng = np.random.default_rng(4000 + sum(map(ord, c["name"])))
    orders = [None] + [rng.permutation(n) for _ in range(N_ORDERS)]
    runs = [solve(O, c, order=o, h_order=h) for o in orders for h in (0, 1)]
    ref = runs[0]
    out = dict(ref=ref, same=all(decisions(r) == decisions(ref) for r in runs), spread=max(np.abs(r["T"] - ref["T"]).max() for r in runs),
               margin=min(margin(r, c["mode"]) for r in runs))
    out["ok"] = bool(out["same"] and out["spread"] <= CERT_TOL and out["margin"] >= MARGIN)
    if cache:
        _CACHE[key] = out
    return out


def notices(O, c, counterfactual):
    """Would a device that got `counterfactual` wrong (oracle.ALIGN_COUNTERFACTUALS) fail what the GPU test asserts on this case?
    ok or iters differ, the pose is more than 2 POSE_TOL away (it cannot be within POSE_TOL of both), or error / chi2 differ by more
    than twice their relative bounds."""
    ref, r = certify(O, c)["ref"], solve(O, c, counterfactual=counterfactual)
    rel = lambda a, b: abs(a - b) / max(1.0, abs(b))
    return bool(r["ok"] != ref["ok"] or not np.array_equal(r["iters"], ref["iters"]) or np.abs(r["T"] - ref["T"]).max() > 2 * POSE_TOL or
                rel(r["error"], ref["error"]) > 2e-7 or rel(r["chi2"], ref["chi2"]) > 2e-9)
