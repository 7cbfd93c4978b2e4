"""Cameras other than synth's, shared by the camera-sweep tests (helper, no tests).

Every tracking parity test calls set_camera with synth's pinhole: fx = fy = 500, the principal point at the image centre,
bounds (0, 640, 0, 480).  With that camera fx and fy, cx and cy, invW and invH (both 0.1) and `x - min_x` and `x` cannot be
told apart, no keypoint ever falls outside the frame grid, and mvKeysUn == mvKeys.  The table below holds cameras that
separate them, and the builders restate the few lines of sdslam_amd.synth that read its FX ... CY with a camera argument
(synth itself stays as it is: bench.py and the goldens depend on it).  With CAMERAS["synth"] every builder returns exactly
what synth returns; tests/test_cameras_cpu.py asserts that.

Every value is stored as float(np.float32(v)): the C ABI of set_camera takes floats, so the oracle and the Python
references are called with exactly what the device gets."""
from collections import namedtuple

import numpy as np

from sdslam_amd import synth
from sdslam_amd.synth import _bilinear, intersect_surface, make_image, se3_exp

W, H = 640, 480
Camera = namedtuple("Camera", "name K dist bounds")      # K = (fx, fy, cx, cy); dist = (k1, k2, p1, p2, k3) or None


def f32(v):
    return float(np.float32(v))


def _oracle():
    from oracle import oracle as O
    return O


def image_bounds(K, dist):
    """Frame::ComputeImageBounds: the four image corners undistorted; min_x from the two left corners, max_x from the two right
    ones, min_y from the two upper, max_y from the two lower, as float32."""
    if dist is None:
        return (0.0, float(W), 0.0, float(H))
    c = _oracle().undistort_points(np.array([[0, 0], [W, 0], [0, H], [W, H]], np.float32), K, dist)
    return (f32(min(c[0, 0], c[2, 0])), f32(max(c[1, 0], c[3, 0])), f32(min(c[0, 1], c[1, 1])), f32(max(c[2, 1], c[3, 1])))


def _cam(name, K, dist=None, bounds=None):
    K = tuple(f32(v) for v in K)
    dist = None if dist is None else tuple(f32(v) for v in dist)
    bounds = image_bounds(K, dist) if bounds is None else tuple(f32(v) for v in bounds)
    return Camera(name, K, dist, bounds)


TUM1_K, TUM1_DIST = (517.3, 516.5, 318.6, 255.3), (0.2624, -0.9531, -0.0054, 0.0026, 1.1633)
# tum1's k1 is positive: its undistorted corners lie INSIDE the image (min_x = 10.8, min_y = 14.7), so ComputeImageBounds
# gives bounds that are not the image's and a min != 0, but not a negative one.  (A barrel lens with negative bounds, EuRoC
# cam0's, was tried: ImageAlign, which projects with the pinhole model into the distorted image, ends further from the true
# pose than it starts there, in the oracle alone, so it cannot serve as a sound case.)
# aniso: fy / fx = 1.25.  ImageAlign scales its whole Jacobian with fx alone (src/ImageAlign.cc, cam_fx_ * scale), so its v
# rows are 25 % too small here; the oracle alone still converges from the perturbed start on both scenes (asserted in
# tests/test_cameras_cpu.py), so fy = 575 stays and was not moved towards fx.
# window: aniso's K behind bounds that lie inside the image.  The extractor's keypoints keep 19 px and more from the image
# edge, so the bounds cut 60 / 50 / 40 / 30 px off: that leaves over 70 keypoints per frame outside the grid and about 90
# local-map projections between bounds and image edge (tests/test_cameras_cpu.py asserts at least 20 of each; bounds of
# (40, 610, 25, 470) leave 5 and 13).  invW = 64 / 530 != invH = 48 / 410.
WINDOW_BOUNDS = (60.0, 590.0, 40.0, 450.0)
CAMERAS = {c.name: c for c in (
    _cam("synth", (synth.FX, synth.FY, synth.CX, synth.CY)),                    # control: today's results
    _cam("aniso", (460.0, 575.0, 301.5, 262.25)),                               # fx <-> fy, cx <-> cy; ImageAlign's fx-only scale
    _cam("offaxis", (500.0, 500.0, 212.7, 305.3)),                              # cx != w/2, cy != h/2, inexact floats
    _cam("tum1", TUM1_K, TUM1_DIST),                                            # mvKeysUn != mvKeys, min > 0, invW != invH
    _cam("window", (460.0, 575.0, 301.5, 262.25), None, WINDOW_BOUNDS),         # min != 0, skip key, bounds inside the image
    _cam("wide", (500.0, 500.0, 212.7, 305.3), None, (-12.0, 655.0, -9.0, 490.0)),     # min < 0 (as a barrel lens gives), on offaxis' views
)}
NAMES = list(CAMERAS)


# ---- the Brown model and its inverse ------------------------------------------------------------------------------
def distort_normalised(x, y, dist):
    k1, k2, p1, p2, k3 = dist
    r2 = x * x + y * y
    rad = 1.0 + r2 * (k1 + r2 * (k2 + r2 * k3))
    return x * rad + 2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x), y * rad + p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y


def undistort_normalised(xd, yd, dist, tol=1e-10, max_iters=200):
    """The undistorted normalised point of a distorted one by fixed-point iteration in float64 (the contraction factor of
    TUM1's coefficients is about 0.5 at the image corners)."""
    k1, k2, p1, p2, k3 = dist
    x, y = xd.copy(), yd.copy()
    for _ in range(max_iters):
        r2 = x * x + y * y
        rad = 1.0 + r2 * (k1 + r2 * (k2 + r2 * k3))
        xn = (xd - (2.0 * p1 * x * y + p2 * (r2 + 2.0 * x * x))) / rad
        yn = (yd - (p1 * (r2 + 2.0 * y * y) + 2.0 * p2 * x * y)) / rad
        step = max(np.abs(xn - x).max(), np.abs(yn - y).max())
        x, y = xn, yn
        if step < tol:
            break
    return x, y


_RAYS = {}


def pixel_rays(cam, w=W, h=H):
    """Camera-frame rays (x, y, 1) through the centres of the pixel grid: ((u - cx) / fx, (v - cy) / fy, 1) without
    distortion, the undistorted normalised point of the pixel with it."""
    key = (cam.K, cam.dist, w, h)
    if key not in _RAYS:
        fx, fy, cx, cy = cam.K
        v, u = np.mgrid[0:h, 0:w].astype(np.float64)
        x, y = (u - cx) / fx, (v - cy) / fy
        if cam.dist is not None:
            x, y = undistort_normalised(x, y, cam.dist)
        _RAYS[key] = np.stack([x, y, np.ones_like(u)], -1)
    return _RAYS[key]


# ---- synth's builders with the camera as an argument -----------------------------------------------------------------
def render(tex, Tcw, cam, w=W, h=H, depth=2.0):
    """synth.render_plane_view with the pixel rays of `cam`: what that lens sees of the textured surface."""
    fx, fy, cx, cy = cam.K
    R, t = Tcw[:3, :3], Tcw[:3, 3]
    rays = pixel_rays(cam, w, h)
    Rwc = R.T
    Ow = -Rwc @ t
    dw = rays @ Rwc.T
    Xw = intersect_surface(Ow, dw, depth)
    ur = fx * Xw[..., 0] / depth + cx
    vr = fy * Xw[..., 1] / depth + cy
    return _bilinear(tex, 2.0 * ur + 0.5, 2.0 * vr + 0.5)


_SCENES = {}


def make_scene(seed, cam, upsilon=(0.02, -0.01, 0.015), omega_deg=(0.4, -0.3, 0.5), w=W, h=H):
    """synth.make_scene seen through `cam` (cached: cameras with one K and distortion share their images)."""
    key = (seed, cam.K, cam.dist, tuple(upsilon), tuple(omega_deg), w, h)
    if key not in _SCENES:
        tex = make_image(seed, 2 * w, 2 * h)
        T_ref, T_cur = np.eye(4), se3_exp(upsilon, omega_deg)
        _SCENES[key] = dict(ref=render(tex, T_ref, cam, w, h), cur=render(tex, T_cur, cam, w, h), T_ref=T_ref, T_cur=T_cur, depth=2.0)
    return dict(_SCENES[key], K=cam.K)


def _kp_rays(kps_un, cam):
    fx, fy, cx, cy = cam.K
    return np.stack([(kps_un["x"].astype(np.float64) - cx) / fx, (kps_un["y"].astype(np.float64) - cy) / fy, np.ones(len(kps_un))], -1)


def backproject_on_surface(xy, cam, depth=2.0):
    fx, fy, cx, cy = cam.K
    xy = np.asarray(xy, np.float64)
    rays = np.stack([(xy[:, 0] - cx) / fx, (xy[:, 1] - cy) / fy, np.ones(len(xy))], -1)
    return intersect_surface(np.zeros(3), rays, depth)


def tracking_case(seed, ref_kps_un, ref_desc, cam, max_points=300):
    """synth.tracking_case; ref_kps_un are the UNDISTORTED keypoints of the ref view (pinhole coordinates of cam.K)."""
    n = len(ref_kps_un)
    valid = np.zeros(n, np.uint8)
    valid[:min(n, max_points)] = 1
    Xw = backproject_on_surface(np.stack([ref_kps_un["x"], ref_kps_un["y"]], 1), cam)
    return dict(valid=valid, Xw=Xw, desc=ref_desc.copy(), octave=ref_kps_un["octave"].astype(np.int32).copy(),
                angle=ref_kps_un["angle"].astype(np.float32).copy(), obs=np.ones(n, np.int32))


def keyframe_case(kps_un, desc, T_kf, cam, max_points=300):
    n = len(kps_un)
    R, t = T_kf[:3, :3], T_kf[:3, 3]
    Ow = -R.T @ t
    Xw = intersect_surface(Ow, _kp_rays(kps_un, cam) @ R, 2.0) if n else np.zeros((0, 3))
    valid = np.zeros(n, np.uint8)
    valid[:min(n, max_points)] = 1
    return dict(valid=valid, Xw=np.ascontiguousarray(Xw), desc=desc.copy(), octave=kps_un["octave"].astype(np.int32).copy(),
                angle=kps_un["angle"].astype(np.float32).copy(), obs=np.ones(n, np.int32))


def planted_matches(seed, kps_un, T_cw, cam, n_match, outlier_frac, noise_px=0.0, n_exact_inliers=None):
    fx, fy, cx, cy = cam.K
    rng = np.random.Generator(np.random.PCG64(seed))
    n = len(kps_un)
    chosen = np.sort(rng.choice(n, size=n_match, replace=False))
    n_in = int(round(n_match * (1.0 - outlier_frac))) if n_exact_inliers is None else n_exact_inliers
    inl = np.zeros(n, bool)
    inl[rng.choice(chosen, size=n_in, replace=False)] = True
    R, t = T_cw[:3, :3], T_cw[:3, 3]
    xy = np.stack([kps_un["x"], kps_un["y"]], 1).astype(np.float64)
    xy_n = xy + rng.normal(size=xy.shape) * noise_px
    z = rng.uniform(1.0, 5.0, n)
    Xc = np.stack([(xy_n[:, 0] - cx) / fx * z, (xy_n[:, 1] - cy) / fy * z, z], 1)
    Xw = (Xc - t) @ R
    bad = ~inl
    Xw[bad] = rng.uniform(-2.0, 2.0, size=(int(bad.sum()), 3)) + np.array([0, 0, 3.0])
    cm = np.full(n, -1, np.int32)
    cm[chosen] = chosen
    last = dict(valid=np.ones(n, np.uint8), Xw=np.ascontiguousarray(Xw), desc=np.zeros((n, 32), np.uint8),
                octave=kps_un["octave"].astype(np.int32).copy(), angle=kps_un["angle"].astype(np.float32).copy(), obs=np.ones(n, np.int32))
    return last, cm, inl & (cm >= 0)


def local_map_case(seed, kps_un, desc, T_cur, cam, n_extra=300, scale_factor=1.2, nlevels=8):
    rng = np.random.Generator(np.random.PCG64(seed))
    R, t = T_cur[:3, :3], T_cur[:3, 3]
    Ow = -R.T @ t
    n = len(kps_un)
    Xw = intersect_surface(Ow, _kp_rays(kps_un, cam) @ R, 2.0)
    PO = Xw - Ow
    d = np.linalg.norm(PO, axis=1)
    sf = scale_factor ** kps_un["octave"].astype(np.float64)
    mf_max = (d * sf * rng.uniform(0.85, 1.15, n)).astype(np.float32)
    mf_min = (mf_max / np.float32(scale_factor ** (nlevels - 1))).astype(np.float32)
    nrm = PO / d[:, None] + rng.normal(size=(n, 3)) * 0.25
    nrm /= np.linalg.norm(nrm, axis=1)[:, None]
    dsc = desc.copy()
    flips = rng.integers(0, 256, size=(n, 6))
    for k in range(6):
        dsc[np.arange(n), flips[:, k] // 8] ^= (1 << (flips[:, k] % 8)).astype(np.uint8)
    pts = dict(cand=np.ones(n, np.uint8), Xw=Xw, normal=nrm, min_dist=np.float32(0.8) * mf_min, max_dist=np.float32(1.2) * mf_max,
               mf_max_dist=mf_max, desc=dsc, obs=rng.integers(0, 4, n).astype(np.int32))
    ex = n_extra
    eX = Ow + (rng.normal(size=(ex, 3)) * np.array([1.5, 1.2, 2.5]) + np.array([0, 0, 1.0])) @ R
    ed = np.linalg.norm(eX - Ow, axis=1)
    emf = (ed * rng.uniform(0.3, 3.0, ex)).astype(np.float32)
    en = rng.normal(size=(ex, 3))
    en /= np.linalg.norm(en, axis=1)[:, None]
    extra = dict(cand=(rng.random(ex) > 0.1).astype(np.uint8), Xw=eX, normal=en, min_dist=np.float32(0.8) * emf / np.float32(3.58),
                 max_dist=np.float32(1.2) * emf, mf_max_dist=emf, desc=rng.integers(0, 256, size=(ex, 32)).astype(np.uint8),
                 obs=rng.integers(0, 3, ex).astype(np.int32))
    out = {k: np.concatenate([pts[k], extra[k]]) for k in pts}
    perm = rng.permutation(n + ex)
    return {k: np.ascontiguousarray(v[perm]) for k, v in out.items()}


def cam9(cam, bf=40.0):
    """(K, bf, bounds) as the nine floats sd_debug_fuse takes."""
    return np.array([*cam.K, bf, *cam.bounds], np.float32)


def cam5(cam, bf=40.0):
    """(K, bf) as the five floats sd_debug_triangulate takes."""
    return np.array([*cam.K, bf], np.float32)


# ---- the wrong cameras a subtly broken kernel would effectively use -------------------------------------------------
def mutations(cam):
    """[(label, camera, raw_keypoints)]: the mutations that change `cam`.  raw_keypoints: the stage is given mvKeys where it
    should read mvKeysUn."""
    (fx, fy, cx, cy), (x0, x1, y0, y1) = cam.K, cam.bounds
    cand = [("fx<->fy", cam._replace(K=(fy, fx, cx, cy)), False),
            ("cx<->cy", cam._replace(K=(fx, fy, cy, cx)), False),
            ("min->0", cam._replace(bounds=(0.0, x1, 0.0, y1)), False),
            ("invW<->invH", cam._replace(bounds=(x0, f32(x0 + (y1 - y0)), y0, f32(y0 + (x1 - x0)))), False)]
    out = [m for m in cand if (m[1].K, m[1].bounds) != (cam.K, cam.bounds)]
    if cam.dist is not None:
        out.append(("raw keypoints", cam, True))
    return out


# ---- the cases of the sweep (SEEDS ... BF are every sweep's: sweep_rig and world_frames take them from here) ------------------
CFG = (1000, 1.2, 8, 20)                           # the P8 pyramid
MP = 1300                                          # the tracker's max_points: 1000 keypoints' points + 300 extra local points
N_EXTRA = 300
SEEDS = (20, 21)
MOTIONS = [((0.02, -0.01, 0.015), (0.4, -0.3, 0.5)), ((-0.03, 0.02, -0.01), (-0.6, 0.2, 0.3))]
START = se3_exp((0.003, -0.002, 0.001), (0.05, 0.02, -0.04))      # e2e_cases.prior: the perturbed start is START @ T_cur
POSE_BOUND = 5e-3                                  # tests/test_pnp_ransac.py's "converges to the truth" bound
BF = 40.0


def undistorted(O, kps, cam):
    """Frame::UndistortKeyPoints by the oracle: mvKeysUn of mvKeys."""
    if cam.dist is None:
        return kps
    out = kps.copy()
    xy = O.undistort_points(np.stack([kps["x"], kps["y"]], 1), cam.K, cam.dist)
    out["x"], out["y"] = xy[:, 0], xy[:, 1]
    return out


def oracle_rig(O, name):
    """The two VGA scenes through camera `name` with the oracle's extraction, undistorted keypoints, pyramids and tables, and the
    last-frame and local-map cases built from the undistorted keypoints (sweep_rig.oracle_rig with this sweep's parameters)."""
    import sweep_rig as SR      # (it imports this module for the builders above)
    return SR.oracle_rig(O, ("cameras", name), CAMERAS[name], W, H, CFG, MP, n_extra=N_EXTRA)


def area_queries(cam):
    """A dozen GetFeaturesInArea discs (x, y, r, min_level, max_level): the four bounds corners, one straddling min_x, one
    straddling min_y, two centred outside the bounds (one reaching in, one not), the centre at two radii and with level ranges."""
    x0, x1, y0, y1 = cam.bounds
    mx, my = 0.5 * (x0 + x1), 0.5 * (y0 + y1)
    q = [(x0, y0, 30.0, -1, -1), (x1, y0, 30.0, -1, -1), (x0, y1, 30.0, -1, -1), (x1, y1, 30.0, -1, -1),
         (x0 + 5.0, my, 20.0, -1, -1), (mx, y0 + 5.0, 20.0, -1, -1), (x1 + 15.0, my + 40.0, 40.0, -1, -1), (x0 - 50.0, y0 - 50.0, 30.0, -1, -1),
         (mx, my, 25.0, -1, -1), (mx, my, 60.0, -1, -1), (mx, my, 60.0, 1, 3), (mx, my, 60.0, 2, -1)]
    return [tuple(f32(v) for v in t[:3]) + t[3:] for t in q]


def epnp_trials(cam):
    """Exact correspondences for compute_pose alone: 4, 5 and 60 points in front of a random pose, projected with cam.K, world
    points and pixels rounded to float before either side sees them."""
    fx, fy, cx, cy = cam.K
    rng = np.random.default_rng(23)
    out = []
    for n in (4, 5, 60):
        T = se3_exp(rng.normal(size=3) * 0.1, rng.normal(size=3) * 5.0)
        Xc = np.stack([rng.uniform(-1.2, 1.2, n), rng.uniform(-0.9, 0.9, n), rng.uniform(1.0, 5.0, n)], 1)
        Xw = ((Xc - T[:3, 3]) @ T[:3, :3]).astype(np.float32).astype(np.float64)
        Xc = Xw @ T[:3, :3].T + T[:3, 3]
        uv = np.stack([fx * Xc[:, 0] / Xc[:, 2] + cx, fy * Xc[:, 1] / Xc[:, 2] + cy], 1).astype(np.float32).astype(np.float64)
        out.append((Xw, uv, T))
    return out


def pose_close(T_est, T_true, what):
    d = np.abs(np.asarray(T_est, np.float64) - T_true).max()
    assert d <= POSE_BOUND, (what, d)
    return d


# ---- the table is what its comments say ---------------------------------------------------------------------------
for _c in CAMERAS.values():
    assert all(v == f32(v) for v in _c.K + _c.bounds + (_c.dist or ())), _c.name
    assert _c.bounds[1] > _c.bounds[0] and _c.bounds[3] > _c.bounds[2], _c.name
assert CAMERAS["synth"].K == (synth.FX, synth.FY, synth.CX, synth.CY) and CAMERAS["synth"].bounds == (0.0, 640.0, 0.0, 480.0)
assert CAMERAS["aniso"].K[0] != CAMERAS["aniso"].K[1] and CAMERAS["offaxis"].K[2] != W / 2 and CAMERAS["offaxis"].K[3] != H / 2
_b = CAMERAS["tum1"].bounds
assert _b[0] > 0 and _b[2] > 0 and np.float32(64) / np.float32(_b[1] - _b[0]) != np.float32(48) / np.float32(_b[3] - _b[2])
_b = CAMERAS["window"].bounds
assert _b[0] > 0 and _b[2] > 0 and np.float32(64) / np.float32(_b[1] - _b[0]) != np.float32(48) / np.float32(_b[3] - _b[2])
_b = CAMERAS["wide"].bounds
assert _b[0] < 0 and _b[2] < 0 and np.float32(64) / np.float32(_b[1] - _b[0]) != np.float32(48) / np.float32(_b[3] - _b[2])
# the inversion of the Brown model behind tum1's rendering: re-distorting the rays reproduces the pixel grid to 1e-6 px
_v, _u = np.mgrid[0:H, 0:W].astype(np.float64)
for _n in ("tum1",):
    _c, _r = CAMERAS[_n], pixel_rays(CAMERAS[_n])
    _xd, _yd = distort_normalised(_r[..., 0], _r[..., 1], _c.dist)
    assert np.abs(_xd * _c.K[0] + _c.K[2] - _u).max() < 1e-6 and np.abs(_yd * _c.K[1] + _c.K[3] - _v).max() < 1e-6, _n
