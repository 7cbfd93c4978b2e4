"""Frame geometries other than VGA, shared by the geometry-sweep tests (helper, no tests).

Every tracking parity test runs at 640 x 480 (one at 1280 x 720): landscape, both sides multiples of 16, the 8 x 1.2 pyramid,
cols > rows on every level, even row pitches w + 38, bounds (0, W, 0, H) with invW = 0.1, and no keypoint-derived point within
3 px of the right or bottom border of an aligned level.  At such a frame k_align's `cols` and `rows`, a wrong pitch, a level
size taken by another rounding than cvRound, k_stereo_from_depth's `w` and `h` and a frame-grid cell that is taller than wide
cannot be told apart from the right thing.  The table below holds frames that separate them.

                W x H     extractor           K                          there for
    vga       640 x 480   (300, 1.2, 8, 20)   500 500 320 240            control: today's results
    odd       637 x 479   (300, 1.2, 8, 20)   500 500 318.5 239.5        odd pitch w + 38, byte-unaligned rows, level sizes that need cvRound
                                                                         (level 3 is 369 wide, 368 by truncation; level 4 is 231 high, 230 by truncation)
    wide      752 x 480   (300, 1.2, 8, 20)   458.7 457.3 367.2 248.4    x > 640, cells 11.75 px wide, invW != 0.1
    portrait  480 x 640   (300, 1.2, 8, 20)   500 500 240 320            rows > cols on every level, y > 480, cells taller than wide
    small15   321 x 243   (300, 1.5, 5, 20)   250 250 160.5 121.5        level 4 is 63 x 48, the smallest aligned level; the sf / inv_sf tables
                                                                         of a 1.5 pyramid in modes 0 / 1 against mode 3
No row had to be moved: the extraction plan accepts all five (tests/test_geometries_cpu.py asserts it).

Every K value is float(np.float32(v)), as sd_track_set_camera takes it; the bounds are (0, W, 0, H).  Scenes come from
cameras.make_scene(seed, cam, ..., w=W, h=H) with the two MOTIONS of cameras.py, so B = 2.

Planted border points.  ImageAlign takes the FIRST 300 valid points of the last frame (src/ImageAlign.cc:62-72), so the
last frame holds the points of the first 300 - 12 reference keypoints and, appended after the keypoints' rows, 12 planted
points: for every aligned level l in {2, 3, 4} four surface points whose reference projection (u, v) has
floor(u s) + 3 == cols_l - 1 (just visible) and == cols_l (just clipped) at mid-height, and floor(v s) + 3 == rows_l - 1 and
== rows_l at mid-width, s = inv_sf[l] as k_align uses it in mode 0, cols_l x rows_l the oracle's level(l) shape.  They carry
zero descriptors, octave 0, angle 0 and one observation.  max_points = 300 + 12.

Modes 2 and 3 take only the first 100 valid points, so that last frame never shows them a planted point.  Mode 3 (keyframe
against keyframe, level 4 alone, scale (float)(1.0 / sf[4])) therefore runs on a last frame of its own, `last3`: the points
of the first 100 - 4 reference keypoints and the four level-4 pairs built for that scale, 100 valid points in all."""
from collections import namedtuple

import numpy as np

import cameras as CM
import sweep_rig as SR
from sdslam_amd.synth import intersect_surface

Geometry = namedtuple("Geometry", "name w h cfg cam")
N_PLANTED = 12
N_ALIGNED = 300                      # AL_MAXP: the points ImageAlign takes in modes 0 and 1
N_ALIGNED_KF = 100                   # the points it takes in modes 2 and 3
MP = 300 + N_PLANTED                 # the tracker's max_points
ALIGNED_LEVELS = (2, 3, 4)
BF = CM.BF
DEPTH_FACTOR = 5000.0
POISON_U16, POISON_F32 = np.uint16(65535), np.float32(1e9)


def _geo(name, w, h, cfg, K):
    return Geometry(name, w, h, cfg, CM.Camera(name, tuple(CM.f32(v) for v in K), None, (0.0, float(w), 0.0, float(h))))


GEOMETRIES = {g.name: g for g in (
    _geo("vga", 640, 480, (300, 1.2, 8, 20), (500.0, 500.0, 320.0, 240.0)),
    _geo("odd", 637, 479, (300, 1.2, 8, 20), (500.0, 500.0, 318.5, 239.5)),
    _geo("wide", 752, 480, (300, 1.2, 8, 20), (458.7, 457.3, 367.2, 248.4)),
    _geo("portrait", 480, 640, (300, 1.2, 8, 20), (500.0, 500.0, 240.0, 320.0)),
    _geo("small15", 321, 243, (300, 1.5, 5, 20), (250.0, 250.0, 160.5, 121.5)),
)}
NAMES = list(GEOMETRIES)
LOOPED = ["wide", "portrait"]        # the geometries that also run relocalisation, DetectLoop and the sequential loop


# ---- k_align's clip test, restated (track_align.hip: project -> (float)(u2 * scale) -> floor -> four comparisons) ------------
def project_level(Xw, T_ref, K, scale):
    """(uf, vf, behind) of world points in a reference level: xc = (r0 p0 + r1 p1 + r2 p2) + t in double, u2 = fx xc0 / zc + cx,
    u_ref = (float)(u2 * scale) with the float scale widened to double, uf = floor(u_ref).  behind: 1 / zc < 0."""
    fx, fy, cx, cy = K
    Xw, T = np.asarray(Xw, np.float64), np.asarray(T_ref, np.float64)
    xc = [(T[i, 0] * Xw[:, 0] + T[i, 1] * Xw[:, 1] + T[i, 2] * Xw[:, 2]) + T[i, 3] for i in range(3)]
    invz = 1.0 / xc[2]
    s = np.float64(np.float32(scale))
    u_ref = ((fx * xc[0] * invz + cx) * s).astype(np.float32)
    v_ref = ((fy * xc[1] * invz + cy) * s).astype(np.float32)
    return np.floor(u_ref).astype(np.int64), np.floor(v_ref).astype(np.int64), invz < 0


def clip_visible(Xw, T_ref, K, scale, cols, rows):
    """The points k_align keeps on a level: !(uf - 3 < 0 || vf - 3 < 0 || uf + 3 >= cols || vf + 3 >= rows), in front."""
    uf, vf, behind = project_level(Xw, T_ref, K, scale)
    return ~behind & ~((uf - 3 < 0) | (vf - 3 < 0) | (uf + 3 >= cols) | (vf + 3 >= rows))


def kf_scale(sf, level=4):
    """The level scale of mode 3: (float)(1.0 / sf[level]), the division in double."""
    return np.float32(1.0 / np.float64(np.float32(sf[level])))


def planted_points(geo, scales, shapes, levels=ALIGNED_LEVELS):
    """Four planted points per level of `levels` and what each claims: (Xw [4 n, 3], [(level, axis, visible)]), axis 0 = right
    border, 1 = bottom; scales[l] is the level scale the aligner multiplies with."""
    uv, claims = [], []
    for l in levels:
        rows, cols = shapes[l]
        s = float(np.float32(scales[l]))
        for axis, n, mid in ((0, cols, 0.5 * geo.h), (1, rows, 0.5 * geo.w)):
            for visible in (True, False):
                c = ((n - 4 if visible else n - 3) + 0.5) / s          # floor(c s) + 3 == n - 1 / == n, half a level pixel from flipping
                uv.append((c, mid) if axis == 0 else (mid, c))
                claims.append((l, axis, visible))
    return CM.backproject_on_surface(np.array(uv), geo.cam), claims


def with_planted(last, Xp):
    """`last` (its first 300 - 12 rows valid) with the planted points appended: zero descriptors, octave 0, valid, one observation."""
    k = len(Xp)
    add = dict(valid=np.ones(k, np.uint8), Xw=Xp, desc=np.zeros((k, 32), np.uint8), octave=np.zeros(k, np.int32), angle=np.zeros(k, np.float32),
               obs=np.ones(k, np.int32))
    return {key: np.ascontiguousarray(np.concatenate([last[key], add[key]])) for key in last}


# ---- depth maps: strided, poisoned ------------------------------------------------------------------------------------------
def surface_depth(T_cw, geo):
    """The camera-frame depth of the scene surface along every pixel's ray, as an RGB-D sensor at T_cw reports it (float32)."""
    R, t = T_cw[:3, :3], T_cw[:3, 3]
    Xs = intersect_surface(-R.T @ t, CM.pixel_rays(geo.cam, geo.w, geo.h) @ R, 2.0)
    return (Xs @ R.T + t)[..., 2].astype(np.float32)


def strided(maps, poison):
    """[B, H, W] maps laid out with a row stride of W + 5 elements and a frame stride of (H + 3) * stride, the slack filled with
    `poison`: (flat buffer, stride, frame_stride)."""
    B, h, w = maps.shape
    stride = w + 5
    fstride = (h + 3) * stride
    flat = np.full(B * fstride, poison, maps.dtype)
    for f in range(B):
        flat[f * fstride:f * fstride + h * stride].reshape(h, stride)[:, :w] = maps[f]
    return flat, stride, fstride


def depth_scale(factor):
    return np.float32(1) if factor == 0 else np.float32(1) / np.float32(factor)


def stereo_from_depth(kps, kps_un, flat, f, w, h, stride, fstride, convert, scale, bf, swap_uv=False):
    """k_stereo_from_depth for frame f, line by line: v = (int)kp.y, u = (int)kp.x of the RAW keypoint; inside u < w && v < h the
    element at f * frame_stride + v * stride + u, as float, times `scale` if converted; d > 0 gives depth = d and
    uright = kps_un.x - bf / d in float.  swap_uv reads [u, v] (the mutation of tests/test_geometries_cpu.py; an index past the
    buffer reads as 0)."""
    n = len(kps)
    ur, dd = np.full(n, -1, np.float32), np.full(n, -1, np.float32)
    u, v = kps["x"].astype(np.int64), kps["y"].astype(np.int64)
    inside = (u >= 0) & (v >= 0) & (u < w) & (v < h)
    idx = f * fstride + ((u * stride + v) if swap_uv else (v * stride + u))
    ok = inside & (idx < len(flat))
    raw = np.zeros(n, np.float32)
    raw[ok] = flat[idx[ok]].astype(np.float32)
    d = raw * np.float32(scale) if convert else raw
    pos = inside & (d > 0)
    dd[pos] = d[pos]
    ur[pos] = kps_un["x"][pos].astype(np.float32) - np.float32(bf) / d[pos]
    return ur, dd


# (dtype code, depth_map_factor, converted): f32 as it is, f32 scaled, u16 at the TUM factor, u16 at factor 1 (always converted)
DEPTH_CALLS = [("f32", 0, 1.0, False), ("f32", 0, 2.0, True), ("u16", 1, DEPTH_FACTOR, True), ("u16", 1, 1.0, True)]


# ---- the cases of the sweep ------------------------------------------------------------------------------------------------
def _plant_and_add_depth(O, rig):
    """On top of sweep_rig.oracle_rig: the level shapes, the planted points behind the last frame's 300 - 12 keypoint points,
    mode 3's own last frame, the padded aligned levels and the depth maps of the current views."""
    geo, cam = GEOMETRIES[rig["cam"].name], rig["cam"]
    for i, f in enumerate(rig["fr"]):
        shapes = [a.shape for a in f["pr"]]
        Xp, claims = planted_points(geo, f["tab"]["inv_sf"], shapes)
        Xp3, claims3 = planted_points(geo, {4: kf_scale(f["tab"]["sf"])}, shapes, levels=(4,))
        last3 = with_planted(CM.tracking_case(i, f["rk"], f["rd"], cam, max_points=N_ALIGNED_KF - len(Xp3)), Xp3)
        f.update(last=with_planted(f["last"], Xp), shapes=shapes, Xp=Xp, claims=claims, last3=last3, Xp3=Xp3, claims3=claims3,
                 pc_pad=[f["oc"].level(l, padded=True) for l in ALIGNED_LEVELS], pr_pad=[f["orf"].level(l, padded=True) for l in ALIGNED_LEVELS])
    depth = np.stack([surface_depth(s["T_cur"], geo) for s in rig["scenes"]])
    depth[:, :, ::7] = 0.0                                              # holes: keypoints without depth
    raw = np.round(depth.astype(np.float64) * DEPTH_FACTOR).astype(np.uint16)
    rig.update(geo=geo, depth_f32=depth, depth_u16=raw, buf_f32=strided(depth, POISON_F32), buf_u16=strided(raw, POISON_U16))


def oracle_rig(O, name):
    """The two scenes of geometry `name` with the oracle's extraction, pyramids and tables, the last frame with its planted
    points, the local map (filling max_points) and the depth maps of the current views."""
    geo = GEOMETRIES[name]
    return SR.oracle_rig(O, ("geometries", name), geo.cam, geo.w, geo.h, geo.cfg, MP, n_last=N_ALIGNED - N_PLANTED, extend=_plant_and_add_depth)


def align_points(last):
    return last["Xw"][last["valid"] != 0]


def area_queries(geo):
    """GetFeaturesInArea discs (x, y, r, min_level, max_level): the four bounds corners, straddling the right and the bottom
    bound and around the last pixel (W - 1, H - 1), with radii of a quarter to a third of the short side because the keypoints
    are sparse near the border; centred discs whose r exceeds a grid cell in one direction only (cells are W / 64 wide and
    H / 48 high); and a large centred disc with and without a level range."""
    w, h = float(geo.w), float(geo.h)
    cw, ch = w / 64.0, h / 48.0
    r_one = 0.5 * (cw + ch)                                             # between the two cell sides (equal at vga only: 10 x 10)
    m = min(w, h)
    q = [(0.0, 0.0, 0.3 * m, -1, -1), (w, 0.0, 0.3 * m, -1, -1), (0.0, h, 0.3 * m, -1, -1), (w, h, 0.3 * m, -1, -1),
         (w - 5.0, 0.5 * h, 0.25 * m, -1, -1), (0.5 * w, h - 5.0, 0.25 * m, -1, -1), (w - 1.0, h - 1.0, 0.35 * m, -1, -1),
         (0.5 * w, 0.5 * h, r_one, -1, -1), (0.31 * w, 0.64 * h, r_one, -1, -1), (0.5 * w, 0.5 * h, 0.2 * w, -1, -1), (0.5 * w, 0.5 * h, 0.2 * w, 1, 3)]
    return [tuple(CM.f32(v) for v in t[:3]) + t[3:] for t in q]


def grid_occupancy(kps_un, bounds):
    """Frame::AssignFeaturesToGrid's counts [64][48]: PosInGrid rounds (x - min_x) * invW and (y - min_y) * invH in float and
    drops a keypoint whose cell is outside the grid (src/Frame.cc:323-335)."""
    x0, x1, y0, y1 = (np.float32(b) for b in bounds)
    iw, ih = np.float32(64) / (x1 - x0), np.float32(48) / (y1 - y0)
    def c_round(p):                                                     # round(): halves away from zero (numpy's go to even)
        p = p.astype(np.float64)
        return np.where(p >= 0, np.floor(p + 0.5), np.ceil(p - 0.5)).astype(np.int64)
    px = c_round((kps_un["x"].astype(np.float32) - x0) * iw)
    py = c_round((kps_un["y"].astype(np.float32) - y0) * ih)
    ok = (px >= 0) & (px < 64) & (py >= 0) & (py < 48)
    g = np.zeros((64, 48), np.int32)
    np.add.at(g, (px[ok], py[ok]), 1)
    return g


def swapped_levels(levels, padded_levels, shapes):
    """The aligned levels as arrays whose shape is (cols, rows) instead of (rows, cols) over the SAME pixels and pitch: what an
    aligner that exchanged cols and rows in its clip test would work with.  (Each padded level sits in the corner of a canvas
    large enough for the exchanged shape; the other levels stay as they are.)"""
    out = list(levels)
    for k, l in enumerate(ALIGNED_LEVELS):
        rows, cols = shapes[l]
        side = max(rows, cols) + 38
        canvas = np.zeros((side, side), np.uint8)
        canvas[:rows + 38, :cols + 38] = padded_levels[k]
        out[l] = canvas[19:19 + cols, 19:19 + rows]
    return out


# ---- the table is what its comments say ----------------------------------------------------------------------------------
for _g in GEOMETRIES.values():
    assert all(v == CM.f32(v) for v in _g.cam.K + _g.cam.bounds) and _g.cam.bounds == (0.0, float(_g.w), 0.0, float(_g.h)), _g.name
assert GEOMETRIES["odd"].w % 2 == 1 and (GEOMETRIES["odd"].w + 38) % 2 == 1 and GEOMETRIES["portrait"].h > GEOMETRIES["portrait"].w
assert GEOMETRIES["wide"].w > 640 and np.float32(64) / np.float32(GEOMETRIES["wide"].w) != np.float32(0.1)
