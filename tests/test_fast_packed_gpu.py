"""k_fast_cells scores its queued pixels two per lane (phase B: entry e0 + lane in the low 16-bit halves, e0 + 64 + lane in
the high halves, packed f16 min3 / max3).  These frames aim at what that pairing adds: 0 / 255 extremes, scores at th - 1,
th and th + 1, a flat frame, checkerboards, and per-wave queues of 1, 63, 64, 65, 127, 128 and 129 entries (odd tails,
high halves with no entry, chunks that end exactly at 64 / 128), at thresholds 0, 1, 20 and 254.  Bar: per-cell FAST
counts and selected keys of every level, keypoints and descriptors, all identical to the oracle."""
import numpy as np
import pytest

import sdslam_amd as sd
from sdslam_amd.synth import make_image

W, H = 640, 480
CFG = (1000, 1.2, 8)
QUEUE_SIZES = (1, 63, 64, 65, 127, 128, 129)
BAND_ROWS = (0, 1, 5, 6, 10, 11)   # dot rows inside a wave's band (the band of a level-0 zone is 19 rows at VGA)


def _dot_sites(x0, x1, y0):
    """Dot positions of one wave band in raster order: rows y0 + BAND_ROWS, columns x = 0, 1, 2 (mod 6).  No two dots are a
    FAST ring offset or (+-3, +-3) apart, so on a flat background exactly the dots pass the compass test."""
    return [(y0 + r, x) for r in BAND_ROWS for x in range(x0, x1) if x % 6 < 3]


def _level0_bands():
    """(zone, four wave bands) of every level-0 cell: one strip per cell at VGA, so wave w owns zone rows [w * rpw, (w + 1) * rpw)."""
    cells = sd.plan_info(*CFG, 20, W, H)["cells"]
    out = []
    for _, zx0, zy0, zw, zh, _ in cells[cells[:, 0] == 0]:
        rpw = (zh + 3) >> 2
        out.append(((zx0, zy0, zw, zh), [(zy0 + w * rpw, min(zy0 + (w + 1) * rpw, zy0 + zh)) for w in range(4)]))
    return out


def queue_frame(bg, dot):
    """Level-0 cell c, wave w gets QUEUE_SIZES[(c + w) % 7] isolated dots: every size in every wave."""
    img = np.full((H, W), bg, np.uint8)
    expect = []
    for c, ((zx0, zy0, zw, zh), bands) in enumerate(_level0_bands()):
        for w, (b0, b1) in enumerate(bands):
            n = QUEUE_SIZES[(c + w) % len(QUEUE_SIZES)]
            sites = _dot_sites(zx0, zx0 + zw, b0)[:n]
            assert len(sites) == n and all(y < b1 for y, _ in sites), "band too small for the dot lattice"
            for y, x in sites:
                img[y, x] = dot
            expect.append((zx0, zy0, zw, zh, b0, b1, n))
    return img, expect


def compass_pass(img, th):
    """Phase A's compass test of k_fast_cells, on the host: max(v - D, Bt - v) > th."""
    p = img.astype(np.int32)
    v = p[3:-3, 3:-3]
    p0, p8, p4, p12 = p[6:, 3:-3], p[:-6, 3:-3], p[3:-3, 6:], p[3:-3, :-6]
    D = np.maximum(np.minimum(p0, p8), np.minimum(p4, p12))
    Bt = np.minimum(np.maximum(p0, p8), np.maximum(p4, p12))
    out = np.zeros(img.shape, bool)
    out[3:-3, 3:-3] = np.maximum(v - D, Bt - v) > th
    return out


def tuned_frame(th, seed):
    """Patches whose centre scores th - 1, th or th + 1 (clipped to 0..255) while passing the compass test: the ring is far
    brighter (darker) than the centre except ring points 2 and 10, which every nine-arc contains one of, at +-s."""
    ring = [(0, 3), (1, 3), (2, 2), (3, 1), (3, 0), (3, -1), (2, -2), (1, -3), (0, -3), (-1, -3), (-2, -2), (-3, -1), (-3, 0),
            (-3, 1), (-2, 2), (-1, 3)]
    rng = np.random.default_rng(seed)
    img = np.full((H, W), 128, np.uint8)
    k = 0
    for cy in range(24, H - 24, 11):
        for cx in range(24, W - 24, 11):
            s = th + (k % 3)   # score s - 1: th - 1, th, th + 1
            bright = (k // 3) % 2 == 0
            k += 1
            v = int(rng.integers(0, 40)) if bright else int(rng.integers(215, 256))
            far = 255 if bright else 0
            near = min(v + s, 255) if bright else max(v - s, 0)
            img[cy - 3:cy + 4, cx - 3:cx + 4] = v
            for i, (dx, dy) in enumerate(ring):
                img[cy + dy, cx + dx] = near if i in (2, 10) else far
    return img


def checkerboard(sq, lo=0, hi=255):
    yy, xx = np.mgrid[0:H, 0:W]
    return np.where(((yy // sq) + (xx // sq)) % 2 == 0, lo, hi).astype(np.uint8)


def frames(th):
    rng = np.random.default_rng(11 + th)
    qb, _ = queue_frame(0, 255)
    qd, _ = queue_frame(255, 0)
    sparse = np.full((H, W), 0, np.uint8)   # isolated bright and dark dots at +-255
    ys, xs = rng.integers(8, H - 8, 600), rng.integers(8, W - 8, 600)
    sparse[ys[:300], xs[:300]] = 255
    dark = np.full((H, W), 255, np.uint8)
    dark[ys[300:], xs[300:]] = 0
    return {
        "queue_bright": qb, "queue_dark": qd, "dots_bright": sparse, "dots_dark": dark,
        "tuned": tuned_frame(th, th), "flat": np.full((H, W), 77, np.uint8),
        "checker1": checkerboard(1), "checker3": checkerboard(3), "checker4_mid": checkerboard(4, 100, 140),
        "textured": make_image(300 + th), "noise": rng.integers(0, 256, size=(H, W)).astype(np.uint8),
    }


def test_queue_frames_hit_the_sizes():
    """The queue frames really give every wave of a level-0 cell the intended number of phase-A survivors (host check of
    the frame construction, at every threshold of the GPU test: dots are 255 on 0 or 0 on 255)."""
    for bg, dot in ((0, 255), (255, 0)):
        img, expect = queue_frame(bg, dot)
        for th in (0, 1, 20, 254):
            passed = compass_pass(img, th)
            seen = set()
            for zx0, zy0, zw, zh, b0, b1, n in expect:
                assert int(passed[b0:b1, zx0:zx0 + zw].sum()) == n
                seen.add(n)
            assert seen == set(QUEUE_SIZES)


@pytest.mark.gpu
@pytest.mark.parametrize("th", [0, 1, 20, 254])
def test_fast_paired_scoring_matches_oracle(oracle, th):
    if sd.device_count() < 1:
        pytest.fail("no HIP device: the gpu-marked tests need a real MI355X")
    fr = frames(th)
    names = list(fr)
    imgs = np.stack([fr[n] for n in names])
    ext = sd.ORBextractor(*CFG, th, W, H, len(names))
    kps, desc, n = ext.extract_batch(imgs)
    for i, name in enumerate(names):
        ora = oracle.OrbOracle(*CFG, th)
        ok, od = ora.extract(imgs[i])
        for l in range(CFG[2]):
            assert np.array_equal(ext.cell_counts(l, i), ora.cell_totals(l)), f"{name} th {th}: FAST counts level {l}"
            lk = ora.level_keypoints(l)
            exp = (lk["response"].astype(np.uint32) << 24) | (lk["y"].astype(np.uint32) << 12) | lk["x"].astype(np.uint32)
            assert np.array_equal(ext.level_keys(l, i), exp), f"{name} th {th}: selected keys level {l}"
        assert n[i] == len(ok), (name, th)
        assert np.array_equal(kps[i, :n[i]], ok) and np.array_equal(desc[i, :n[i]], od), (name, th)
    ext.close()
