"""k_fast_cells stages its pixel tile in 16-byte units from a left edge aligned down to 16 bytes, and its queue entries are
byte offsets into that tile (the score map has the tile's pitch).  These cases aim at what that adds: every residue of the
tile's left edge modulo 16, zones narrower than one unit, tile rows that end at the source row's last unit, the level-0
path from caller frames in both its branches (16-byte units / dword by dword), cells of several strips (the offset-bound
row-ownership test with rows above the strip), and queues at their worst-case fill and empty.  Bar: per-cell FAST counts,
selected keys of every level, keypoints and descriptors, all identical to the oracle."""
import numpy as np
import pytest

import sdslam_amd as sd
from sdslam_amd.synth import make_image

EDGE = 19   # border of the padded pyramid levels (the FAST zones start EDGE - 3 pixels inside a level)
TH = 20
# (nfeatures, scaleFactor, nlevels, w, h): small frames whose grids put the zones' left edges on every residue
GEOMETRIES = [
    (800, 1.2, 8, 131, 97),    # odd width: level 0 is read from the padded pyramid like every other level
    (800, 2.0, 5, 132, 100),   # width a multiple of 4 only: level 0 from the frames, dword by dword
    (300, 1.2, 8, 160, 120),   # width a multiple of 16: level 0 from the frames in 16-byte units
    (500, 1.2, 8, 200, 150),
]


def _zones(nf, sf, nl, w, h):
    """(level, tile left edge x in the source row, zone width, source row bytes) of every cell with a FAST zone; host frames
    are uploaded densely (row pitch w), and level 0 is read from them when that pitch is a multiple of 4."""
    info = sd.plan_info(nf, sf, nl, TH, w, h)
    out = []
    for level, zx0, _, zw, zh, _ in info["cells"]:
        if zw <= 0 or zh <= 0:
            continue
        direct = level == 0 and w % 4 == 0
        lw = int(info["levels"][level][0])
        row_bytes = w if direct else (lw + 2 * EDGE + 63) // 64 * 64
        out.append((int(level), int(zx0) - 3 + (0 if direct else EDGE), int(zw), row_bytes, direct))
    return out


def _check(oracle, ext, cfg, imgs, kps, desc, n, what):
    nf, sf, nl = cfg
    for i in range(len(imgs)):
        ora = oracle.OrbOracle(nf, sf, nl, TH)
        ok, od = ora.extract(imgs[i])
        for l in range(nl):
            assert np.array_equal(ext.cell_counts(l, i), ora.cell_totals(l)), f"{what} frame {i}: FAST counts level {l}"
            lk = ora.level_keypoints(l)
            exp = (lk["response"].astype(np.uint32) << 24) | (lk["y"].astype(np.uint32) << 12) | lk["x"].astype(np.uint32)
            assert np.array_equal(ext.level_keys(l, i), exp), f"{what} frame {i}: selected keys level {l}"
        assert n[i] == len(ok), (what, i)
        assert np.array_equal(kps[i, :n[i]], ok) and np.array_equal(desc[i, :n[i]], od), (what, i)


def _frames(w, h, seed, count):
    rng = np.random.default_rng(seed)
    fr = [make_image(seed + k, w, h) for k in range(count - 1)]
    fr.append(rng.integers(0, 256, size=(h, w)).astype(np.uint8))   # noise: corners in every cell, at every column
    return np.stack(fr)


def test_geometries_cover_the_alignment_cases():
    """Host check of the chosen geometries: all 16 residues of the tile's left edge, a zone narrower than 16 pixels, a tile
    row of a single 16-byte unit, both level-0 branches, and the smallest distance a tile row's last unit keeps from the end
    of its source row (pyramid rows are padded by EDGE on both sides and to 64 bytes: never closer than 2 * EDGE - 3 = 35
    bytes; in caller frames the last column of cells ends 16 bytes before the row does, which is the closest there is)."""
    residues, narrow, one_unit, tail, branches = set(), False, False, [], set()
    for nf, sf, nl, w, h in GEOMETRIES:
        for level, xs, zw, row_bytes, direct in _zones(nf, sf, nl, w, h):
            sh = xs % 16
            residues.add(sh)
            narrow |= zw < 16
            one_unit |= sh + zw + 6 <= 16
            end = (xs + zw + 6 + 15) // 16 * 16   # first byte past the tile row's last unit
            assert end <= row_bytes, (w, h, level, xs, zw)
            tail.append(row_bytes - end)
            if direct:
                branches.add(w % 16 == 0)
            else:
                assert row_bytes - end >= 2 * EDGE - 3 - 15
    assert residues == set(range(16)), sorted(residues)
    assert narrow and one_unit
    assert branches == {True, False}
    assert min(tail) <= 16, min(tail)


@pytest.mark.gpu
@pytest.mark.parametrize("geom", GEOMETRIES, ids=lambda g: f"{g[3]}x{g[4]}_{g[2]}x{g[1]}_{g[0]}")
def test_every_alignment_residue(oracle, geom):
    if sd.device_count() < 1:
        pytest.fail("no HIP device: the gpu-marked tests need a real MI355X")
    nf, sf, nl, w, h = geom
    imgs = _frames(w, h, 900 + w, 3)
    ext = sd.ORBextractor(nf, sf, nl, TH, w, h, len(imgs))
    kps, desc, n = ext.extract_batch(imgs)
    _check(oracle, ext, (nf, sf, nl), imgs, kps, desc, n, f"{w}x{h}")
    ext.close()


@pytest.mark.gpu
def test_level0_from_frames_both_branches(oracle):
    """The same frames from a 16-byte aligned buffer with pitches that are multiples of 16 (16-byte units), from a pointer 4
    bytes into a larger allocation, and with a pitch that is a multiple of 4 only (dword loop, twice): identical results,
    equal to the oracle's.  The bytes between the rows are noise: nothing of them may reach a result."""
    if sd.device_count() < 1:
        pytest.fail("no HIP device: the gpu-marked tests need a real MI355X")
    from sdslam_amd.capi import DeviceBuffer
    nf, sf, nl, w, h = 300, 1.2, 8, 160, 120
    imgs = _frames(w, h, 77, 3)
    B = len(imgs)
    rng = np.random.default_rng(5)
    results = []
    for offset, stride in ((0, 160), (0, 176), (4, 160), (0, 164), (4, 172)):
        wide = offset % 16 == 0 and stride % 16 == 0
        host = rng.integers(0, 256, size=offset + B * h * stride + 64).astype(np.uint8)
        view = host[offset:offset + B * h * stride].reshape(B, h, stride)
        view[:, :, :w] = imgs
        d = DeviceBuffer(host.nbytes)
        assert d.ptr.value % 16 == 0
        d.upload(host)
        ext = sd.ORBextractor(nf, sf, nl, TH, w, h, B)
        ext.extract_batch_device(d.ptr.value + offset, B, w, h, stride, stride * h)
        kps, desc, n = ext.download(0, B)
        _check(oracle, ext, (nf, sf, nl), imgs, kps, desc, n, f"offset {offset} pitch {stride} ({'16-byte' if wide else 'dword'})")
        results.append((kps.copy(), desc.copy(), n.copy()))
        ext.close()
        d.free()
    for k, dsc, n in results[1:]:
        assert np.array_equal(n, results[0][2]) and np.array_equal(k, results[0][0]) and np.array_equal(dsc, results[0][1])


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", [(640, 480), (1280, 720)])
def test_strips_and_merged_launch(oracle, w, h):
    """Batch 2 at full size.  640 x 480: whole-cell strips on the large levels and the merged launch of the small ones.
    1280 x 720: a level-0 zone's worst-case queue alone (2 bytes per pixel) is larger than any strip budget, so its cells are
    walked in several strips -- rows above the strip (sr0 > 0) in the tile, ownership decided on tile offsets."""
    if sd.device_count() < 1:
        pytest.fail("no HIP device: the gpu-marked tests need a real MI355X")
    cfg = (1000, 1.2, 8)
    if w == 1280:
        cells = sd.plan_info(*cfg, TH, w, h)["cells"]
        c0 = cells[cells[:, 0] == 0]
        assert (2 * c0[:, 3] * c0[:, 4]).max() > 40 * 1024
    a = make_image(31 + w, w, h)
    imgs = np.stack([a, np.ascontiguousarray(a[::-1, ::-1])])
    ext = sd.ORBextractor(*cfg, TH, w, h, 2)
    kps, desc, n = ext.extract_batch(imgs)
    _check(oracle, ext, cfg, imgs, kps, desc, n, f"{w}x{h}")
    ext.close()


@pytest.mark.gpu
def test_dense_and_empty_queues(oracle):
    """Noise: nearly every pixel passes the compass test, the per-wave queues run close to their capacity of one entry per
    pixel (and the tile offsets stored in them to their largest values).  A constant frame: empty queues, no corner at
    either threshold."""
    if sd.device_count() < 1:
        pytest.fail("no HIP device: the gpu-marked tests need a real MI355X")
    w, h = 160, 120
    cfg = (500, 1.2, 8)
    rng = np.random.default_rng(3)
    salt = np.where(rng.integers(0, 2, size=(h, w)) == 0, 0, 255).astype(np.uint8)
    imgs = np.stack([rng.integers(0, 256, size=(h, w)).astype(np.uint8), salt, np.full((h, w), 93, np.uint8)])
    ext = sd.ORBextractor(*cfg, TH, w, h, len(imgs))
    kps, desc, n = ext.extract_batch(imgs)
    _check(oracle, ext, cfg, imgs, kps, desc, n, "dense / empty")
    assert n[2] == 0
    ext.close()
