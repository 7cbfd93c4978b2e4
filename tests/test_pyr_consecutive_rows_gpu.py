"""k_pyr_rows (runs of consecutive rows that share their source rows) beside k_pyr_split and the generic kernel: every padded
pyramid level read back from the device equals the CPU oracle's byte for byte, through the host-image and the device-pointer
entry; and the host's row-block table is held to the resize's row offsets, recomputed here.

Cases (frame, pyramid, "extract.pyr_rows"):
  vga        640x480 8x1.2   the workload's plan; runs of five rows, now and then four, a last run of one
  euroc      752x480 8x1.2   w + 38 is not a multiple of 4 on several levels: masked last group
  qvga       320x240 8x1.2   every level of this frame is still 67 rows or more, so all seven take k_pyr_rows ...
  small      240x160 8x1.2   ... this is the nearest frame whose top levels leave it: levels 6-7 leave k_pyr_rows (too few rows for
                             single-reflection borders, or its runs too short), beside k_pyr_rows on levels 1-5
  x2         640x480 5x2.0   no shared source rows: exact-2x levels, the plan keeps k_pyr_rows out
  x1_5       640x480 4x1.5   runs of two rows: the plan keeps k_pyr_rows out (k_pyr_split resizes the levels) ...
  x1_5_rows  640x480 4x1.5   ... and with the option at 2 the same levels go through k_pyr_rows: runs of two and one
  x1_33_rows 640x480 4x1.3333  option at 2: runs of three (no 8x1.2 geometry has a run of two or three)
"""
import numpy as np
import pytest

from sdslam_amd.synth import make_image

pytestmark = pytest.mark.gpu

NF, TH = 1000, 20
CASES = {
    "vga": (640, 480, 8, 1.2, 1),
    "euroc": (752, 480, 8, 1.2, 1),
    "qvga": (320, 240, 8, 1.2, 1),
    "small": (240, 160, 8, 1.2, 1),
    "x2": (640, 480, 5, 2.0, 1),
    "x1_5": (640, 480, 4, 1.5, 1),
    "x1_5_rows": (640, 480, 4, 1.5, 2),
    "x1_33_rows": (640, 480, 4, 1.3333, 2),
}
# levels 1... of each case that the plan gives to k_pyr_rows
ROWS_LEVELS = {"vga": 7, "euroc": 7, "qvga": 7, "small": 5, "x2": 0, "x1_5": 0, "x1_5_rows": 3, "x1_33_rows": 3}
R = 5   # rows of a block


@pytest.fixture(scope="module")
def sd():
    import sdslam_amd
    if sdslam_amd.device_count() < 1:
        pytest.fail("no HIP device: the gpu-marked tests need a real MI355X")
    return sdslam_amd


def _row_offsets(sn, dn):
    """First source row of every output row: cv::resize INTER_LINEAR (float position, floor)."""
    scale = 1.0 / (float(dn) / sn)
    f = ((np.arange(dn, dtype=np.float64) + 0.5) * scale - 0.5).astype(np.float32)
    return np.floor(f).astype(np.int64)


def _expected_blocks(sn, dn):
    yo, out, y0 = _row_offsets(sn, dn), [], 0
    while y0 < dn:
        n = 1
        while n < R and y0 + n < dn and yo[y0 + n] == yo[y0 + n - 1] + 1:
            n += 1
        rows = range(y0, y0 + n)
        border = any(1 <= y <= 19 or dn - 20 <= y <= dn - 2 for y in rows)
        out.append((y0, n, int(yo[y0]), int(border)))
        y0 += n
    return np.array(out, np.int32)


def _blocks(sd, name):
    W, H, nl, sf, mode = CASES[name]
    with sd.options({"extract.pyr_rows": mode}):
        heights = sd.plan_info(NF, sf, nl, TH, W, H)["levels"][:, 1]
        return heights, [sd.plan_row_blocks(NF, sf, nl, TH, W, H, l) for l in range(nl)]


@pytest.mark.parametrize("name", list(CASES))
def test_levels_equal_the_oracle(sd, oracle, name):
    W, H, nl, sf, mode = CASES[name]
    frames = np.stack([np.ascontiguousarray(make_image(310 + i, max(W, 640), max(H, 480))[:H, :W]) for i in range(2)])
    ora = oracle.OrbOracle(NF, sf, nl, TH)
    want = []
    for i in range(2):
        ora.extract(frames[i])
        want.append([ora.level(l, padded=True) for l in range(nl)])
    with sd.options({"extract.pyr_rows": mode}):
        _, blocks = _blocks(sd, name)
        assert sum(len(b) > 0 for b in blocks) == ROWS_LEVELS[name], [len(b) for b in blocks]
        ext = sd.ORBextractor(NF, sf, nl, TH, W, H, 2)
        ext.extract_batch(frames)
        for i in range(2):
            for l in range(nl):
                assert np.array_equal(ext.level(l, i, padded=True), want[i][l]), f"host entry: level {l} of frame {i}"
        ext.close()
        ext = sd.ORBextractor(NF, sf, nl, TH, W, H, 2)
        buf = sd.DeviceBuffer(frames.nbytes)
        buf.upload(frames[::-1])     # the other order: the levels of a slot change between the two entries
        ext.extract_batch_device(buf.ptr, 2, W, H)
        ext.download(0, 2)
        for i in range(2):
            for l in range(nl):
                assert np.array_equal(ext.level(l, i, padded=True), want[1 - i][l]), f"device entry: level {l} of frame {i}"
        ext.close()
        buf.free()


def test_row_block_table(sd):
    """The table is the resize's row offsets cut into runs, every run length the table has room for (1 ... 5) is walked by some
    case above, and the first and last blocks of a level carry its border rows."""
    seen = set()
    for name in CASES:
        heights, blocks = _blocks(sd, name)
        assert len(blocks[0]) == 0, "level 0 is a copy"
        for l in range(1, len(blocks)):
            b = blocks[l]
            if len(b) == 0:
                continue
            want = _expected_blocks(int(heights[l - 1]), int(heights[l]))
            assert np.array_equal(b, want), (name, l)
            assert b[:, 1].sum() == heights[l] and np.array_equal(b[1:, 0], np.cumsum(b[:-1, 1]))   # every row once, in order
            assert b[0, 3] == 1 and b[-1, 3] == 1, (name, l, "first / last block without border rows")
            flagged = {int(y) for k in b if k[3] for y in range(k[0], k[0] + k[1])}
            assert set(range(1, 20)) | set(range(int(heights[l]) - 20, int(heights[l]) - 1)) <= flagged, (name, l)
            assert not b[len(b) // 2, 3], (name, l, "a block in the middle of the level is flagged")
            seen |= {int(n) for n in b[:, 1]}
    assert seen == set(range(1, R + 1)), seen


def test_option_off_is_k_pyr_split(sd):
    with sd.options({"extract.pyr_rows": 0}):
        assert all(len(sd.plan_row_blocks(NF, 1.2, 8, TH, 640, 480, l)) == 0 for l in range(8))
