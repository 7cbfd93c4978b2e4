"""GPU: the host layer of the extractor (orb_host.hip) where no other test looks -- the stage timers on every path of the launch
pipeline, the two downloads on their bulk and row paths, and the host-input and device-input entry points against each other.
Small frames throughout; results are compared bit for bit between runs of the same library (test_orb_gpu / test_golden pin
them to the oracle)."""
import ctypes as C
import time

import numpy as np
import pytest

from sdslam_amd.capi import KP_DTYPE, _p
from sdslam_amd.synth import make_image

pytestmark = pytest.mark.gpu
W, H = 160, 120
SD_ERR_INVALID_ARG, SD_ERR_CAPACITY = 1, 3


@pytest.fixture(scope="module")
def sd():
    import sdslam_amd
    if sdslam_amd.device_count() < 1:
        pytest.fail("no HIP device: the gpu-marked tests need a real MI355X")
    return sdslam_amd


def _frames(seed0, n, w=W, h=H):
    return np.stack([make_image(seed0 + i, w, h) for i in range(n)])


def _device_copy(sd, frames, offset=0):
    """The frames in device memory, `offset` bytes into an allocation with room to spare behind them."""
    buf = sd.DeviceBuffer(frames.nbytes + 256)
    frames = np.ascontiguousarray(frames)
    assert sd.lib().sd_dev_upload(C.c_void_p(buf.ptr.value + offset), _p(frames), frames.nbytes) == 0
    return buf, buf.ptr.value + offset


def _same(a, b, what):
    (ka, da, na), (kb, db, nb) = a, b
    assert np.array_equal(na, nb), (what, na, nb)
    for f in range(len(na)):
        assert np.array_equal(ka[f, :na[f]], kb[f, :na[f]]), f"{what}: keypoints of frame {f}"
        assert np.array_equal(da[f, :na[f]], db[f, :na[f]]), f"{what}: descriptors of frame {f}"


# name: (nfeatures, scaleFactor, nlevels), options, byte offset of the device frames, tracker attached
STAGE_CASES = {
    "default": ((300, 1.2, 8), {}, 0, False),
    "fast0_from_pyramid": ((300, 1.2, 8), {"extract.fast0_from_frames": 0}, 0, False),
    "misaligned_frames": ((300, 1.2, 8), {}, 1, False),      # generic pyramid kernel for level 0, no direct FAST
    "pyramid_5x2": ((300, 2.0, 5), {}, 0, False),
    "no_grid_cell": ((6, 1.2, 8), {}, 0, False),             # no FAST launch at all
    "pyr_early": ((300, 1.2, 8), {"extract.pyr_early": 1}, 0, True),
}


@pytest.mark.parametrize("case", list(STAGE_CASES), ids=list(STAGE_CASES))
def test_stage_timers_on_every_pipeline_path(sd, case):
    """sd_orb_stage_ms after three profiled device-input extractions (the first behind nothing, the next two on the early
    level-0 FAST path): SD_OK and five finite times in [0, wall time of the calls]; a begin / end pair naming an event that
    the path did not record fails in hipEventElapsedTime.  Profiling changes no result, and after off / on there is nothing
    to read until the next call."""
    (nfeatures, sf, nlevels), opts, offset, with_tracker = STAGE_CASES[case]
    if case == "no_grid_cell":
        assert len(sd.plan_info(nfeatures, sf, nlevels, 20, W, H)["cells"]) == 0
    frames = _frames(40, 2)
    buf, d_ptr = _device_copy(sd, frames, offset)
    ext = ref = trk = None
    with sd.options(opts):      # (restores the options on the way out, also on failure)
        try:
            ext = sd.ORBextractor(nfeatures, sf, nlevels, 20, W, H, 2)
            if with_tracker:    # a second output set, which extract.pyr_early needs
                ref = sd.ORBextractor(nfeatures, sf, nlevels, 20, W, H, 2)
                trk = sd.Tracker(ext, ref, 300, 2, 8)
            ext.set_profiling(True)
            t0 = time.perf_counter()
            for _ in range(3):
                ext.extract_batch_device(d_ptr, 2, W, H)
            ext.sync()
            wall_ms = (time.perf_counter() - t0) * 1e3
            ms = ext.stage_ms()
            print(case, dict(zip(ext.stage_names(), ms.tolist())), "wall", wall_ms)
            assert len(ms) == 5 and np.isfinite(ms).all() and (ms >= 0).all() and (ms <= wall_ms).all(), (ms, wall_ms)
            profiled = ext.download(0, 2)
            ext.set_profiling(False)
            ext.extract_batch_device(d_ptr, 2, W, H)
            plain = ext.download(0, 2)
            _same(profiled, plain, case)
            assert (plain[2] > 0).all() or case == "no_grid_cell"
            ext.set_profiling(True)
            with pytest.raises(sd.SdError) as e:
                ext.stage_ms()
            assert e.value.code == SD_ERR_INVALID_ARG
            ext.extract_batch_device(d_ptr, 2, W, H)
            ms = ext.stage_ms()
            assert np.isfinite(ms).all() and (ms >= 0).all()
            _same(ext.download(0, 2), plain, case + ", profiling on again")
        finally:
            for x in (trk, ext, ref):
                if x is not None:
                    x.close()
            buf.free()


def _download_c(ext, frame0, n_frames, cap_per_frame, counts_only=False):
    """sd_orb_download with a row capacity of the caller's choice (ORBextractor.download always passes nfeatures)."""
    k = np.zeros((n_frames, max(cap_per_frame, 1)), KP_DTYPE)
    d = np.zeros((n_frames, max(cap_per_frame, 1), 32), np.uint8)
    n = np.full(n_frames, -1, np.int32)
    rc = ext.L.sd_orb_download(ext.h, frame0, n_frames, None if counts_only else _p(k), None if counts_only else _p(d),
                               cap_per_frame, _p(n))
    return rc, (k, d, n)


def _download_un_c(ext, frame0, n_frames, cap_per_frame):
    k = np.zeros((n_frames, max(cap_per_frame, 1)), KP_DTYPE)
    return ext.L.sd_orb_download_undistorted(ext.h, C.c_int(frame0), C.c_int(n_frames), _p(k), C.c_int(cap_per_frame)), k


def test_downloads_bulk_rows_capacity_and_range(sd):
    NF = 12
    frames = _frames(60, NF)
    ext = sd.ORBextractor(300, 1.2, 8, 20, W, H, NF)
    try:
        assert int(ext.features_per_level().sum()) == ext.cap       # download() passes the device pitch: the bulk branch
        ext.set_distortion(140.0, 140.0, 80.0, 60.0, -0.28, 0.07, 0.0002, 0.00002, 0.0)
        ext.extract_batch(frames)
        k, d, n = bulk = ext.download(0, NF)                         # more than 8 frames at the device pitch: two bulk copies
        assert (n > 20).all()
        for f in range(NF):                                          # row path, one frame at a time
            _same(ext.download(f, 1), (k[f:f + 1], d[f:f + 1], n[f:f + 1]), f"frame {f} alone")
        _same(ext.download(2, 9), (k[2:11], d[2:11], n[2:11]), "frames 2..10")
        rc, rows = _download_c(ext, 2, 9, ext.cap + 3)               # another row pitch: the row path over several frames
        assert rc == 0
        _same(rows, (k[2:11], d[2:11], n[2:11]), "frames 2..10, row path")
        un = ext.download_undistorted(0, NF)
        for f in range(NF):
            a, b = un[f, :n[f]], k[f, :n[f]]
            assert not np.array_equal(a["x"], b["x"]) and not np.array_equal(a["y"], b["y"])
            for field in ("size", "angle", "response", "octave", "class_id"):
                assert np.array_equal(a[field], b[field])
        small = int(n.max()) - 1
        rc, _ = _download_c(ext, 0, NF, small)
        assert rc == SD_ERR_CAPACITY
        rc, _ = _download_un_c(ext, 0, NF, small)
        assert rc == SD_ERR_CAPACITY
        rc, (_, _, n_only) = _download_c(ext, 0, NF, small, counts_only=True)
        assert rc == 0 and np.array_equal(n_only, n)
        for frame0, cnt in ((0, NF + 1), (NF, 1), (5, NF - 4), (-1, 2), (0, 0)):
            assert _download_c(ext, frame0, cnt, ext.cap)[0] == SD_ERR_INVALID_ARG, (frame0, cnt)
            assert _download_un_c(ext, frame0, cnt, ext.cap)[0] == SD_ERR_INVALID_ARG, (frame0, cnt)
        huge, one_k, one_n = 0x7fffffff, np.zeros(1, KP_DTYPE), np.zeros(1, np.int32)    # refused before anything is sized by it
        assert ext.L.sd_orb_download(ext.h, 0, huge, _p(one_k), None, ext.cap, _p(one_n)) == SD_ERR_INVALID_ARG
        assert ext.L.sd_orb_download_undistorted(ext.h, C.c_int(0), C.c_int(huge), _p(one_k), C.c_int(ext.cap)) == SD_ERR_INVALID_ARG
        ext.extract_batch(frames[:5])                                # a shorter batch: the range follows the LAST batch
        assert _download_c(ext, 0, 6, ext.cap)[0] == SD_ERR_INVALID_ARG
        assert _download_un_c(ext, 5, 1, ext.cap)[0] == SD_ERR_INVALID_ARG
        ext.set_distortion(140.0, 140.0, 80.0, 60.0, 0.0)            # k1 == 0: mvKeysUn = mvKeys
        ext.extract_batch(frames)
        _same(ext.download(0, NF), bulk, "after set_distortion(k1 = 0)")
        un = ext.download_undistorted(0, NF)
        for f in range(NF):
            assert np.array_equal(un[f, :n[f]], k[f, :n[f]]), f
    finally:
        ext.close()


def test_host_and_device_entry_points_agree(sd):
    """The same frames tightly packed, with padded rows and frames, and from device memory; then a second batch through the
    device entry on the same handle (own stream, behind a finished selection: the early level-0 FAST path)."""
    w, h, nf = 131, 97, 3
    a, b = _frames(80, nf, w, h), _frames(90, nf, w, h)
    cfg = (300, 1.2, 8, 20, w, h, nf)
    ext, fresh, bufs = sd.ORBextractor(*cfg), sd.ORBextractor(*cfg), []
    try:
        packed = ext.extract_batch(a)
        assert (packed[2] > 20).all()
        stride, rows = w + 5, h + 2
        padded = np.full((nf, rows, stride), 255, np.uint8)
        padded[:, :h, :w] = a
        k, d, n = np.zeros((nf, ext.cap), KP_DTYPE), np.zeros((nf, ext.cap, 32), np.uint8), np.zeros(nf, np.int32)
        assert ext.L.sd_orb_extract_batch(ext.h, _p(padded), nf, w, h, stride, rows * stride, _p(k), _p(d), ext.cap, _p(n)) == 0
        _same((k, d, n), packed, "padded host frames")
        for fr in (a, b):
            bufs.append(_device_copy(sd, fr))
        ext.extract_batch_device(bufs[0][1], nf, w, h)
        _same(ext.download(0, nf), packed, "device frames")
        ext.extract_batch_device(bufs[1][1], nf, w, h)
        second = ext.download(0, nf)
        expected = fresh.extract_batch(b)
        _same(second, expected, "second device batch on the same handle")
        assert not np.array_equal(second[0][0, :8], packed[0][0, :8])
    finally:
        ext.close()
        fresh.close()
        for buf, _ in bufs:
            buf.free()
