"""CPU (no GPU): the close-point and device-depth entry points are declared in the C ABI, exported, bound in Python, and refuse a NULL
handle with SD_ERR_INVALID_ARG before touching a device."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sd():
    import sdslam_amd
    from sdslam_amd import build
    build.build()          # hipcc cross-compiles gfx950 without a GPU
    return sdslam_amd


def test_close_points_declared_exported_and_bound(sd):
    hdr = open(os.path.join(ROOT, "include", "sdslam_hip.h")).read()
    L = sd.lib()
    for name in ("sd_track_close_points", "sd_track_get_close_points", "sd_track_stereo_from_depth_device"):
        assert re.search(rf"^int {name}\(sd_track\* h,", hdr, re.M), name
        assert hasattr(L, name), name
    assert re.search(r"^#define SD_DEPTH_F32 0\b", hdr, re.M) and re.search(r"^#define SD_DEPTH_U16 1\b", hdr, re.M)
    assert (sd.Tracker.DEPTH_F32, sd.Tracker.DEPTH_U16) == (0, 1)
    for meth in ("close_points", "get_close_points", "stereo_from_depth_device"):
        assert callable(getattr(sd.Tracker, meth)), meth


def test_close_points_refuse_a_null_handle(sd):
    L = sd.lib()
    out = (C.c_int32 * 2)(-5, -5)
    assert L.sd_track_close_points(None, 1, 1, 1.0) == 1
    assert L.sd_track_get_close_points(None, 0, 1, out) == 1
    assert list(out) == [-5, -5]
    assert L.sd_track_stereo_from_depth_device(None, 1, 4096, 1, 640, 480, 640, 640 * 480, 5000.0) == 1
    assert b"handle is NULL" in L.sd_last_error()
