"""The C++ facade's ORBmatcher::RefreshMapPoints on the GPU: tests/native/facade_refresh.cc extracts two small batches, builds toy
KeyFrame / MapPoint objects over the device's keypoints (a bad keyframe, a keyframe that is not resident, a bad point, a point
without observations), runs the method and compares every point's descriptor, normal and distances bit for bit with a straight
C++ restatement of src/MapPoint.cc:225-343 over the same iteration order, then reads the local row back: it holds the refreshed
fields, and the bytes of the points left alone.  (The host part alone, under sanitizers, is in tests/test_refresh_cpu.py.)"""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_facade_refresh_on_the_device(tmp_path):
    import sdslam_amd
    if sdslam_amd.device_count() < 1:
        pytest.fail("no HIP device: the gpu-marked tests need a real MI355X")
    exe = str(tmp_path / "sd_facade_refresh")
    libdir = os.path.dirname(sdslam_amd.lib_path())
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-O1", "-ffp-contract=off", "-DRUN_ON_GPU", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "native", "facade_refresh.cc"), "-o", exe, "-L", libdir, "-lsdslam_hip",
                           f"-Wl,-rpath,{libdir}"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "facade_refresh OK" in out.stdout, out.stdout + out.stderr
