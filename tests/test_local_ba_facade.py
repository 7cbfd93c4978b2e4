"""The C++ facade's Optimizer::LocalBundleAdjustment on the GPU: tests/native/facade_local_ba.cc plants seven keyframes (four local
ones, one of them fixed by its id, two fixed cameras, the current keyframe) with reference-shaped KeyFrame / MapPoint objects,
runs the method once on a scene with wrong observations and once without, and compares the poses and positions the objects
were given, byte for byte, with sd_debug_local_ba on lists built by straight loops; the EraseMapPointMatch / EraseObservation
calls with the erase flags in the reference's order; the normals and distances with a restatement of UpdateNormalAndDepth over
the observations as they are afterwards; and checks that pbStopFlag and a refusal touch nothing.  (The host part alone, under
sanitizers, is in tests/test_local_ba_cpu.py.)"""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_facade_local_ba_on_the_device(tmp_path):
    import sdslam_amd
    if sdslam_amd.device_count() < 1:
        pytest.fail("no HIP device: the gpu-marked tests need a real MI355X")
    exe = str(tmp_path / "sd_facade_local_ba")
    libdir = os.path.dirname(sdslam_amd.lib_path())
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-O1", "-ffp-contract=off", "-DRUN_ON_GPU", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "native", "facade_local_ba.cc"), "-o", exe, "-L", libdir, "-lsdslam_hip",
                           f"-Wl,-rpath,{libdir}"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "facade_local_ba OK" in out.stdout, out.stdout + out.stderr
