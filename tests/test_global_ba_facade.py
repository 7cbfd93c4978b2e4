"""The C++ facade's Optimizer::BundleAdjustment / GlobalBundleAdjustemnt on the GPU: tests/native/facade_global_ba.cc checks the roles
and CSR lists the facade builds against lists typed in, then plants six keyframes with mock KeyFrame / MapPoint / Map objects, runs
both nLoopKF branches and compares what the objects were given, byte for byte, with sd_debug_global_ba on lists built by straight
loops; the order of the SetPose / SetWorldPos / refresh calls with the reference's; the normals and distances with a restatement of
UpdateNormalAndDepth; and checks that a set stop flag and two refusals return false and touch nothing."""
import os
import subprocess

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_facade_global_ba_on_the_device(tmp_path):
    import sdslam_amd
    if sdslam_amd.device_count() < 1:
        pytest.fail("no HIP device: the gpu-marked tests need a real MI355X")
    exe = str(tmp_path / "sd_facade_global_ba")
    libdir = os.path.dirname(sdslam_amd.lib_path())
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-O1", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "native", "facade_global_ba.cc"), "-o", exe, "-L", libdir, "-lsdslam_hip",
                           f"-Wl,-rpath,{libdir}"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "facade_global_ba OK" in out.stdout, out.stdout + out.stderr
