"""The C++ facade's LocalMapping::KeyFrameCulling and the erase_on_device path of Optimizer::LocalBundleAdjustment:
tests/native/facade_cull.cc, with keyframes and points that cascade as the reference's do.  Host side (no GPU): the candidates
and flags from GetVectorCovisibleKeyFrames(), mnId and the not-erase predicate, the SetBadFlag calls and their order for a verdict
array, and the device part's scene under a straight restatement of the reference's loop.  On the GPU: the method on planted
keyframes against that restatement on a twin scene (SetBadFlag order, every object's state), a device refusal and a covisible
keyframe that is not resident (false, nothing touched), and LocalBundleAdjustment with erase_on_device false and true on twin
scenes with wrong observations, every object compared."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_and_run(tmp_path, defines):
    import sdslam_amd
    exe = str(tmp_path / "sd_facade_cull")
    libdir = os.path.dirname(sdslam_amd.lib_path())
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-O1", "-ffp-contract=off"] + defines + ["-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "native", "facade_cull.cc"), "-o", exe, "-L", libdir, "-lsdslam_hip",
                           f"-Wl,-rpath,{libdir}"])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    print(out.stdout)
    assert out.returncode == 0 and "facade_cull OK" in out.stdout, out.stdout + out.stderr


def test_facade_cull_host_side(tmp_path):
    from sdslam_amd import build
    build.build()                                                           # hipcc cross-compiles gfx950 without a GPU
    build_and_run(tmp_path, [])


@pytest.mark.gpu
def test_facade_cull_on_the_device(tmp_path):
    import sdslam_amd
    if sdslam_amd.device_count() < 1:
        pytest.fail("no HIP device: the gpu-marked tests need a real MI355X")
    build_and_run(tmp_path, ["-DRUN_ON_GPU"])
