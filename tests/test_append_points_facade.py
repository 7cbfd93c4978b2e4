"""The C++ facade's appending ORBmatcher::CreateNewMapPoints overload (include/sdslam/sdslam.hpp) without a GPU:
tests/native/facade_append_points.cc instantiates the template against toy KeyFrame / MapPoint classes with the reference's member
names, links against the library, and runs the in-order walk (new MapPoint at its row position, AddObservation x 2, AddMapPoint
x 2, mlpRecentAddedMapPoints, no object for a dropped point) on rows it writes itself, checking every object afterwards."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def sd():
    import sdslam_amd
    from sdslam_amd import build
    build.build()          # hipcc cross-compiles gfx950 without a GPU
    return sdslam_amd


def test_cpp_append_points_facade_walks_the_rows_in_order(sd, tmp_path):
    exe = str(tmp_path / "sd_facade_append_points")
    libdir = os.path.dirname(sd.lib_path())
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "native", "facade_append_points.cc"), "-o", exe,
                           "-L", libdir, "-lsdslam_hip", f"-Wl,-rpath,{libdir}"])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "facade append points ok" in out.stdout, (out.returncode, out.stdout, out.stderr)
