"""The C++ facade's RGB-D calls (TrackBatch::ComputeStereoFromRGBD on a 16-bit map in device memory, CloseTrackedPoints /
CloseTrackedPointsResult): the program compiles and links without a GPU; on the GPU its counts after TrackWithMotionModel
(source 0) and TrackLocalMap (source 1) equal the same frame pair driven from Python."""
import os
import subprocess

import numpy as np
import pytest

from sdslam_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M = 1000
BF = 4.0


@pytest.fixture(scope="module")
def sd():
    import sdslam_amd
    from sdslam_amd import build
    build.build()
    return sdslam_amd


def _compile(sd, tmp_path):
    exe = str(tmp_path / "sd_facade_close_points")
    libdir = os.path.dirname(sd.lib_path())
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "native", "facade_close_points.cc"), "-o", exe,
                           "-L", libdir, "-lsdslam_hip", f"-Wl,-rpath,{libdir}"])
    return exe


def test_cpp_close_points_facade_compiles_and_links(sd, tmp_path):
    exe = _compile(sd, tmp_path)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "facade close points ok" in out.stdout, (out.returncode, out.stdout, out.stderr)


def _cm(T):
    return np.asarray(T, np.float64).T.reshape(16)


@pytest.mark.gpu
def test_cpp_close_points_facade_matches_python(sd, tmp_path):
    if sd.device_count() < 1:
        pytest.fail("no HIP device: the gpu-marked tests need a real MI355X")
    seq = synth.make_sequence(83, 2, with_depth=True)
    views = seq["views"]
    raw = np.round(seq["depth"][1] * 5000.0).astype(np.uint16)
    raw[:, ::9] = 0
    depth = raw.astype(np.float32) * (np.float32(1) / np.float32(5000))
    vel = seq["T"][1] @ np.linalg.inv(seq["T"][0])
    th = np.float32(np.median(depth[depth > 0]))
    cur, ref = sd.ORBextractor(1000, 1.2, 8, 20, 640, 480, 1), sd.ORBextractor(1000, 1.2, 8, 20, 640, 480, 1)
    trk = sd.Tracker(cur, ref, max_points=M, max_batch=1, pnp_max_iterations=100)
    try:
        trk.set_camera(*seq["K"], BF, (0.0, 640.0, 0.0, 480.0))
        k, d, n = trk.ref.extract_batch(views[:1])
        local, last, ids = synth.static_map(k[0, :n[0]], d[0, :n[0]], seq["T"][0])
        trk.set_last(0, [last])
        trk.set_local(0, [local])
        trk.set_poses(0, [seq["T"][0]], [seq["T"][0]])
        trk.cur.extract_batch(views[1:2])
        dmap = sd.DeviceBuffer(raw.nbytes)
        dmap.upload(raw)
        trk.stereo_from_depth_device(dmap.ptr, trk.DEPTH_U16, 640, 480, depth_map_factor=5000.0)
        trk.set_prior(0, [vel], relative=True)
        trk.track_with_motion_model(1, th=15.0, mono=False)
        trk.close_points(1, 0, th)
        c0 = trk.get_close_points(0, 1)
        trk.track_local_map(1, th=3.0)
        trk.close_points(1, 1, th)
        c1 = trk.get_close_points(0, 1)
        dmap.free()
    finally:
        trk.close()
        cur.close()
        ref.close()
    want = np.array([c0["tracked"][0], c0["non_tracked"][0], c1["tracked"][0], c1["non_tracked"][0]], np.int32)
    assert (want > 0).all(), want
    inp, outp = str(tmp_path / "close.in"), str(tmp_path / "close.out")
    with open(inp, "wb") as f:
        f.write(np.array([640, 480, len(ids), M], np.int32).tobytes())
        f.write(np.array([BF, th, 5000.0], np.float32).tobytes())
        f.write(np.ascontiguousarray(views).tobytes())
        f.write(raw.tobytes())
        f.write(_cm(seq["T"][0]).tobytes())
        f.write(_cm(vel).tobytes())
        for key, dt in (("Xw", np.float64), ("normal", np.float64), ("min_dist", np.float32), ("max_dist", np.float32),
                        ("mf_max_dist", np.float32), ("desc", np.uint8), ("obs", np.int32)):
            f.write(np.ascontiguousarray(local[key], dt).tobytes())
        for key, dt in (("valid", np.uint8), ("octave", np.int32), ("angle", np.float32)):
            f.write(np.ascontiguousarray(last[key], dt).tobytes())
    exe = _compile(sd, tmp_path)
    out = subprocess.run([exe, inp, outp], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "ran" in out.stdout, (out.returncode, out.stdout, out.stderr)
    got = np.fromfile(outp, np.int32)
    assert np.array_equal(got, want), (got, want)
