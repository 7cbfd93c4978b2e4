"""The C++ facade's IMU sensor-model methods (TrackBatch::SetSensorModel / SetMeasurements / ImuState): on the GPU
tests/native/facade_imu.cc tracks three frames of one stream with the device's IMU prior; its X, P, gravity and final pose per
frame equal the same frames driven from Python, byte for byte.  (The link check without a GPU is in tests/test_imu_cpu.py.)"""
import os
import subprocess

import numpy as np
import pytest

from sdslam_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M = 1000
DT = 1.0 / 30.0


def _cm(T):
    return np.asarray(T, np.float64).T.reshape(16)


@pytest.mark.gpu
def test_cpp_imu_facade_matches_python_loop(tmp_path):
    import sdslam_amd as sd
    from sdslam_amd import build
    build.build()
    if sd.device_count() < 1:
        pytest.fail("no HIP device: the gpu-marked tests need a real MI355X")
    T = 4
    seq = synth.make_sequence(81, T)
    views = seq["views"]
    rng = np.random.Generator(np.random.PCG64(7))
    meas = np.concatenate([rng.uniform(-0.02, 0.02, (T, 3)), np.tile([0.0, 1.0, 0.0], (T, 1))], 1)
    cur, ref = sd.ORBextractor(1000, 1.2, 8, 20, 640, 480, 1), sd.ORBextractor(1000, 1.2, 8, 20, 640, 480, 1)
    trk = sd.Tracker(cur, ref, max_points=M, max_batch=1, pnp_max_iterations=100)
    try:
        trk.set_camera(*seq["K"], 0.0, (0.0, 640.0, 0.0, 480.0))
        k, d, n = trk.ref.extract_batch(views[:1])
        local, last, ids = synth.static_map(k[0, :n[0]], d[0, :n[0]], seq["T"][0])
        trk.set_last(0, [last])
        trk.set_local(0, [local])
        trk.set_map_ids(0, [ids], 0)
        trk.set_map_ids(0, [ids], 1)
        trk.set_poses(0, [seq["T"][0]], [seq["T"][0]])
        trk.set_sensor_model(1)
        want = []
        for t in range(1, T):
            trk.cur.extract_batch(views[t:t + 1])
            trk.set_measurements(0, meas[t:t + 1])
            trk.motion_predict(1, DT)
            trk.track_with_motion_model(1, th=15.0)
            trk.track_local_map(1, th=1.0)
            trk.motion_update(1, 1)
            im = trk.get_imu(0, 1)
            want.append((int(im["started"][0]), im["X"][0].copy(), im["P"][0].copy(), im["gravity"][0].copy(), _cm(trk.get_align(0, 1)["T"][0])))
            assert trk.get_local_map(0, 1)["status"][0] == 2, t
            trk.advance(1, 1)
    finally:
        trk.close()
        cur.close()
        ref.close()
    assert want[-1][0] == 1 and np.abs(want[-1][1][7:10]).max() > 1e-3 and want[-1][3][1] > 0.05   # started, a velocity, gravity
    inp, outp = str(tmp_path / "imu.in"), str(tmp_path / "imu.out")
    with open(inp, "wb") as f:
        f.write(np.array([640, 480, T, len(ids), M], np.int32).tobytes())
        f.write(np.array([DT], np.float64).tobytes())
        f.write(np.ascontiguousarray(meas).tobytes())
        f.write(np.ascontiguousarray(views).tobytes())
        f.write(_cm(seq["T"][0]).tobytes())
        for key, dt in (("Xw", np.float64), ("normal", np.float64), ("min_dist", np.float32), ("max_dist", np.float32),
                        ("mf_max_dist", np.float32), ("desc", np.uint8), ("obs", np.int32)):
            f.write(np.ascontiguousarray(local[key], dt).tobytes())
        f.write(ids.astype(np.int32).tobytes())
        for key, dt in (("valid", np.uint8), ("octave", np.int32), ("angle", np.float32)):
            f.write(np.ascontiguousarray(last[key], dt).tobytes())
    exe = str(tmp_path / "sd_facade_imu")
    libdir = os.path.dirname(sd.lib_path())
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "native", "facade_imu.cc"), "-o", exe,
                           "-L", libdir, "-lsdslam_hip", f"-Wl,-rpath,{libdir}"])
    out = subprocess.run([exe, inp, outp], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "ran" in out.stdout, (out.returncode, out.stdout, out.stderr)
    raw = open(outp, "rb").read()
    o = 0
    for t in range(T - 1):
        started = int(np.frombuffer(raw, np.int32, 1, o)[0])
        X = np.frombuffer(raw, np.float64, 16, o + 4)
        P = np.frombuffer(raw, np.float64, 256, o + 132)
        g = np.frombuffer(raw, np.float64, 3, o + 2180)
        pose = np.frombuffer(raw, np.float64, 16, o + 2204)
        o += 2332
        assert started == want[t][0], t
        assert X.tobytes() == want[t][1].tobytes() and P.tobytes() == want[t][2].tobytes() and g.tobytes() == want[t][3].tobytes(), t
        assert pose.tobytes() == want[t][4].tobytes(), t
    assert o == len(raw)
