"""The C++ facade's sequential-tracking methods (TrackBatch::SetMapIds / SetPrior / AdvanceLastFrame / GetLastFrame /
CurrentExtractor): the program compiles and links without a GPU; on the GPU it runs a short loop whose per-frame results and
final last frame equal the same loop driven from Python, bit for bit."""
import os
import subprocess

import numpy as np
import pytest

from sdslam_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M = 1000


@pytest.fixture(scope="module")
def sd():
    import sdslam_amd
    from sdslam_amd import build
    build.build()
    return sdslam_amd


def _compile(sd, tmp_path):
    exe = str(tmp_path / "sd_facade_sequence")
    libdir = os.path.dirname(sd.lib_path())
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "native", "facade_sequence.cc"), "-o", exe,
                           "-L", libdir, "-lsdslam_hip", f"-Wl,-rpath,{libdir}"])
    return exe


def test_cpp_sequence_facade_compiles_and_links(sd, tmp_path):
    exe = _compile(sd, tmp_path)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "facade sequence ok" in out.stdout, (out.returncode, out.stdout, out.stderr)


def _cm(T):
    return np.asarray(T, np.float64).T.reshape(16)


@pytest.mark.gpu
def test_cpp_sequence_facade_matches_python_loop(sd, tmp_path):
    if sd.device_count() < 1:
        pytest.fail("no HIP device: the gpu-marked tests need a real MI355X")
    T = 6
    seq = synth.make_sequence(81, T)
    views = seq["views"]
    vel = [seq["T"][t] @ np.linalg.inv(seq["T"][t - 1]) for t in range(1, T)]
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
        recs, poses = [], []
        for t in range(1, T):
            trk.cur.extract_batch(views[t:t + 1])
            trk.set_prior(0, [vel[t - 1]], relative=True)
            trk.track_with_motion_model(1, th=15.0)
            trk.track_local_map(1, th=1.0)
            tw, tl = trk.get_tracked(0, 1), trk.get_local_map(0, 1)
            recs.append([tw["status"][0] == 2, tw["nmatches"][0], tw["nmatches_map"][0], tl["status"][0] == 2, tl["n_inliers"][0]])
            poses.append(_cm(trk.get_align(0, 1)["T"][0]))
            trk.advance(1, 1)
        py_last = trk.get_last(0, 1)
    finally:
        trk.close()
        cur.close()
        ref.close()
    inp, outp = str(tmp_path / "seq.in"), str(tmp_path / "seq.out")
    with open(inp, "wb") as f:
        nm = len(ids)
        f.write(np.array([640, 480, T, nm, M], np.int32).tobytes())
        f.write(np.ascontiguousarray(views).tobytes())
        f.write(_cm(seq["T"][0]).tobytes())
        f.write(np.stack([_cm(v) for v in vel]).tobytes())
        for key, dt in (("Xw", np.float64), ("normal", np.float64), ("min_dist", np.float32), ("max_dist", np.float32),
                        ("mf_max_dist", np.float32), ("desc", np.uint8), ("obs", np.int32)):
            f.write(np.ascontiguousarray(local[key], dt).tobytes())
        f.write(ids.astype(np.int32).tobytes())
        for key, dt in (("valid", np.uint8), ("octave", np.int32), ("angle", np.float32)):
            f.write(np.ascontiguousarray(last[key], dt).tobytes())
    exe = _compile(sd, tmp_path)
    out = subprocess.run([exe, inp, outp], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "ran" in out.stdout, (out.returncode, out.stdout, out.stderr)
    raw = open(outp, "rb").read()
    o = 0
    for t in range(T - 1):
        rec = np.frombuffer(raw, np.int32, 5, o)
        o += 20
        pose = np.frombuffer(raw, np.float64, 16, o)
        o += 128
        assert np.array_equal(rec, np.array(recs[t], np.int32)), t
        assert np.array_equal(pose, poses[t]), t
        assert rec[3] == 1, t                                         # tracked
    nl = int(np.frombuffer(raw, np.int32, 1, o)[0])
    o += 4
    assert nl == py_last["n_last"][0]
    for key, dt, w in (("valid", np.uint8, 1), ("Xw", np.float64, 3), ("desc", np.uint8, 32), ("octave", np.int32, 1),
                       ("angle", np.float32, 1), ("obs", np.int32, 1), ("ids", np.int32, 1)):
        a = np.frombuffer(raw, dt, nl * w, o)
        o += a.nbytes
        assert np.array_equal(a, py_last[key][0][:nl].reshape(-1)), key
    assert o == len(raw)
