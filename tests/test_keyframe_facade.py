"""The C++ facade's RGB-D map point calls (TrackBatch::StereoInitialization / CreatedPoints, Tracking::NeedNewKeyFrame /
CreateNewKeyFrame): the program compiles and links without a GPU; on the GPU its creation records after the initialisation and
after the first tracked frame, its decision byte and the ids of its handed-off last frame equal the same frames driven from
Python."""
import os
import subprocess

import numpy as np
import pytest

from sdslam_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
M = 1000
BF = 4.0
TH = np.float32(2.0)
STATE = np.array([1, 2000, 0, 0, 1, 0, 0, 0], np.int32)     # one keyframe, idle mapper: c1b and c2 hold on frame 1
NEXT_ID = 77


@pytest.fixture(scope="module")
def sd():
    import sdslam_amd
    from sdslam_amd import build
    build.build()
    return sdslam_amd


def _compile(sd, tmp_path):
    exe = str(tmp_path / "sd_facade_keyframe")
    libdir = os.path.dirname(sd.lib_path())
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "native", "facade_keyframe.cc"), "-o", exe,
                           "-L", libdir, "-lsdslam_hip", f"-Wl,-rpath,{libdir}"])
    return exe


def test_cpp_keyframe_facade_compiles_and_links(sd, tmp_path):
    exe = _compile(sd, tmp_path)
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "facade keyframe ok" in out.stdout, (out.returncode, out.stdout, out.stderr)


def _record(buf, pos):
    mode, n, P, cand = np.frombuffer(buf, np.int32, 4, pos)
    pos += 16
    kp = np.frombuffer(buf, np.int32, n, pos)
    ids = np.frombuffer(buf, np.int32, n, pos + 4 * n)
    Xw = np.frombuffer(buf, np.float64, 3 * n, pos + 8 * n).reshape(n, 3)
    return dict(mode=mode, created=n, P=P, candidates=cand, kp_index=kp, ids=ids, Xw=Xw), pos + 32 * n


@pytest.mark.gpu
def test_cpp_keyframe_facade_matches_python(sd, tmp_path):
    if sd.device_count() < 1:
        pytest.fail("no HIP device: the gpu-marked tests need a real MI355X")
    seq = synth.make_sequence(84, 2, with_depth=True)
    views = seq["views"]
    raw = np.round(seq["depth"] * 5000.0).astype(np.uint16)
    raw[:, :, ::9] = 0
    vel = seq["T"][1] @ np.linalg.inv(seq["T"][0])
    cur, ref = sd.ORBextractor(1000, 1.2, 8, 20, 640, 480, 1), sd.ORBextractor(1000, 1.2, 8, 20, 640, 480, 1)
    trk = sd.Tracker(cur, ref, max_points=M, max_batch=1, pnp_max_iterations=100)
    try:
        trk.set_camera(*seq["K"], BF, (0.0, 640.0, 0.0, 480.0))
        dmap = sd.DeviceBuffer(raw.nbytes)
        dmap.upload(raw)
        trk.set_next_map_id(0, [NEXT_ID])
        trk.set_keyframe_state(0, STATE[None])
        trk.cur.extract_batch(views[:1])
        trk.stereo_from_depth_device(dmap.ptr.value, trk.DEPTH_U16, 640, 480, depth_map_factor=5000.0)
        trk.stereo_init(1)
        c0 = trk.get_created(0, 1)
        trk.advance(1, 2)
        trk.cur.extract_batch(views[1:2])
        trk.stereo_from_depth_device(dmap.ptr.value + raw[0].nbytes, trk.DEPTH_U16, 640, 480, depth_map_factor=5000.0)
        trk.set_prior(0, [vel], relative=True)
        trk.track_with_motion_model(1, th=15.0, mono=False)
        trk.track_local_map(1, th=3.0)
        trk.close_points(1, 1, TH)
        trk.need_keyframe(1, True, 1, 0, 30)
        trk.create_keyframe_points(1, 1, TH, use_flags=True, frame_id=1)
        flag = trk.get_keyframe_flags(0, 1)[0]
        c1 = trk.get_created(0, 1)
        trk.advance(1, 1)
        last = trk.get_last(0, 1)
        dmap.free()
    finally:
        trk.close()
        cur.close()
        ref.close()
    assert c0["mode"][0] == 2 and c0["created"][0] > 500 and flag == 1 and c1["mode"][0] == 1 and c1["created"][0] > 50
    inp, outp = str(tmp_path / "kf.in"), str(tmp_path / "kf.out")
    with open(inp, "wb") as f:
        f.write(np.array([640, 480, M, NEXT_ID, 0, 30], np.int32).tobytes())
        f.write(STATE.tobytes())
        f.write(np.array([BF, TH, 5000.0], np.float32).tobytes())
        f.write(np.ascontiguousarray(views).tobytes())
        f.write(raw.tobytes())
        f.write(np.asarray(vel, np.float64).T.reshape(16).tobytes())
    exe = _compile(sd, tmp_path)
    out = subprocess.run([exe, inp, outp], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "ran" in out.stdout, (out.returncode, out.stdout, out.stderr)
    buf = open(outp, "rb").read()
    g0, pos = _record(buf, 0)
    gflag = np.frombuffer(buf, np.int32, 1, pos)[0]
    g1, pos = _record(buf, pos + 4)
    n = np.frombuffer(buf, np.int32, 1, pos)[0]
    gids = np.frombuffer(buf, np.int32, n, pos + 4)
    assert gflag == flag
    for g, c in ((g0, c0), (g1, c1)):
        k = int(c["created"][0])
        assert (g["mode"], g["created"], g["P"], g["candidates"]) == (c["mode"][0], k, c["P"][0], c["candidates"][0])
        assert np.array_equal(g["kp_index"], c["kp_index"][0, :k]) and np.array_equal(g["ids"], c["ids"][0, :k])
        assert np.array_equal(g["Xw"], c["Xw"][0, :k])
    assert n == last["n_last"][0] and np.array_equal(gids, last["ids"][0, :n])
