"""GPU: RGB-D depth maps read from device memory (sd_track_stereo_from_depth_device).

Bars: mvuRight / mvDepth equal the host call (sd_track_stereo_from_depth) on the converted map bit for bit -- both pyramids,
a distorted camera, pitched rows, padded frames, partial batches, keypoints on the map's last row and column; the conversion
is Tracking::GrabImageRGBD's (src/Tracking.cc:113-117, 147-148); the call is queued on the tracking stream without a host
wait and in order with the caller's fenced streams; a closed RGB-D loop fed from HBM equals the loop fed through the host
call."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

_CHILD = os.environ.get("SD_DEPTH_DEVICE_CHILD") == "1"
if _CHILD:
    import torch as _torch_first  # noqa: F401  (before the library: one HIP runtime in the process)

from sdslam_amd import synth  # noqa: E402

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
K = (synth.FX, synth.FY, synth.CX, synth.CY)
BOUNDS = (0.0, 640.0, 0.0, 480.0)
CFGS = {"p8": (1000, 1.2, 8, 20), "p5": (1000, 2.0, 5, 20)}
W, H = 640, 480
M = 1000
BF = 4.0
F32, U16 = 0, 1
DIST = (0.2624, -0.9531, -0.0054, 0.0026, 1.1633)   # k1 != 0: mvKeys != mvKeysUn
SLEEP = 40_000_000


@pytest.fixture(scope="module")
def sd():
    import sdslam_amd
    if sdslam_amd.device_count() < 1:
        pytest.fail("no HIP device: the gpu-marked tests need a real MI355X")
    return sdslam_amd


def _dev(sd, arr):
    arr = np.ascontiguousarray(arr)
    buf = sd.DeviceBuffer(arr.nbytes)
    buf.upload(arr)
    return buf


def _code(sd, fn):
    with pytest.raises(sd.SdError) as e:
        fn()
    return e.value.code


class Rig:
    """cur / ref extractors of B frames and a tracker; the cur frames extracted (through a distorted camera on request)."""

    def __init__(self, sd, cfg, B=4, distorted=False, seed0=900, extract=True, camera=True):
        self.B = B
        self.cur, self.ref = sd.ORBextractor(*cfg, W, H, B), sd.ORBextractor(*cfg, W, H, B)
        if distorted:
            self.cur.set_distortion(*K, *DIST)
        self.trk = sd.Tracker(self.cur, self.ref, max_points=M, max_batch=B)
        if camera:
            self.trk.set_camera(*K, BF, BOUNDS)
        if extract:
            self.cur.extract_batch(np.stack([synth.make_image(seed0 + i) for i in range(B)]))

    def close(self):
        self.trk.close()
        self.cur.close()
        self.ref.close()


def _stereo(trk, B):
    u, d = trk.get_stereo(0, B)
    return np.concatenate([u, d], 1)


@pytest.mark.parametrize("name,distorted", [("p8", False), ("p8", True), ("p5", True)])
def test_f32_device_equals_host_call(sd, name, distorted):
    """f32 maps, factor 1: the device call on a pitched, padded buffer equals the host call on the dense maps.  The maps end
    at keypoint j of frame 0 (its pixel is the last row and column; keypoints beyond are outside); holes every 7th column.
    A call on 2 of 4 slots leaves slots 2, 3 alone, as the host call does."""
    rig = Rig(sd, CFGS[name], distorted=distorted)
    trk, B = rig.trk, rig.B
    try:
        kps, _, n = rig.cur.download(0, B)
        if distorted:
            un = rig.cur.download_undistorted(0, B)
            assert np.abs(un["x"][0, :n[0]] - kps["x"][0, :n[0]]).max() > 0.5
        k0 = kps[0, :n[0]]
        j = int(np.argmin((k0["x"] / W - 0.6) ** 2 + (k0["y"] / H - 0.6) ** 2))
        w, hgt = int(k0["x"][j]) + 1, int(k0["y"][j]) + 1
        assert ((k0["x"] >= w) | (k0["y"] >= hgt)).any() and ((k0["x"] < w - 1) & (k0["y"] < hgt - 1)).any()
        rng = np.random.Generator(np.random.PCG64(7))
        maps = []
        for s in range(2):
            d = rng.uniform(0.3, 6.0, (B, hgt, w)).astype(np.float32)
            d[:, :, ::7] = 0.0
            d[:, ::11, :] = -1.0
            d[0, hgt - 1, w - 1] = 1.25 + s
            maps.append(d)
        stride, fstride = w + 13, (hgt + 3) * (w + 13) + 5
        bufs = []
        for d in maps:
            flat = np.full(B * fstride, 99.0, np.float32)          # padding: a read of it would show
            for f in range(B):
                flat[f * fstride:f * fstride + hgt * stride].reshape(hgt, stride)[:, :w] = d[f]
            bufs.append(_dev(sd, flat))
        trk.stereo_from_depth(maps[0])
        host1 = _stereo(trk, B)
        trk.stereo_from_depth(maps[1][:2])
        host2 = _stereo(trk, B)
        trk.stereo_from_depth(np.zeros((B, hgt, w), np.float32))
        trk.stereo_from_depth_device(bufs[0].ptr, F32, w, hgt, stride, fstride)
        dev1 = _stereo(trk, B)
        trk.stereo_from_depth_device(bufs[1].ptr, F32, w, hgt, stride, fstride, n_frames=2)
        dev2 = _stereo(trk, B)
        assert np.array_equal(dev1, host1) and np.array_equal(dev2, host2)
        cap = trk.cap
        assert dev1[0, cap + j] == np.float32(1.25) and dev2[0, cap + j] == np.float32(2.25)
        assert np.array_equal(dev2[2:], dev1[2:])
        dd = dev1[:, cap:]
        assert (dd == -1).sum() > B * 50 and (dd > 0).sum() > B * 50
        for b in bufs:
            b.free()
    finally:
        rig.close()


def test_conversion_rule(sd):
    """u16 at factor 5000 equals the host call on float32(raw) * (1.0f / 5000.0f); f32 at factor 2 is scaled; f32 at
    factor 1 + 5e-6 (scale within 1e-5 of 1) is not, u16 at that factor is; factor 0 means scale 1; raw 0 gives -1, raw
    65535 is accepted."""
    rig = Rig(sd, CFGS["p8"], B=2)
    trk, B = rig.trk, rig.B
    try:
        kps, _, n = rig.cur.download(0, B)
        rng = np.random.Generator(np.random.PCG64(11))
        raw = rng.integers(1, 65536, (B, H, W)).astype(np.uint16)
        raw[:, :, ::5] = 0
        k = kps[0, :n[0]]
        px = [(int(y), int(x)) for x, y in zip(k["x"], k["y"])]
        i_max = 0
        i_zero = next(i for i in range(1, n[0]) if px[i] != px[0])
        raw[0][px[i_max]] = 65535
        raw[0][px[i_zero]] = 0
        fmap = raw.astype(np.float32) * np.float32(1e-3)
        draw, dfmap = _dev(sd, raw), _dev(sd, fmap)
        s5000 = np.float32(1) / np.float32(5000)
        near = 1 + 5e-6
        s_near = np.float32(1) / np.float32(near)
        assert s_near != 1 and abs(float(s_near) - 1) < 1e-5

        def host(m):
            trk.stereo_from_depth(m)
            return _stereo(trk, B)

        def dev(buf, dtype, factor):
            trk.stereo_from_depth_device(buf.ptr, dtype, W, H, depth_map_factor=factor)
            return _stereo(trk, B)
        raw_f = raw.astype(np.float32)
        cases = [(draw, U16, 5000.0, raw_f * s5000), (draw, U16, near, raw_f * s_near), (draw, U16, 0.0, raw_f),
                 (dfmap, F32, 2.0, fmap * np.float32(0.5)), (dfmap, F32, near, fmap), (dfmap, F32, 0.0, fmap), (dfmap, F32, 1.0, fmap)]
        got = {}
        for buf, dtype, factor, want in cases:
            g = dev(buf, dtype, factor)
            assert np.array_equal(g, host(want)), (dtype, factor)
            got[(dtype, factor)] = g
        assert not np.array_equal(got[(F32, near)], host(fmap * s_near))     # scaling would have changed it
        assert not np.array_equal(got[(U16, near)], host(raw_f))             # u16 is scaled even there
        g = got[(U16, 5000.0)]
        cap = trk.cap
        assert g[0, cap + i_max] == np.float32(65535) * s5000
        assert g[0, cap + i_zero] == -1 and g[0, i_zero] == -1
        draw.free()
        dfmap.free()
    finally:
        rig.close()


def test_device_depth_errors(sd):
    """SD_ERR_INVALID_ARG: no camera, no extraction, NULL pointer / handle, unknown dtype, w or hgt < 1, stride < w, a pointer
    not aligned to its element size; SD_ERR_CAPACITY: n_frames > max_batch."""
    rig = Rig(sd, CFGS["p8"], B=2, extract=False, camera=False)
    trk = rig.trk
    buf = _dev(sd, np.zeros(2 * H * W, np.float32))
    p = buf.ptr.value
    try:
        assert _code(sd, lambda: trk.stereo_from_depth_device(p, F32, W, H)) == 1           # no camera
        trk.set_camera(*K, BF, BOUNDS)
        assert _code(sd, lambda: trk.stereo_from_depth_device(p, F32, W, H)) == 1           # no extraction
        rig.cur.extract_batch(np.stack([synth.make_image(1)] * 2))
        trk.stereo_from_depth_device(p, F32, W, H)
        trk.stereo_from_depth_device(p + 2, U16, W, H, depth_map_factor=5000.0)             # aligned for u16
        trk.get_stereo(0, 2)
        assert _code(sd, lambda: trk.stereo_from_depth_device(p, F32, W, H, n_frames=3)) == 3
        assert _code(sd, lambda: trk.stereo_from_depth_device(None, F32, W, H)) == 1
        for dt in (-1, 2):
            assert _code(sd, lambda: trk.stereo_from_depth_device(p, dt, W, H)) == 1
        assert _code(sd, lambda: trk.stereo_from_depth_device(p, F32, 0, H, stride=W)) == 1
        assert _code(sd, lambda: trk.stereo_from_depth_device(p, F32, W, 0, frame_stride=W * H)) == 1
        assert _code(sd, lambda: trk.stereo_from_depth_device(p, F32, W, H, stride=W - 1)) == 1
        assert _code(sd, lambda: trk.stereo_from_depth_device(p + 2, F32, W, H)) == 1
        assert _code(sd, lambda: trk.stereo_from_depth_device(p + 1, U16, W, H)) == 1
        assert trk.L.sd_track_stereo_from_depth_device(None, 1, p, F32, W, H, W, W * H, 1.0) == 1
    finally:
        buf.free()
        rig.close()


def _download(ptr, nbytes):
    from sdslam_amd import capi
    out = np.zeros(nbytes, np.uint8)
    capi._check(capi.lib().sd_dev_download(out.ctypes.data_as(ctypes.c_void_p), ptr, nbytes))
    return out


def _rgbd_loop(sd, seqs, raw, device, th_close):
    """2 streams: extraction from HBM -> depth -> prior -> TrackWithMotionModel -> TrackLocalMap -> close points -> records ->
    hand-off, T-1 frames.  device: u16 maps in HBM, factor 5000; else the host call on the converted f32 maps (it
    synchronises inside).  Nothing is read back until after the last frame."""
    B, T = len(seqs), raw.shape[0]
    views = np.stack([s["views"] for s in seqs], 1)
    ext = [sd.ORBextractor(*CFGS["p8"], W, H, B) for _ in range(2)]
    trk = sd.Tracker(ext[0], ext[1], max_points=M, max_batch=B, pnp_max_iterations=100)
    try:
        trk.set_camera(*K, BF, BOUNDS)
        rk, rd, rn = trk.ref.extract_batch(views[0])
        maps = [synth.static_map(rk[b, :rn[b]], rd[b, :rn[b]], seqs[b]["T"][0], seed=b) for b in range(B)]
        trk.set_last(0, [m[1] for m in maps])
        trk.set_local(0, [m[0] for m in maps])
        trk.set_map_ids(0, [m[2] for m in maps], 0)
        trk.set_map_ids(0, [m[2] for m in maps], 1)
        trk.set_poses(0, [s["T"][0] for s in seqs], [s["T"][0] for s in seqs])
        frames, rec = _dev(sd, views), sd.DeviceBuffer(T * B * 160)
        dmaps = _dev(sd, raw) if device else None
        conv = raw.astype(np.float32) * (np.float32(1) / np.float32(5000))
        for t in range(1, T):
            trk.cur.extract_batch_device(frames.ptr.value + t * B * W * H, B, W, H)
            if device:
                trk.stereo_from_depth_device(dmaps.ptr.value + t * B * W * H * 2, U16, W, H, depth_map_factor=5000.0)
            else:
                trk.stereo_from_depth(conv[t])
            trk.set_prior(0, [s["T"][t] @ np.linalg.inv(s["T"][t - 1]) for s in seqs], relative=True)
            trk.track_with_motion_model(B, th=15.0, mono=False, align_mode=0)
            trk.track_local_map(B, th=3.0, min_inliers=30)
            trk.close_points(B, 1, th_close)
            trk.pack_records(B, 3, rec.ptr.value + t * B * 160)
            trk.advance(B, 1)
        out = dict(last=trk.get_last(0, B), local_map=trk.get_local_map(0, B), matches=trk.get_matches(0, B),
                   close=trk.get_close_points(0, B), stereo=_stereo(trk, B), records=_download(rec.ptr, T * B * 160)[B * 160:])
        for b_ in (frames, rec, dmaps):
            if b_ is not None:
                b_.free()
        return out
    finally:
        trk.close()
        for e in ext:
            e.close()


def test_closed_rgbd_loop_from_hbm_equals_host_depth_loop(sd):
    """2 streams x 8 frames with views and 16-bit depth (factor 5000) resident in HBM: records (status, matches, inliers,
    pose of every frame), the last frame's matches, stereo and close-point counts and the final hand-off equal the same loop
    driven through the host call on the converted f32 maps (the loop test_closed_loop_rgbd pins to the oracle)."""
    seqs = [synth.make_sequence(s, 8, with_depth=True) for s in (21, 22)]
    raw = np.round(np.stack([s["depth"] for s in seqs], 1) * 5000.0).astype(np.uint16)
    raw[..., ::11] = 0
    a = _rgbd_loop(sd, seqs, raw, True, 2.0)
    b = _rgbd_loop(sd, seqs, raw, False, 2.0)
    assert np.array_equal(a["records"], b["records"])
    recs = a["records"].view(np.float64).reshape(-1, 20)
    assert (recs[:, 19] == 1).all() and (recs[:, 17] > 50).all()
    for key in ("local_map", "close", "last"):
        for k in a[key]:
            assert np.array_equal(a[key][k], b[key][k]), (key, k)
    assert np.array_equal(a["matches"][0], b["matches"][0]) and np.array_equal(a["stereo"], b["stereo"])
    assert (a["close"]["tracked"] > 0).all() and (a["close"]["non_tracked"] > 0).all()


# ---- ordering against a caller's streams (child process with torch loaded first, as tests/test_stream_order_gpu.py)

def _in_child(request):
    if _CHILD:
        return True
    cmd = [sys.executable] + (["-s"] if sys.flags.no_user_site else []) + [
        "-m", "pytest", f"{request.node.path}::{request.node.name}", "-m", "gpu", "-q", "-p", "no:cacheprovider"]
    env = dict(os.environ, SD_DEPTH_DEVICE_CHILD="1", GPU_MAX_HW_QUEUES="16")
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and " passed" in r.stdout, r.stdout[-6000:] + r.stderr[-2000:]
    return False


def _stream(torch):
    hip = ctypes.CDLL("libamdhip64.so.7")
    p = ctypes.c_void_p()
    assert hip.hipStreamCreateWithFlags(ctypes.byref(p), ctypes.c_uint(1)) == 0   # hipStreamNonBlocking
    return torch.cuda.ExternalStream(p.value)


def _two_maps(torch):
    """Two 16-bit depth maps (as int16 bits) for 4 frames that differ everywhere, on the device."""
    rng = np.random.Generator(np.random.PCG64(5))
    a = rng.integers(3000, 15000, (4, H, W)).astype(np.uint16)
    b = rng.integers(3000, 15000, (4, H, W)).astype(np.uint16)
    return [torch.from_numpy(m.view(np.int16)).cuda() for m in (a, b)]


def _call(trk, d):
    trk.stereo_from_depth_device(d.data_ptr(), U16, W, H, depth_map_factor=5000.0)


def test_fenced_upload_is_read_without_host_wait(sd, request):
    if not _in_child(request):
        return
    import torch
    """The upload of the maps sits on a caller's stream behind a delay and is fenced with direction 1: the call returns
    while the delay is pending and reads the uploaded maps (equal to a synchronised run)."""
    rig = Rig(sd, CFGS["p8"])
    trk = rig.trk
    try:
        A, Bm = _two_maps(torch)
        d = A.clone()
        torch.cuda.synchronize()
        _call(trk, Bm)
        want = _stereo(trk, rig.B)
        _call(trk, A)
        assert not np.array_equal(_stereo(trk, rig.B), want)
        S = _stream(torch)
        with torch.cuda.stream(S):
            torch.cuda._sleep(SLEEP)
            d.copy_(Bm)
        trk.stream_fence(S.cuda_stream, 1)
        _call(trk, d)
        assert not S.query(), "the delay ended before the call returned: the test proved nothing"
        assert np.array_equal(_stereo(trk, rig.B), want)
    finally:
        rig.close()


def test_direction0_fence_protects_the_maps_being_read(sd, request):
    if not _in_child(request):
        return
    import torch
    """The call is held back behind a fenced delay; after sd_track_stream_fence(S, 0) the caller overwrites the maps on S.
    The results are those of the old contents."""
    rig = Rig(sd, CFGS["p8"])
    trk = rig.trk
    try:
        A, Bm = _two_maps(torch)
        d = A.clone()
        torch.cuda.synchronize()
        _call(trk, A)
        want = _stereo(trk, rig.B)
        trk.stereo_from_depth(np.zeros((rig.B, H, W), np.float32))
        S2, S = _stream(torch), _stream(torch)
        with torch.cuda.stream(S2):
            torch.cuda._sleep(SLEEP)
        trk.stream_fence(S2.cuda_stream, 1)
        _call(trk, d)
        trk.stream_fence(S.cuda_stream, 0)
        with torch.cuda.stream(S):
            d.copy_(Bm)
        assert not S2.query(), "the delay ended before the call was queued"
        assert not S.query(), "the overwrite was not held behind the call"
        assert np.array_equal(_stereo(trk, rig.B), want)
        S.synchronize()
        assert torch.equal(d, Bm)
    finally:
        rig.close()
