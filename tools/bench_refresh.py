"""Time the map-point refresh that ends LocalMapping::SearchInNeighbors (ComputeDistinctiveDescriptors + UpdateNormalAndDepth) for
1000 points, two ways, each behind a queued sd_track_fuse over the keyframes:

  (a) the path before sd_track_refresh_points: sd_track_get_fuse (the host wait and download), both functions on the host, and
      the upload of the refreshed fields through sd_track_set_local;
  (b) sd_track_set_observations + sd_track_refresh_points(write_local = 1) queued behind the same fuse, ended by
      sd_track_get_refreshed (the statuses and fields the caller's MapPoint objects need in either path).

    python tools/bench_refresh.py [--points 1000] [--keyframes 32] [--out profiles/refresh_bench.jsonl]

Observation counts: 90 % of the points 1 + geometric(p = 0.2) clipped to 60 (mean about 6), 8 % uniform in 60..200, 2 % uniform in
240..256 (near the cap of 256); 10 % of the observations belong to a bad keyframe.  Observations name random keypoints of the
--keyframes resident frames and of the current keyframe (a point's list may name a frame more than once: timing only).
The host side of (a) is timed twice: tools/refresh_host.cc, a straight C++ loop built with g++ -O2 -ffp-contract=off (its
results must equal the device's bit for bit), and the numpy restatement tests/refresh_ref.py on --numpy-points points,
extrapolated by observation-pair count.
Method (measuring guide): 20 untimed calls, then batches of 20 calls, each call ended by its synchronising getter, until 1 s has
passed; host wall clock; mean and min / max over the batches.  Appends one JSON line to --out."""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def timed(call, sync):
    for _ in range(20):
        call()
    sync()
    batches, t = [], 0.0
    while t < 1.0:
        t0 = time.perf_counter()
        for _ in range(20):
            call()
            sync()
        dt = time.perf_counter() - t0
        t += dt
        batches.append(1e3 * dt / 20)
    return dict(mean=round(float(np.mean(batches)), 4), min=round(min(batches), 4), max=round(max(batches), 4), batches=len(batches))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--points", type=int, default=1000)
    ap.add_argument("--keyframes", type=int, default=32)
    ap.add_argument("--numpy-points", type=int, default=100)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "refresh_bench.jsonl"))
    a = ap.parse_args()
    import sdslam_amd as sd
    import refresh_ref as RR
    from sdslam_amd import capi, synth
    W, H, NF, B, P = 640, 480, 1000, a.keyframes, a.points
    K = (synth.FX, synth.FY, synth.CX, synth.CY)
    cfg = (NF, 1.2, 8, 20)
    cur, ref = sd.ORBextractor(*cfg, W, H, 1), sd.ORBextractor(*cfg, W, H, B)
    tex = synth.make_image(31, 2 * W, 2 * H)
    rng = np.random.default_rng(7)
    T1 = synth.se3_exp((0.01, 0.0, 0.0), (0.1, -0.2, 0.1))
    T2 = [synth.se3_exp((0.2, 0.03, 0.03) * rng.uniform(-1.5, 1.5, 3), rng.uniform(-0.5, 0.5, 3)) @ T1 for _ in range(B)]
    k1, d1, n1 = cur.extract_batch(np.stack([synth.render_plane_view(tex, T1, W, H)]))
    k2, d2, n2 = ref.extract_batch(np.stack([synth.render_plane_view(tex, T, W, H) for T in T2]))
    trk = sd.Tracker(cur, ref, max_points=P, max_batch=B, pnp_max_iterations=8)
    trk.set_camera(*K, 0.0, (0.0, float(W), 0.0, float(H)))
    trk.set_poses(0, T2, [T1] * B)
    trk.set_uright_ref(0, np.full((B, trk.cap), -1, np.float32))
    # the points: surface points the current keyframe's keypoints see, with the fields a Fuse upload carries
    pts = synth.local_map_case(3, k1[0, :n1[0]][:P], d1[0, :n1[0]][:P], T1, n_extra=max(0, P - int(n1[0])))
    pts = {k: np.asarray(v)[:P] for k, v in pts.items()}
    P = len(pts["cand"])
    u = rng.random(P)
    counts = np.where(u < 0.90, np.minimum(rng.geometric(0.2, P), 60), np.where(u < 0.98, rng.integers(60, 201, P), rng.integers(240, 257, P)))
    nmin = int(min(n1[0], n2.min()))
    obs = [[(int(f), int(k), int(b)) for f, k, b in zip(rng.integers(-1, B, c), rng.integers(0, nmin, c), rng.random(c) < 0.1)] for c in counts]
    ref_obs = np.array([rng.integers(0, c) for c in counts], np.int32)
    trk.set_local(0, [pts] * B)
    fuse = lambda: trk.fuse(B, kf_side=1, point_row=0, th=3.0)

    def device():
        fuse()
        trk.set_observations(obs, ref_obs)
        trk.refresh_points(0, True)
    ms_b = timed(device, trk.get_refreshed)
    ms_fuse = timed(fuse, lambda: trk.get_fuse(0, B))                        # (a) starts with this: the wait and the download
    off, fr, kp, kb = capi._refresh_csr(obs)
    ms_b_prepared = timed(lambda: (fuse(), capi._check(trk.L.sd_track_set_observations(trk.h, P, capi._p(off), capi._p(fr), capi._p(kp),
                                                                                      capi._p(kb), capi._p(ref_obs), None)),
                                   trk.refresh_points(0, True)), trk.get_refreshed)
    device()
    g = trk.get_refreshed()
    # the host arrays of the same lists
    kd = [np.concatenate([d2[f, :nmin] for f in range(B)] + [d1[0, :nmin]]).reshape(B + 1, nmin, 32),
          np.concatenate([k2[f, :nmin]["octave"] for f in range(B)] + [k1[0, :nmin]["octave"]]).reshape(B + 1, nmin)]
    cen = np.stack([RR.centre_of(T) for T in T2] + [RR.centre_of(T1)])
    fi = np.where(fr < 0, B, fr)
    hd, hc, ho = np.ascontiguousarray(kd[0][fi, kp]), np.ascontiguousarray(cen[fi]), np.ascontiguousarray(kd[1][fi, kp].astype(np.int32))
    X = np.ascontiguousarray(pts["Xw"], np.float64)
    sf = np.cumprod(np.r_[np.float32(1), np.full(7, np.float32(1.2))]).astype(np.float32)
    so = os.path.join(tempfile.mkdtemp(), "librefresh_host.so")
    subprocess.check_call(["g++", "-O2", "-ffp-contract=off", "-shared", "-fPIC", os.path.join(ROOT, "tools", "refresh_host.cc"), "-o", so])
    host = C.CDLL(so).refresh_host
    out = capi._refresh_outputs(P)
    args = [P] + [capi._p(x) for x in (off, hd, hc, ho, kb, ref_obs)] + [None, capi._p(X), capi._p(sf), 8] + [capi._p(out[k]) for k in capi._REFRESH_FIELDS]
    host.argtypes = [C.c_int] + [C.c_void_p] * 9 + [C.c_int] + [C.c_void_p] * 7
    ms_host = timed(lambda: host(*args), lambda: None)
    assert RR.same_outputs(out, g) == [], "the C++ loop and the device disagree"
    m = min(a.numpy_points, P)
    pairs = (counts.astype(np.float64) ** 2)
    t0 = time.perf_counter()
    RR.refresh_points(off[:m + 1], hd, hc, ho, ref_obs[:m], X[:m], sf, obs_kf_bad=kb)
    ms_numpy = 1e3 * (time.perf_counter() - t0) * pairs.sum() / pairs[:m].sum()
    row = dict(pts, desc=g["desc"], normal=g["normal"], mf_max_dist=g["max_dist"], max_dist=np.float32(1.2) * g["max_dist"],
               min_dist=np.float32(0.8) * g["min_dist"])
    ms_upload = timed(lambda: trk.set_local(0, [row]), lambda: None)         # sd_track_set_local waits for its copies
    res = dict(bench="refresh", points=P, keyframes=B, observations=int(counts.sum()), points_over_200=int((counts > 200).sum()),
               distribution="90% 1+geom(0.2)<=60, 8% U[60,200], 2% U[240,256]; 10% bad keyframes",
               ms_b_fuse_setobs_refresh_get=ms_b, ms_b_with_csr_prebuilt=ms_b_prepared, ms_fuse_and_get_fuse=ms_fuse,
               ms_a_host_cpp_O2=ms_host, ms_a_upload_set_local=ms_upload, ms_a_host_numpy_extrapolated=round(float(ms_numpy), 1),
               numpy_points_timed=m,
               ms_a_total_cpp=round(ms_fuse["mean"] + ms_host["mean"] + ms_upload["mean"], 4),
               method="20 warm-up calls, batches of 20 synchronised calls for >= 1 s, host wall clock; mean, min, max over batches",
               lib=os.path.basename(sd.lib_path()))
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
