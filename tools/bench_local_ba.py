"""Time sd_track_local_ba on one problem: 20 local + 10 fixed keyframes, 2000 points, about 5 observations each, resident (planted
keyframes, as tests/test_local_ba_gpu.py plants them), write_back = 0 so that every call solves the same problem.

    python tools/bench_local_ba.py [--out profiles/local_ba_bench.jsonl]

The host queues the worst-case schedule (15 iterations of one linearisation and ten trials); the kernels of steps the state record
does not ask for return at once.  What those launches cost is measured on the same lists with one observation of a keyframe that
is not resident: the device refuses the problem in its second kernel and EVERY later launch of the schedule is a skipped one.
ms_per_skipped_launch = that call / its launches; skipped_share = the launches the real run skipped (the schedule less
4 per iteration and 5 per trial that ran, read off info16) times that, over ms_call.  The reduced solve (k_ba_schur + k_ba_solve) is device time and is read off a kernel trace of this script
(profiles/local_ba_kernel_trace.txt), not off the host clock.
Method: 5 untimed calls, then batches of 5 calls each ended by the synchronising getter until 1 s has passed; host wall clock,
median of the batches.  Appends one JSON line to --out."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "local_ba_bench.jsonl"))
    a = ap.parse_args()
    import sdslam_amd as sd
    from sdslam_amd import capi
    import ba_cases
    B, W, H, P = 29, 640, 480, 2000
    roles = [1] * 19 + [0] * 10 + [1]                      # the last camera is the current keyframe
    p = ba_cases.scene(77, roles, P, lambda r: int(r.integers(4, 7)), stereo_share=0.4, pix_noise=0.5, pose_noise=0.004, point_noise=0.02,
                       wrong_share=0.05)
    p["inv_sigma2"][:] = 1.0                               # octave 0 everywhere: the same float on the device
    cfg = (1000, 1.2, 8, 20)
    cur, ref = sd.ORBextractor(*cfg, W, H, 1), sd.ORBextractor(*cfg, W, H, B)
    img = np.random.default_rng(5).integers(0, 256, (B, H, W)).astype(np.uint8)
    cur.extract_batch(img[:1])
    ref.extract_batch(img)
    trk = sd.Tracker(cur, ref, max_points=P, max_batch=B, pnp_max_iterations=8)
    E = len(p["kf"])
    kp_of, kps, descs = np.zeros(E, np.int64), [], []
    ur = -np.ones((B + 1, trk.cap), np.float32)
    for c in range(B + 1):
        e = np.flatnonzero(p["kf"] == c)
        assert len(e) <= trk.cap
        kp_of[e] = np.arange(len(e))
        k = np.zeros(len(e), capi.KP_DTYPE)
        k["x"], k["y"], k["size"] = p["uv"][e, 0], p["uv"][e, 1], 31.0
        kps.append(k)
        descs.append(np.zeros((len(e), 32), np.uint8))
        ur[c, :len(e)] = p["ur"][e]
    ref.set_keypoints(0, kps[:B], descs[:B])
    cur.set_keypoints(0, kps[B:], descs[B:])
    trk.set_camera(*p["cam"], p["bf"], (0.0, float(W), 0.0, float(H)))
    trk.set_uright_ref(0, ur[:B])
    trk.set_uright(0, ur[B:])
    trk.set_poses(0, list(p["poses"][:B]), [p["poses"][B]] * B)
    row = dict(cand=np.ones(P, np.uint8), Xw=p["Xw"], normal=np.zeros((P, 3)), min_dist=np.zeros(P, np.float32), max_dist=np.zeros(P, np.float32),
               mf_max_dist=np.zeros(P, np.float32), desc=np.zeros((P, 32), np.uint8), obs=np.ones(P, np.int32))
    trk.set_local(0, [row])
    obs = [[(int(p["kf"][e]) if p["kf"][e] < B else -1, int(kp_of[e]), 0) for e in range(p["off"][i], p["off"][i + 1])] for i in range(P)]
    trk.set_ba_keyframes(p["roles"][:B], 1)

    def timed():
        call = lambda: trk.local_ba(0, write_back=False)
        for _ in range(5):
            call()
        trk.get_local_ba()
        batches, t = [], 0.0
        while t < 1.0:
            t0 = time.perf_counter()
            for _ in range(5):
                call()
                trk.get_local_ba()
            batches.append((time.perf_counter() - t0) / 5)
            t += batches[-1] * 5
        return 1e3 * float(np.median(batches))

    trk.set_observations(obs, np.zeros(P, np.int32))
    ms_call = timed()
    info = trk.get_local_ba()["info16"]
    want = capi.debug_local_ba(p)["info16"]
    assert info.tolist() == want.tolist() and info[0] == 0, (info, want)
    refused = [o + [(-2, 0, 0)] if i == 0 else o for i, o in enumerate(obs)]
    trk.set_observations(refused, np.zeros(P, np.int32))
    ms_refused = timed()
    assert trk.get_local_ba()["info16"][0] == 1
    n_free = int((p["roles"] == 1).sum())
    launches = 2 + 1 + 2 * (1 + 1) + 15 * (4 + 10 * 5) + 1
    ran = 4 * int(info[6] + info[9]) + 5 * int(info[7] + info[10])
    per = ms_refused / launches
    res = dict(bench="local_ba", keyframes_free=n_free, keyframes_fixed=int(info[2]), points=P, observations=E, info16=info.tolist(),
               ms_call=round(ms_call, 4), ms_refused_call_all_launches_skipped=round(ms_refused, 4), launches=launches, launches_that_ran=ran + 9,
               us_per_skipped_launch=round(1e3 * per, 3), skipped_share=round(per * (launches - ran - 9) / ms_call, 4))
    print(json.dumps(res))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
