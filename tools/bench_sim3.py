"""Time the device Sim3Solver (k_sim3): B candidate slots, N correspondences at 40 % outliers.

    python tools/bench_sim3.py [--slots 1024] [--n 300] [--host-slots 16]

Prints one JSON line: ms per iterate(5) call and per find() call on the tracking stream (>= 20 warm-up calls, timed region
>= 1 s, host clock around a queue of calls closed by one synchronising getter), and for context the same solves through
tests/sim3_ref.py on this host (extrapolated from --host-slots) and the bytes a caller no longer downloads per call
(matches12 and the two flag rows).  For the kernel's share run it once under `rocprofv3 --kernel-trace --stats -- python
tools/bench_sim3.py` (a run of its own, no counters)."""
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
    ap.add_argument("--slots", type=int, default=1024)
    ap.add_argument("--n", type=int, default=300)
    ap.add_argument("--host-slots", type=int, default=16)
    a = ap.parse_args()
    import sdslam_amd as sd
    import sim3_cases as SC
    import sim3_ref as R3
    from sdslam_amd import synth
    B, N, W, H, NF = a.slots, a.n, 640, 480, 1000
    cfg = (NF, 1.2, 8, 20)
    cur, ref = sd.ORBextractor(*cfg, W, H, B), sd.ORBextractor(*cfg, W, H, B)
    img = np.stack([synth.make_image(i, W, H) for i in range(8)])
    imgs = img[np.arange(B) % 8]
    k1, _, n1 = cur.extract_batch(imgs)
    k2, _, n2 = ref.extract_batch(imgs[::-1].copy())
    trk = sd.Tracker(cur, ref, max_points=NF, max_batch=B, pnp_max_iterations=300)
    trk.set_camera(*SC.K, 0.0, (0.0, float(W), 0.0, float(H)))
    rng = np.random.default_rng(3)
    slots = []
    for b in range(B):
        sl = SC.make_slot(rng, "n70_out30", k1["octave"][b], n1[b], k2["octave"][b], n2[b], cap=NF, n_override=N, out_override=0.4)
        slots.append(sl)
    rand = rng.integers(0, 2 ** 31, size=(B, 900), dtype=np.int64).astype(np.int32)
    SC.upload(trk, slots, rand)

    def timed(call):
        for _ in range(20):
            call()
        trk.get_sim3(0, 1)
        reps, t = 0, 0.0
        while t < 1.0:
            t0 = time.perf_counter()
            for _ in range(20):
                call()
            trk.get_sim3(0, 1)
            t += time.perf_counter() - t0
            reps += 20
        return 1e3 * t / reps

    ms_it5 = timed(lambda: trk.sim3(B, 0, 0.99, 20, 300, 5))
    ms_find = timed(lambda: trk.sim3(B, 0, 0.99, 20, 300, 300))
    g = trk.get_sim3(0, B)
    hs = min(a.host_slots, B)
    t0 = time.perf_counter()
    for b in range(hs):
        s = R3.Sim3Solver(slots[b]["kf1"], slots[b]["kf2"], slots[b]["matches12"], False, SC.K, R3.level_sigma2(1.2, 8), rand[b])
        s.set_ransac_parameters(0.99, 20, 300)
        s.find()
    host_ms = 1e3 * (time.perf_counter() - t0) * B / hs
    print(json.dumps(dict(bench="sim3", slots=B, N=N, outliers=0.4, ms_iterate5=round(ms_it5, 4), ms_find=round(ms_find, 4),
                          returned=int(g["returned"].sum()), mean_iterations=float(g["iterations"].mean()),
                          host_restatement_ms_find=round(host_ms, 1), bytes_not_downloaded_per_call=int(B * NF * (4 + 1 + 1)))))


if __name__ == "__main__":
    main()
