"""Time the device Fuse search (k_fuse) next to sd_track_match_local (k_match_local, the nearest existing kernel) on the same
keyframes, points and slots in the same session.

    python tools/bench_fuse.py [--keyframes 30] [--out profiles/NAME.json]

Two shapes at VGA, ~1000 keypoints and 1000 points: --keyframes target keyframes against one shared point row (kf_side 1: the
first loop of SearchInNeighbors) and --keyframes x 1000 candidates against one broadcast keyframe (kf_side 0: its second
Fuse).  Per shape: ms per call from HIP events on the tracking stream (sd_track_set_profiling is not used: the events are the
library's stream fence around a queue of calls; >= 20 warm-up calls, timed region >= 1 s) for sd_track_match_local, for
sd_track_fuse, and for sd_track_match_local again (the yardstick's run-to-run spread).  Slot 0 of every shape is checked against
the numpy restatement of tests/fuse_ref.py.  Prints one JSON line.  SD_LIB runs another build of the library (e.g. one built
with SD_EXTRA_FLAGS=-DFUSE_GL=4 SD_OUT=...: lanes per point side by side)."""
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
    ap.add_argument("--keyframes", type=int, default=30)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    import sdslam_amd as sd
    import fuse_cases as FC
    import fuse_ref as FR
    from sdslam_amd import synth
    W, H, NF, B = 640, 480, 1000, a.keyframes
    K = (synth.FX, synth.FY, synth.CX, synth.CY)
    cam9 = np.array([*K, 40.0, 0, W, 0, H], np.float32)
    cfg = (NF, 1.2, 8, 20)
    cur, ref = sd.ORBextractor(*cfg, W, H, B), sd.ORBextractor(*cfg, W, H, B)
    tex = synth.make_image(31, 2 * W, 2 * H)
    rng = np.random.default_rng(5)
    T_kf = [synth.se3_exp(rng.uniform(-0.06, 0.06, 3), rng.uniform(-0.5, 0.5, 3)) for _ in range(8)]
    views = np.stack([synth.render_plane_view(tex, T, W, H) for T in T_kf])
    sel = np.arange(B) % 8
    k1, d1, n1 = cur.extract_batch(views[sel])
    k2, d2, n2 = ref.extract_batch(views[sel])
    n0 = min(int(n1[0]), 900)
    rows = [synth.local_map_case(100 + int(s), k1[0, :n0], d1[0, :n0], T_kf[0], n_extra=NF - n0) for s in range(B)]
    trk = sd.Tracker(cur, ref, max_points=NF, max_batch=B, pnp_max_iterations=8)
    trk.set_camera(*K, 40.0, (0.0, float(W), 0.0, float(H)))
    trk.set_local(0, rows)
    stream = torch.cuda.Stream()

    def timed(call, sync):
        """ms per call: events on a side stream fenced against the tracking stream, so only device time between them counts."""
        def burst(n):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            sd.lib().sd_track_stream_fence(trk.h, stream.cuda_stream, 0)
            e0.record(stream)
            sd.lib().sd_track_stream_fence(trk.h, stream.cuda_stream, 1)
            for _ in range(n):
                call()
            sd.lib().sd_track_stream_fence(trk.h, stream.cuda_stream, 0)
            e1.record(stream)
            sync()
            e1.synchronize()
            return e0.elapsed_time(e1)
        burst(20)
        reps, ms, t0 = 0, 0.0, time.perf_counter()
        while time.perf_counter() - t0 < 1.0:
            ms += burst(20)
            reps += 20
        return ms / reps

    out = dict(bench="fuse", keypoints=float(n2.mean()), points=float(np.mean([len(r["cand"]) for r in rows])),
               lib=os.path.basename(sd.lib_path()))
    for name, side, bc in (("neighbours_%d" % B, 1, -1), ("candidates_%dx%d" % (B, NF), 0, 0)):
        trk.set_current_broadcast(-1)
        trk.set_poses(0, [T_kf[i] for i in sel], [T_kf[0] if bc >= 0 else T_kf[i] for i in sel])
        trk.set_current_broadcast(bc)
        prow = 0 if side else -1
        loc = lambda: trk.match_local(B, 3.0, 0.8, 0.5)
        fus = lambda: trk.fuse(B, side, prow, 3.0, False)
        ms_loc = timed(loc, lambda: trk.get_local(0, 1))
        ms_fus = timed(fus, lambda: trk.get_fuse(0, 1))
        ms_loc2 = timed(loc, lambda: trk.get_local(0, 1))
        g = trk.get_fuse(0, B)
        kk, dd, nn = (k2, d2, n2) if side else (k1, d1, n1)
        m = int(nn[0])
        bi, bd = FR.fuse_search(kk[0, :m], dd[0, :m], np.full(m, -1, np.float32), rows[0], T_kf[0], cam9, FC.SF, FC.INV_SIGMA2, FC.SCALE, 3.0)
        assert np.array_equal(bi, g["best_idx"][0, :len(bi)]) and np.array_equal(bd, g["best_dist"][0, :len(bd)])
        out[name] = dict(slots=B, ms_match_local=round(ms_loc, 4), ms_fuse=round(ms_fus, 4), ms_match_local_again=round(ms_loc2, 4),
                         ratio_to_match_local=round(ms_fus / (0.5 * (ms_loc + ms_loc2)), 3),
                         yardstick_spread=round(abs(ms_loc - ms_loc2) / min(ms_loc, ms_loc2), 4), mean_fused=float(g["n_found"].mean()))
    trk.set_current_broadcast(-1)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
