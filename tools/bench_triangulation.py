"""Time the device SearchForTriangulation (k_tri_geometry + k_search_triangulation) next to sd_track_search_by_points on the
same keyframes, flags and slots in the same session.

    python tools/bench_triangulation.py [--pairs 1024] [--neighbours 20] [--host-pairs 2] [--out profiles/NAME.json]

Two shapes: one current keyframe against --neighbours keyframes (the broadcast; CreateNewMapPoints' loop) and --pairs
independent pairs, ~1000 keypoints each, half of them flagged.  Per shape: ms per call on the tracking stream (>= 20 warm-up
calls, timed region >= 1 s, host clock around a queue of calls closed by one synchronising getter) for SearchByPoints, for
SearchForTriangulation, and for SearchByPoints again (the yardstick's run-to-run spread), their ratio, and the single-threaded
numpy restatement of tests/triangulation_ref.py extrapolated from --host-pairs pairs (the device's result on those pairs must
equal it).  Prints one JSON line.  SD_LIB runs another build of the library (kernel variants side by side)."""
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
    ap.add_argument("--pairs", type=int, default=1024)
    ap.add_argument("--neighbours", type=int, default=20)
    ap.add_argument("--host-pairs", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import sdslam_amd as sd
    import triangulation_ref as TR
    from sdslam_amd import synth
    W, H, NF = 640, 480, 1000
    K = (synth.FX, synth.FY, synth.CX, synth.CY)
    B = max(a.pairs, a.neighbours)
    cfg = (NF, 1.2, 8, 20)
    cur, ref = sd.ORBextractor(*cfg, W, H, B), sd.ORBextractor(*cfg, W, H, B)
    # eight view pairs of the textured surface, repeated over the slots: real epipolar geometry, real descriptors
    tex = synth.make_image(31, 2 * W, 2 * H)
    rng = np.random.default_rng(5)
    T_ref = [synth.se3_exp(rng.uniform(-0.05, 0.05, 3), rng.uniform(-0.4, 0.4, 3)) for _ in range(8)]
    T_cur = [synth.se3_exp((0.15, 0.02, 0.02) * rng.uniform(0.5, 1.5, 3), rng.uniform(-0.5, 0.5, 3)) @ T for T in T_ref]
    view_cur = np.stack([synth.render_plane_view(tex, T, W, H) for T in T_cur])
    view_ref = np.stack([synth.render_plane_view(tex, T, W, H) for T in T_ref])
    sel = np.arange(B) % 8
    k1, d1, n1 = cur.extract_batch(view_cur[sel])
    k2, d2, n2 = ref.extract_batch(view_ref[sel])
    cap = k1.shape[1]
    trk = sd.Tracker(cur, ref, max_points=NF, max_batch=B, pnp_max_iterations=8)
    trk.set_camera(*K, 0.0, (0.0, float(W), 0.0, float(H)))
    trk.set_poses(0, [T_ref[i] for i in sel], [T_cur[i] for i in sel])
    h1, h2 = (rng.random((B, cap)) < 0.5).astype(np.uint8), (rng.random((B, cap)) < 0.5).astype(np.uint8)
    trk.set_point_flags(0, h1, h2)

    def timed(call, sync):
        for _ in range(20):
            call()
        sync()
        reps, t = 0, 0.0
        while t < 1.0:
            t0 = time.perf_counter()
            for _ in range(20):
                call()
            sync()
            t += time.perf_counter() - t0
            reps += 20
        return 1e3 * t / reps

    out = dict(bench="triangulation", keypoints=float(n1.mean()), flagged=0.5, lib=os.path.basename(sd.lib_path()))
    for name, n, bc in (("broadcast_%d" % a.neighbours, a.neighbours, 0), ("pairs_%d" % a.pairs, a.pairs, -1)):
        trk.set_current_broadcast(bc)
        sbp = lambda: trk.search_by_points(n, 0.75, False)
        tri = lambda: trk.search_for_triangulation(n, False, False)
        ms_sbp = timed(sbp, lambda: trk.get_point_matches(0, 1))
        ms_tri = timed(tri, lambda: trk.get_triangulation_matches(0, 1))
        ms_sbp2 = timed(sbp, lambda: trk.get_point_matches(0, 1))
        g = trk.get_triangulation_matches(0, n)
        hp = min(a.host_pairs, n)
        t0 = time.perf_counter()
        for b in range(hp):
            f1 = 0 if bc >= 0 else b
            m1, m2 = int(n1[f1]), int(n2[b])
            u = np.full(cap, -1, np.float32)
            nh, mh = TR.search_for_triangulation(k1[f1, :m1], d1[f1, :m1], h1[b, :m1], u[:m1], k2[b, :m2], d2[b, :m2], h2[b, :m2], u[:m2],
                                                 g["F12"][b], g["epipole"][b], *TR.scale_tables(1.2, 8), False)
            assert nh == g["n_matches"][b] and np.array_equal(mh, g["matches12"][b, :m1])
        host_ms = 1e3 * (time.perf_counter() - t0) * n / max(hp, 1)
        out[name] = dict(slots=n, ms_search_by_points=round(ms_sbp, 4), ms_search_for_triangulation=round(ms_tri, 4),
                         ms_search_by_points_again=round(ms_sbp2, 4), ratio_to_search_by_points=round(ms_tri / (0.5 * (ms_sbp + ms_sbp2)), 3),
                         yardstick_spread=round(abs(ms_sbp - ms_sbp2) / min(ms_sbp, ms_sbp2), 4), mean_matches=float(g["n_matches"].mean()),
                         host_restatement_ms=round(host_ms, 1))
    trk.set_current_broadcast(-1)
    line = json.dumps(out)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
