"""Time LocalMapping::CreateNewMapPoints for one keyframe of 1000 keypoints against 20 neighbours, two ways, and then the chain
into SearchInNeighbors' first Fuse loop, two ways:

  (a) the path before sd_track_triangulate: the device search, sd_track_get_triangulation_matches for all neighbours, the
      triangulation on the host, and the upload of the new points through sd_track_set_local (one row, as Fuse reads it);
  (b) the device search and sd_track_triangulate queued back to back, ended by sd_track_get_new_points (which the caller's
      MapPoint objects need in either path);
  (c) the chain search -> triangulate -> sd_track_append_new_points -> sd_track_fuse(kf_side 1, point_row 0), queued back to back
      and ended by sd_track_get_fuse, against
  (d) the same chain with the round trip the append replaces: search -> triangulate -> sd_track_get_new_points -> the rows and
      cand flags built on the host (numpy) -> sd_track_set_local -> sd_track_fuse -> sd_track_get_fuse.
      Both in the same run, one after the other; their Fuse results must be equal.

    python tools/bench_new_points.py [--neighbours 20] [--host-slots 2] [--out profiles/new_points_bench.jsonl]

The host triangulation of (a) is the numpy restatement tests/new_points_ref.py -- scalar Python, the only host implementation
in this repository, far slower than the reference's C++ -- timed on --host-slots neighbours and extrapolated to all of them; its
verdicts on those neighbours must equal the device's.  It is reported separately (ms_host_triangulation_numpy), so that
ms_a_without_host_triangulation = search + download + upload is a LOWER bound of path (a) for any host implementation.
Method: 20 untimed calls, then batches of 20 calls each ended by its synchronising getter until 1 s has passed; host wall clock.
Appends one JSON line to --out."""
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
    ap.add_argument("--neighbours", type=int, default=20)
    ap.add_argument("--host-slots", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "new_points_bench.jsonl"))
    a = ap.parse_args()
    import sdslam_amd as sd
    import new_points_ref as NR
    import triangulation_ref as TR
    from sdslam_amd import synth
    W, H, NF, B = 640, 480, 1000, a.neighbours
    K = (synth.FX, synth.FY, synth.CX, synth.CY)
    cfg = (NF, 1.2, 8, 20)
    cur, ref = sd.ORBextractor(*cfg, W, H, 1), sd.ORBextractor(*cfg, W, H, B)
    tex = synth.make_image(31, 2 * W, 2 * H)
    rng = np.random.default_rng(5)
    T1 = synth.se3_exp((0.01, 0.0, 0.0), (0.1, -0.2, 0.1))
    T2 = [synth.se3_exp((0.2, 0.03, 0.03) * rng.uniform(-1.5, 1.5, 3), rng.uniform(-0.5, 0.5, 3)) @ T1 for _ in range(B)]
    k1, d1, n1 = cur.extract_batch(np.stack([synth.render_plane_view(tex, T1, W, H)]))
    k2, d2, n2 = ref.extract_batch(np.stack([synth.render_plane_view(tex, T, W, H) for T in T2]))
    cap = k1.shape[1]
    trk = sd.Tracker(cur, ref, max_points=max(NF, cap), max_batch=B, pnp_max_iterations=8)
    trk.set_camera(*K, 0.0, (0.0, float(W), 0.0, float(H)))
    trk.set_poses(0, T2, [T1] * B)
    none = np.zeros((B, cap), np.uint8)
    trk.set_point_flags(0, none, none)
    trk.set_tri_median_depth(0, np.full(B, 2.0, np.float32))
    trk.set_next_map_id(0, [0])
    trk.set_current_broadcast(0)

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

    search = lambda: trk.search_for_triangulation(B, False, False)

    def device():
        search()
        trk.triangulate(B, True)
    ms_b = timed(device, trk.get_new_points)
    ms_search_download = timed(search, lambda: trk.get_triangulation_matches(0, B))
    device()                                                             # the search alone ended the triangulation's result
    g, t, pts = trk.get_triangulation_matches(0, B), trk.get_triangulated(0, B), trk.get_new_points()
    n_pts = int(pts["info"][0])
    mono = np.full(cap, -1, np.float32)
    cam5 = np.array([*K, 0.0], np.float32)
    sf, sigma2 = TR.scale_tables(1.2, 8)
    hs = min(a.host_slots, B)
    m1 = int(n1[0])
    t0 = time.perf_counter()
    for b in range(hs):
        m2 = int(n2[b])
        v, _, _ = NR.triangulate(k1[0, :m1], k1[0, :m1], mono[:m1], mono[:m1], k2[b, :m2], k2[b, :m2], mono[:m2], mono[:m2],
                                 g["matches12"][b, :m1], T1, T2[b], cam5, sf, sigma2, 1.2, True, 2.0)
        assert np.array_equal(v, t["verdict"][b, :m1]), b
    ms_host = 1e3 * (time.perf_counter() - t0) * B / max(hs, 1)
    row = dict(cand=np.ones(n_pts, np.uint8), Xw=pts["Xw"], normal=pts["normal"], min_dist=0.8 * pts["min_dist"],
               max_dist=1.2 * pts["max_dist"], mf_max_dist=pts["max_dist"], desc=pts["desc"], obs=np.full(n_pts, 2, np.int32))
    row = {k: v[:trk.M] for k, v in row.items()}
    ms_upload = timed(lambda: trk.set_local(0, [row]), lambda: None)     # sd_track_set_local waits for its copies
    # (c) / (d): the chain into Fuse.  Row 0 starts empty each time (the n_local upload of an empty row); cand of all B rows.
    M = trk.M
    zero = dict(cand=np.zeros(0, np.uint8), Xw=np.zeros((0, 3)), normal=np.zeros((0, 3)), min_dist=np.zeros(0, np.float32),
                max_dist=np.zeros(0, np.float32), mf_max_dist=np.zeros(0, np.float32), desc=np.zeros((0, 32), np.uint8),
                obs=np.zeros(0, np.int32))

    def chain_device():
        trk.set_local(0, [zero])
        device()
        trk.append_new_points(0, B, False)
        trk.fuse(B, kf_side=1, point_row=0, th=3.0)

    def chain_host():
        device()
        p = trk.get_new_points()
        n = min(int(p["info"][0]), M)
        cand = np.ones((B, n), np.uint8)
        cand[p["slot"][:n], np.arange(n)] = 0
        shared = dict(Xw=p["Xw"][:n], normal=p["normal"][:n], min_dist=np.float32(0.8) * p["min_dist"][:n],
                      max_dist=np.float32(1.2) * p["max_dist"][:n], mf_max_dist=p["max_dist"][:n], desc=p["desc"][:n],
                      obs=np.full(n, 2, np.int32))
        trk.set_local(0, [dict(shared, cand=cand[f]) for f in range(B)])
        trk.fuse(B, kf_side=1, point_row=0, th=3.0)
    get_fuse = lambda: trk.get_fuse(0, B)
    ms_c = timed(chain_device, get_fuse)
    fuse_c = get_fuse()
    ms_d = timed(chain_host, get_fuse)
    fuse_d = get_fuse()
    n_app = min(n_pts, M)
    for k in ("best_idx", "best_dist", "n_found"):
        assert np.array_equal(fuse_c[k][..., :n_app] if fuse_c[k].ndim == 2 else fuse_c[k], fuse_d[k][..., :n_app] if fuse_d[k].ndim == 2 else fuse_d[k]), k
    trk.set_current_broadcast(-1)
    lower = ms_search_download + ms_upload
    out = dict(bench="new_points", keypoints=int(n1[0]), neighbours=B, matches=int((g["matches12"] >= 0).sum()), new_points=n_pts,
               ms_b_search_triangulate_get_new_points=round(ms_b, 4), ms_a_search_and_download=round(ms_search_download, 4),
               ms_a_upload_set_local=round(ms_upload, 4), ms_a_without_host_triangulation=round(lower, 4),
               ms_host_triangulation_numpy=round(ms_host, 1), host_slots_timed=hs, ms_a_with_numpy=round(lower + ms_host, 1),
               ratio_b_to_a_lower_bound=round(ms_b / lower, 3), ms_c_chain_append_fuse_get_fuse=round(ms_c, 4),
               ms_d_chain_get_new_points_set_local_fuse_get_fuse=round(ms_d, 4), ratio_c_to_d=round(ms_c / ms_d, 3),
               fused_found=int(fuse_c["n_found"].sum()), host_triangulation="numpy restatement (tests/new_points_ref.py), extrapolated",
               method="20 warm-up calls, batches of 20 synchronised calls for >= 1 s, host wall clock", lib=os.path.basename(sd.lib_path()))
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
