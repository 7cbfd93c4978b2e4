"""Time sd_track_cull_keyframes, sd_track_erase_observations and the chain local_ba -> erase -> refresh beside the host round
trip it replaces, on the problem of tools/bench_local_ba.py: 20 local + 10 fixed keyframes, 2000 points, 10060 observations,
resident (planted keyframes).

    python tools/bench_cull.py [--out profiles/cull_bench.jsonl]

cull: the call on 29 candidates (monocular, so every point counts) and the synchronising getter of info8 alone.
erase: upload + cull + erase(CULL) + the wait, less upload + cull + the wait (an erase consumes its lists, so each repeat uploads):
ms_erase is that difference of two medians, not a timing of the call alone.
chain: upload, local_ba(write_back = 0), erase(LOCAL_BA), refresh_points, one wait at the end.  round trip: upload, local_ba,
sd_track_get_local_ba (a wait), the erasure and the new CSR arrays in numpy (vectorised: no Python loop over points), upload,
refresh_points, the wait.  Both start from the same upload and end in the same refresh results (asserted).
Method: 5 untimed repeats, then batches of 5 until 1 s has passed; host wall clock, median of the batches.  Appends one JSON line."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def median_ms(step):
    for _ in range(5):
        step()
    batches, t = [], 0.0
    while t < 1.0:
        t0 = time.perf_counter()
        for _ in range(5):
            step()
        batches.append((time.perf_counter() - t0) / 5)
        t += batches[-1] * 5
    return 1e3 * float(np.median(batches))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cull_bench.jsonl"))
    a = ap.parse_args()
    import sdslam_amd as sd
    from sdslam_amd import capi
    from sdslam_amd.capi import _p, _check
    import ba_cases
    B, W, H, P = 29, 640, 480, 2000
    roles = [1] * 19 + [0] * 10 + [1]                      # the last camera is the current keyframe
    p = ba_cases.scene(77, roles, P, lambda r: int(r.integers(4, 7)), stereo_share=0.4, pix_noise=0.5, pose_noise=0.004, point_noise=0.02,
                       wrong_share=0.05)
    p["inv_sigma2"][:] = 1.0
    cfg = (1000, 1.2, 8, 20)
    cur, ref = sd.ORBextractor(*cfg, W, H, 1), sd.ORBextractor(*cfg, W, H, B)
    img = np.random.default_rng(5).integers(0, 256, (B, H, W)).astype(np.uint8)
    cur.extract_batch(img[:1])
    ref.extract_batch(img)
    trk = sd.Tracker(cur, ref, max_points=P, max_batch=B, pnp_max_iterations=8)
    E = len(p["kf"])
    kp_of, kps, descs = np.zeros(E, np.int64), [], []
    ur = -np.ones((B + 1, trk.cap), np.float32)
    rng = np.random.default_rng(9)
    for c in range(B + 1):
        e = np.flatnonzero(p["kf"] == c)
        assert len(e) <= trk.cap
        kp_of[e] = np.arange(len(e))
        k = np.zeros(len(e), capi.KP_DTYPE)
        k["x"], k["y"], k["size"] = p["uv"][e, 0], p["uv"][e, 1], 31.0
        kps.append(k)
        descs.append(rng.integers(0, 256, (len(e), 32)).astype(np.uint8))
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
    trk.set_ba_keyframes(p["roles"][:B], 1)
    L, h = trk.L, trk.h
    off = p["off"].astype(np.int32)
    frame = np.where(p["kf"] < B, p["kf"], -1).astype(np.int32)
    kp = kp_of.astype(np.int32)
    kb, ro, pb = np.zeros(E, np.uint8), np.zeros(P, np.int32), np.zeros(P, np.uint8)
    weight = np.where(p["ur"] >= 0, 2, 1)
    point_of = np.repeat(np.arange(P), np.diff(off))
    trk._n_refresh, trk._n_refresh_obs = P, E

    def upload(off_, fr_, kp_, kb_, ro_, pb_):
        _check(L.sd_track_set_observations(h, P, _p(off_), _p(fr_), _p(kp_), _p(kb_), _p(ro_), _p(pb_)))

    first = lambda: upload(off, frame, kp, kb, ro, pb)
    cand, flags = np.arange(B, dtype=np.int32), np.zeros(B, np.uint8)
    info8 = np.zeros(8, np.int32)

    def wait_cull():
        _check(L.sd_track_get_culled(h, None, None, None, None, None, None, _p(info8), 0, 0, 0))

    first()
    ms_cull = median_ms(lambda: (trk.cull_keyframes(cand, flags, 1, 40.0), wait_cull()))
    culled = trk.get_culled()
    ms_upload_cull = median_ms(lambda: (first(), trk.cull_keyframes(cand, flags, 1, 40.0), wait_cull()))

    def wait_erased():
        _check(L.sd_track_get_erased(h, None, None, None, None, None, _p(info8), 0, 0))

    ms_upload_cull_erase = median_ms(lambda: (first(), trk.cull_keyframes(cand, flags, 1, 40.0), trk.erase_observations(capi.ERASE_CULL), wait_erased()))
    erased_by_cull = info8.copy()

    def chain():
        first()
        trk.local_ba(0, write_back=False)
        trk.erase_observations(capi.ERASE_LOCAL_BA)
        trk.refresh_points(0, write_local=False)
        return trk.get_refreshed()

    obs_erase, info16 = np.zeros(E, np.uint8), np.zeros(16, np.int32)

    def round_trip():
        first()
        trk.local_ba(0, write_back=False)
        _check(L.sd_track_get_local_ba(h, None, None, None, None, _p(obs_erase), _p(info16), P, E))
        kill = obs_erase != 0
        n_obs = np.bincount(point_of, weights=np.where(kill, 0, weight), minlength=P)
        bad = (np.bincount(point_of, weights=kill, minlength=P) > 0) & (n_obs <= 2)
        keep = ~kill & ~bad[point_of]
        new_off = np.concatenate([[0], np.cumsum(np.bincount(point_of, weights=keep, minlength=P))]).astype(np.int32)
        ref_dead = ~keep[off[:-1] + ro] if E else np.zeros(P, bool)
        before_ref = np.cumsum(keep) - keep                                 # survivors in front of each entry
        new_ro = np.where(ref_dead | (new_off[1:] == new_off[:-1]), 0, before_ref[off[:-1] + ro] - new_off[:-1]).astype(np.int32)
        upload(new_off, np.ascontiguousarray(frame[keep]), np.ascontiguousarray(kp[keep]), np.ascontiguousarray(kb[keep]), new_ro,
               (pb | bad).astype(np.uint8))
        trk.refresh_points(0, write_local=False)
        return trk.get_refreshed()

    a_, b_ = chain(), round_trip()
    assert info16[0] == 0 and info16[13] > 0, info16
    for k in a_:
        assert a_[k].tobytes() == b_[k].tobytes(), k
    ms_chain, ms_round_trip = median_ms(chain), median_ms(round_trip)
    first()
    ms_upload_ba = median_ms(lambda: (first(), trk.local_ba(0, write_back=False), trk.get_local_ba()))
    res = dict(bench="cull", keyframes=B + 1, candidates=B, points=P, observations=E, cull_info8=culled["info8"].tolist(),
               erase_cull_info8=erased_by_cull.tolist(), ba_erased=int(info16[13]), ms_cull=round(ms_cull, 4),
               ms_upload_cull=round(ms_upload_cull, 4), ms_upload_cull_erase=round(ms_upload_cull_erase, 4),
               ms_erase=round(ms_upload_cull_erase - ms_upload_cull, 4), ms_upload_local_ba_get=round(ms_upload_ba, 4),
               ms_chain_ba_erase_refresh=round(ms_chain, 4), ms_round_trip_ba_host_erase_upload_refresh=round(ms_round_trip, 4))
    print(json.dumps(res))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
