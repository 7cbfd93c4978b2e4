"""Time sd_track_global_ba on two resident problems (planted keyframes, as tools/bench_local_ba.py plants them), write_back = 0 so that
every call solves the same problem:

    mono_init   2 keyframes, one fixed, 150 monocular points, 20 iterations, robust      (Tracking::CreateInitialMapMonocular)
    loop        128 free keyframes and 2 fixed ones, 2000 points (max_points is at most 2048) seen by 3 .. 6 neighbouring cameras, 10 iterations, not robust
                (LoopClosing::RunGlobalBundleAdjustment); the reduced system has 768 unknowns: the blocked LDL^T, 16 panels

    python tools/bench_global_ba.py [--out profiles/global_ba_bench.jsonl]

Per call: host wall time (5 untimed calls, then batches of 5 calls each ended by the synchronising getter until 1 s has passed;
median of the batches), the launches the host queues and those that did work (read off info16: 4 per iteration, and per trial
schur + solver + 3).  The device time of the solver (k_gba_* or k_ba_solve) and of k_ba_schur comes from a kernel trace taken in a run of
its own: for each shape the tool starts `rocprofv3 --kernel-trace -- python tools/bench_global_ba.py --traced SHAPE`, a child that
makes TRACED_CALLS calls and nothing else, and sums the durations of those kernels per call, the launches that did work apart from the ones that return
at once.  The file is written afresh on every run; nothing is asserted on any number, and there is no g2o here to
compare with."""
import argparse
import csv
import glob
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


TRACED_CALLS = 3
ROCPROF = os.environ.get("ROCPROFV3", "/opt/rocm/bin/rocprofv3")


def traced(name, trials, panels):
    """us per call of the solver kernels and of k_ba_schur from a kernel trace of a child process.  Every launch of the worst-case
    schedule is in the trace; the launches that did work are `trials` (x panels for the blocked solver's kernels) a call, and they
    are taken to be the longest ones of their kernel: a launch that returns at once is shorter than any that works."""
    worked = {"k_gba_diag": trials * panels, "k_gba_panel": trials * panels, "k_gba_trail": trials * (panels - 1), "k_gba_back": trials * panels,
              "k_ba_solve": trials, "k_ba_schur": trials}
    with tempfile.TemporaryDirectory() as d:
        subprocess.run([ROCPROF, "--kernel-trace", "--output-format", "csv", "-d", d, "--", sys.executable, os.path.abspath(__file__),
                        "--traced", name], check=True, stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL, timeout=600)
        ns = {}
        for path in glob.glob(os.path.join(d, "**", "*kernel_trace.csv"), recursive=True):
            for row in csv.DictReader(open(path)):
                key = next((n for n in worked if n in row["Kernel_Name"]), None)
                if key:
                    ns.setdefault(key, []).append(int(row["End_Timestamp"]) - int(row["Start_Timestamp"]))
    out = {}
    for k, v in sorted(ns.items()):
        v.sort(reverse=True)
        w = worked[k] * TRACED_CALLS
        out[k] = dict(launches=len(v) // TRACED_CALLS, worked=worked[k], worked_us=round(sum(v[:w]) / 1e3 / TRACED_CALLS, 2),
                      skipped_us=round(sum(v[w:]) / 1e3 / TRACED_CALLS, 2), skipped_median_us=round(float(np.median(v[w:])) / 1e3, 2) if len(v) > w else 0.0)
    solver = [r for k, r in out.items() if k != "k_ba_schur"]
    return dict(trace_per_call=out, solver_worked_us_per_call=round(sum(r["worked_us"] for r in solver), 2),
                solver_skipped_us_per_call=round(sum(r["skipped_us"] for r in solver), 2),
                schur_worked_us_per_call=out.get("k_ba_schur", {}).get("worked_us", 0.0))


def bench(sd, capi, name, p, n_iterations, robust, W, H, calls=0):
    """p: a problem whose LAST camera becomes the current keyframe.  calls > 0: that many calls and nothing else (the traced child)"""
    B, P, E = len(p["roles"]) - 1, len(p["Xw"]), len(p["kf"])
    p["inv_sigma2"][:] = 1.0                               # octave 0 everywhere: the same float on the device
    cfg = (300, 1.2, 8, 20)
    cur, ref = sd.ORBextractor(*cfg, W, H, 1), sd.ORBextractor(*cfg, W, H, B)
    img = np.random.default_rng(5).integers(0, 256, (B, H, W)).astype(np.uint8)
    cur.extract_batch(img[:1])
    ref.extract_batch(img)
    trk = sd.Tracker(cur, ref, max_points=P, max_batch=B, pnp_max_iterations=8)
    kp_of, kps, descs = np.zeros(E, np.int64), [], []
    ur = -np.ones((B + 1, trk.cap), np.float32)
    for c in range(B + 1):
        e = np.flatnonzero(p["kf"] == c)
        assert len(e) <= trk.cap, (c, len(e), trk.cap)
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
    trk.set_observations(obs, np.zeros(P, np.int32))
    trk.set_ba_keyframes(p["roles"][:B], int(p["roles"][B]))
    call = lambda: trk.global_ba(0, n_iterations, robust, write_back=False)
    if calls:
        for _ in range(calls):
            call()
            trk.get_global_ba()
        return None
    for _ in range(5):
        call()
    trk.get_global_ba()
    batches, t = [], 0.0
    while t < 1.0:
        t0 = time.perf_counter()
        for _ in range(5):
            call()
            trk.get_global_ba()
        batches.append((time.perf_counter() - t0) / 5)
        t += batches[-1] * 5
    info = trk.get_global_ba()["info16"]
    want = capi.debug_global_ba(p, n_iterations, robust)["info16"]
    assert info.tolist() == want.tolist() and info[0] == 0, (info, want)
    n_free = int(info[1])
    panels = -(-6 * n_free // 48)
    solver = 1 if n_free <= 32 else 4 * panels - 1
    trial = 1 + solver + 3
    launches = 6 + n_iterations * (4 + 10 * trial)
    ran = 6 + 4 * int(info[6]) + trial * int(info[7])
    return dict(bench="global_ba", shape=name, keyframes_free=n_free, keyframes_fixed=int(info[2]), points=P, observations=E,
                n_iterations=n_iterations, robust=int(robust), info16=info[:9].tolist(), ms_call=round(1e3 * float(np.median(batches)), 4),
                solver="k_ba_solve (LDS)" if n_free <= 32 else f"blocked LDL^T, {panels} panels", launches=launches, launches_that_ran=ran)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "global_ba_bench.jsonl"))
    ap.add_argument("--traced", default=None, help="(the child under rocprofv3) make TRACED_CALLS calls of this shape and exit")
    a = ap.parse_args()
    import sdslam_amd as sd
    from sdslam_amd import capi
    import gba_cases
    shapes = [("mono_init", gba_cases.mono_init(), 20, True), ("loop", gba_cases.band(128, 2000, seed=19), 10, False)]
    if a.traced:
        name, p, nit, robust = next(s for s in shapes if s[0] == a.traced)
        bench(sd, capi, name, p, nit, robust, 320, 240, calls=TRACED_CALLS)
        return
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    rows = []
    for name, p, nit, robust in shapes:
        rows.append(bench(sd, capi, name, p, nit, robust, 320, 240))
    for res in rows:                                       # each trace in a run of its own, after the timed ones
        n_free = res["keyframes_free"]
        res.update(traced(res["shape"], res["info16"][7], 1 if n_free <= 32 else -(-6 * n_free // 48)))
        print(json.dumps(res))
    with open(a.out, "w") as f:
        f.write("".join(json.dumps(res) + "\n" for res in rows))


if __name__ == "__main__":
    main()
