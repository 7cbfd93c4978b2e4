#!/usr/bin/env python3
"""bench.py -- tracked frames/s of the per-frame tracking hot path on MI355X.

    python bench.py --gpus N --steps K --warmup W [--batch B] [--dump-outputs DIR] [--full]

Workload (BASELINE.json metric: "tracked frames/sec (ORB+ImageAlign+PnP) at 640x480, 1000 kp"):
one *step* tracks a batch of B independent 640x480 frames, all resident in HBM:
    ORB extract (8 levels x1.2, 1000 kp)  ->  ImageAlign (levels 4,3,2, <=30 GN its each)
    ->  SearchByProjection (th 8, mono, orientation check)  ->  PnP RANSAC (<=200 its, EPnP)
    ->  the batch's 160-byte pose records packed on the device
i.e. the TrackWithMotionModel sequence of SURVEY.md §3.2 / config C4.  The last frames' pyramids, map points and the
predicted poses are set up (untimed) beforehand, exactly as the previous tracking step would have left them.

N > 1: one process per GPU over torch.distributed (backend nccl = RCCL).  Either the driver launches the ranks
(torch.distributed.run: RANK / LOCAL_RANK / WORLD_SIZE in the environment) or `python bench.py --gpus N` starts N child
ranks itself.  Frames are independent, so ranks share nothing on the data path (weak scaling: B frames per GPU); the only
exchange is ONE all-gather per step of the fixed-size pose records, issued INSIDE the timed region straight from the
device buffer the last tracking kernel wrote.  Rank 0 prints ONE JSON line.

Variants (same metric name, `config.pose_solver` says which): --pose-solver poseopt = Optimizer::PoseOptimization instead
of PnP RANSAC (what the reference's TrackWithMotionModel really calls); motion_model = the whole
Tracking::TrackWithMotionModel as one device-side call; track adds Tracking::TrackLocalMap over a ~1000-point local map.
--orb-only times extraction alone, --hamming extraction + brute-force SearchByPoints (BASELINE configs[1]: "ORB extract +
Hamming match"), --res WxH other frame sizes, --batch 1 the single-frame latency.

A plain run sets up, warms up, times the K steps and prints the headline line (metric, value, unit, ms_per_step,
higher_is_better, dtype, config).  --dump-outputs DIR writes what the last timed step computed -- the pose records and the
per-frame read-outs of every stage, per-keypoint arrays for a fixed, seeded sample of frames -- as DIR/<name>.npy (float32 /
float64); the inputs are seeded, so two builds can be compared output for output.

--full adds everything beyond the headline: per-stage HIP-event timers inside the timed region (stages_ms_per_step), the
tracking summary, the check of the device-packed / gathered records, the run-to-run spread, and these objects:
  roofline     -- dominant kernel stage: algorithmic bytes per launch / its mean duration (HIP events on the
                  launch stream inside the timed region) against HBM peak; `valu` = the same stage against the measured
                  vector-ALU issue rate, `traffic` = HBM bytes from the committed rocprofv3 PMC passes
  cpu_baseline -- the CPU oracle (a port of the reference path; the reference needs OpenCV/Eigen and cannot be built
                  here) timed on this host: 1 thread (the reference's tracking is single-threaded) with median / p95 per
                  stage, and all cores (one independent frame stream per core)
  stress       -- the hard cases the default workload does not reach: ImageAlign from an identity prior, PnP RANSAC on 40 %
                  outliers, PnP RANSAC forced through all 200 iterations
  h2d_inclusive -- frames/s when every step first uploads its frames from page-locked host memory (never `value`)
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0   # MI355X HBM3E spec peak (MI355X_MICROARCH.md)
CFG = (1000, 1.2, 8, 20)
W, H = 640, 480
BOUNDS = (0.0, 640.0, 0.0, 480.0)
PNP = dict(probability=0.99, min_inliers=10, max_iterations=200, min_set=4, epsilon=0.28, th2=5.991)
RECORD_SOURCE = {"pnp": 0, "poseopt": 1, "motion_model": 2, "track": 3}
# Vector-ALU issue model (measured with tools/valu_microbench.hip on an MI355X, profiles/r03_valu_microbench*.json,
# 8 waves per SIMD, every CU busy, both timing methods within 1-10 %): a full-rate wave64 instruction (v_add / sub / and / or /
# xor / lshrrev / mov, f32 add / mul / fma, 16-bit min / max / sub) occupies a SIMD for 2.2 shader cycles, a half-rate one -- 32-bit
# min / max, v_max3 / v_min3, v_perm, v_alignbyte, shifts left, bfe, 24-bit multiplies, bcnt / mbcnt, dot4 / dot2, every v_pk_*, every
# SDWA form, fp64, compares (4.26) -- for 4.15.  The names below say "vop2" / "vop3" for historical reasons: read them as the
# full-rate and the half-rate bound.  256 CUs x 4 SIMDs at CLK_GHZ (2.38 GHz median under this load, tools/clock_probe.sh).
N_SIMD, CLK_GHZ, VALU_CYCLES_VOP2, VALU_CYCLES_VOP3 = 1024, 2.4, 2.2, 4.15


def _scene(args):
    i, seed0, w, h = args
    from sdslam_amd import synth
    rng = np.random.default_rng(seed0 + 7919 * i)
    ups = np.array([0.02, -0.01, 0.015]) + rng.normal(size=3) * 0.004
    om = np.array([0.4, -0.3, 0.5]) + rng.normal(size=3) * 0.1
    return synth.make_scene(seed0 + i, tuple(ups), tuple(om), w, h)


def make_cases(n_unique, seed0, w=640, h=480, pool=None):
    """n_unique two-view scenes with slightly different motions."""
    jobs = [(i, seed0, w, h) for i in range(n_unique)]
    return pool.map(_scene, jobs) if pool is not None else [_scene(j) for j in jobs]


# ------------------------------------------------------------------------------------------------ CPU baseline
STAGES_CPU = ["pyramid", "fast_nms", "select", "ic_angle", "blur", "rbrief", "image_align", "search_by_projection", "pose_solve"]


def cpu_loop(scenes, lasts, T0s, rs, budget_s, pose_solver="pnp", locals_=None, max_frames=1000, warm=20):
    """The oracle's full tracking step (-O3 -march=native build), one thread: per-frame stage times [n, 9] in ms."""
    from oracle import oracle as O
    from sdslam_amd import synth
    K = (synth.FX, synth.FY, synth.CX, synth.CY)
    O.lib(True)
    ora_ref = [O.OrbOracle(*CFG, fast_build=True) for _ in scenes]
    for o, s in zip(ora_ref, scenes):
        o.extract(s["ref"])
    ref_pyr = [[o.level(l) for l in range(CFG[2])] for o in ora_ref]
    cur = O.OrbOracle(*CFG, fast_build=True)
    tab = cur.tables()
    rows = []
    t0 = time.perf_counter()
    n = 0
    while True:
        i = n % len(scenes)
        s, last = scenes[i], lasts[i]
        ck, cd = cur.extract(s["cur"])
        st = list(cur.stage_ns() / 1e6)
        pc = [cur.level(l) for l in range(CFG[2])]          # Python-side copies between the C calls: not timed
        ta = time.perf_counter()
        if pose_solver in ("motion_model", "track"):          # the reference functions as a whole (oracle composition)
            r = O.track_with_motion_model(pc, ref_pyr[i], tab, ck, cd, BOUNDS, K, s["T_ref"], T0s[i], last, 8.0, mono=True)
            tb = time.perf_counter()
            if pose_solver == "track":
                O.track_local_map(ck, cd, tab, np.log(np.float32(CFG[1])), BOUNDS, K, r["T"], r["match"], last, locals_[i], th=1.0)
            tc = time.perf_counter()
            st += [(tb - ta) * 1e3, (tc - tb) * 1e3, 0.0]
        else:
            r = O.align(pc, ref_pyr[i], tab["inv_sf"], tab["sf"], last["Xw"][last["valid"] != 0], s["T_ref"], T0s[i], K, 0)
            tb = time.perf_counter()
            nm, cm = O.search_by_projection(ck, cd, tab["sf"], BOUNDS, K, r["T"], s["T_ref"], last, th=8.0)
            tc = time.perf_counter()
            valid = (cm >= 0).astype(np.uint8)
            Xw = np.zeros((len(ck), 3))
            Xw[valid != 0] = last["Xw"][cm[valid != 0]]
            if pose_solver == "pnp":
                p = O.PnPOracle(valid, np.stack([ck["x"], ck["y"]], 1), ck["octave"], tab["sigma2"], Xw, K)
                p.set_ransac(PNP["probability"], PNP["min_inliers"], PNP["max_iterations"], 4, PNP["epsilon"], PNP["th2"])
                p.iterate(PNP["max_iterations"], rs)
            else:
                O.pose_optimization(ck, valid, Xw, tab["inv_sigma2"], K, r["T"])
            td = time.perf_counter()
            st += [(tb - ta) * 1e3, (tc - tb) * 1e3, (td - tc) * 1e3]
        n += 1
        if n > warm:
            rows.append(st)
        if time.perf_counter() - t0 > budget_s or len(rows) >= max_frames:
            break
    return np.array(rows)


def parse_pyramid(txt):
    """'8x1.2' -> (1000, 1.2, 8, 20): levels x scale factor; '5x2.0' is the reference's own default (src/Config.cc:48-51)."""
    nl, sf = txt.lower().split("x")
    return (1000, float(sf), int(nl), 20)


def cpu_worker_main(argv):
    """`bench.py --cpu-worker SEED BUDGET POSE_SOLVER PYRAMID`: one independent frame stream on one core (the all-cores leg)."""
    global CFG
    seed, budget, solver = int(argv[0]), float(argv[1]), argv[2]
    if len(argv) > 3:
        CFG = parse_pyramid(argv[3])
    from oracle import oracle as O
    from sdslam_amd import synth
    scenes = make_cases(1, seed)
    orf = O.OrbOracle(*CFG, fast_build=True)
    rk, rd = orf.extract(scenes[0]["ref"])
    lasts = [synth.tracking_case(0, rk, rd)]
    T0 = [synth.se3_exp((0.003, -0.002, 0.001), (0.05, 0.02, -0.04)) @ scenes[0]["T_cur"]]
    rs = synth.glibc_rand_stream(4 * PNP["max_iterations"])
    loc = None
    if solver == "track":
        oc = O.OrbOracle(*CFG, fast_build=True)
        ck, cd = oc.extract(scenes[0]["cur"])
        loc = [{k: v[:1000] for k, v in synth.local_map_case(500, ck, cd, scenes[0]["T_cur"], scale_factor=CFG[1], nlevels=CFG[2]).items()}]
    t0 = time.perf_counter()
    rows = cpu_loop(scenes, lasts, T0, rs, budget, solver if solver != "hamming" else "pnp", loc, max_frames=100000, warm=20)
    print(json.dumps({"frames": len(rows), "busy_s": float(rows.sum() / 1e3), "wall_s": time.perf_counter() - t0}))


def cgroup_cpu_quota():
    """CPU cores the cgroup grants (quota / period), or None when unlimited / unknown."""
    try:
        q, per = open("/sys/fs/cgroup/cpu.max").read().split()[:2]
        return None if q == "max" else float(q) / float(per)
    except Exception:
        pass
    try:
        q = float(open("/sys/fs/cgroup/cpu/cpu.cfs_quota_us").read())
        per = float(open("/sys/fs/cgroup/cpu/cpu.cfs_period_us").read())
        return None if q <= 0 else q / per
    except Exception:
        return None


def cpu_baseline(scenes, lasts, T0s, rs, pose_solver="pnp", locals_=None, budget_1=12.0, budget_all=8.0):
    rows = cpu_loop(scenes, lasts, T0s, rs, budget_1, pose_solver, locals_)
    per_frame = rows.sum(axis=1)
    ncores = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    quota = cgroup_cpu_quota()           # cores this process may really use (cgroup v2 cpu.max / v1 cfs quota), None = unlimited
    nwork = max(1, min(ncores, 64, int(quota) if quota else 64))
    procs = [subprocess.Popen([sys.executable, os.path.abspath(__file__), "--cpu-worker", str(3000 + i), str(budget_all), pose_solver,
                               f"{CFG[2]}x{CFG[1]}"], stdout=subprocess.PIPE, text=True) for i in range(nwork)]
    outs = []
    for p in procs:
        o, _ = p.communicate(timeout=600)
        if p.returncode == 0 and o.strip():
            outs.append(json.loads(o.strip().splitlines()[-1]))
    all_fps = float(sum(o["frames"] / o["busy_s"] for o in outs)) if outs else None
    model = ""
    try:
        model = [l.split(":", 1)[1].strip() for l in open("/proc/cpuinfo") if l.startswith("model name")][0]
    except Exception:
        pass
    what = {"pnp": "PnP RANSAC", "poseopt": "PoseOptimization", "motion_model": "Tracking::TrackWithMotionModel (align+match+pose under image_align)",
            "track": "TrackWithMotionModel + TrackLocalMap (under search_by_projection)"}[pose_solver]
    return {"value": float(len(rows) / (per_frame.sum() / 1e3)), "unit": "frames/s", "cores": 1, "kind": "port",
            "sample": f"{len(rows)} VGA frame pairs after 20 warm-up, full step (ORB extract + ImageAlign + SearchByProjection + {what}), "
                      f"1 thread; all-cores leg: {len(outs)} processes x {budget_all:.0f} s, one independent frame stream each",
            "ms_per_frame_median": float(np.median(per_frame)), "ms_per_frame_p95": float(np.percentile(per_frame, 95)),
            "stages_ms_median": {k: float(v) for k, v in zip(STAGES_CPU, np.median(rows, axis=0))},
            "stages_ms_p95": {k: float(v) for k, v in zip(STAGES_CPU, np.percentile(rows, 95, axis=0))},
            "all_cores": {"value": all_fps, "unit": "frames/s", "cores": len(outs), "host_cpus_visible": ncores, "cgroup_cpu_quota": quota,
                          "cpu_model": model, "note": "workers = min(CPUs in the affinity mask, cgroup quota, 64)"}}


# ------------------------------------------------------------------------------------------------ PMC / VALU figures
STAGE_KERNELS = {"pyramid": ["k_pyr_split", "k_pyr_resize", "k_pyr_edges", "k_pyr_rows", "k_pyr_level"], "fast_nms": ["k_fast_cells"],
                 "select": ["k_select_quota", "k_select_cells", "k_select_bigcells", "k_select_final", "k_select_level"], "blur": ["k_blur"], "orient_desc": ["k_orient_desc"], "image_align": ["k_align"],
                 "search_by_projection": ["k_match_cand", "k_match_assign", "k_match"], "pnp_ransac": ["k_pnp"], "search_by_points": ["k_search_points"]}
PMC_FRAMES = 1024       # frames per launch in the committed PMC passes (tools/run_profiles.sh: default batch)


def pmc_for_stage(stage, batch):
    """HBM bytes per launch (FETCH_SIZE with the gfx950 correction + WRITE_SIZE, MI355X_MICROARCH.md) and VALU issue figures
    of the stage's kernels from the newest committed profiles/*pmc_summary*.json; (None, None) if absent.  PMC counters
    cannot be collected from inside this process; the passes are rocprofv3 runs of this same command."""
    import glob
    files = sorted(glob.glob(os.path.join(ROOT, "profiles", "r*_pmc_summary_b1024.json")))
    if not files:
        return None, None
    d = json.load(open(files[-1]))
    tot, valu, dur = 0.0, 0.0, 0.0
    found = False

    def entry(name):      # templated kernels appear as "void k_align<4>"
        for key, val in d.items():
            if key == name or key.replace("void ", "").split("<")[0] == name:
                return val
        return None
    for k in STAGE_KERNELS.get(stage, []):
        e = entry(k)
        if not e or "FETCH_bytes_corrected_per_launch" not in e:
            continue
        found = True
        # launches per step: relative to a kernel that runs once per step (the pyramid and FAST kernels run per level)
        calls = max(1, round(e.get("duration_ns_samples", 1) / max((d.get("k_select_final") or d.get("k_select_level") or {}).get("duration_ns_samples", 1), 1)))
        tot += calls * (e["FETCH_bytes_corrected_per_launch"] + e.get("WRITE_bytes_per_launch", 0.0))
        valu += calls * e.get("SQ_INSTS_VALU_per_launch", 0.0)
        dur += calls * e.get("duration_ns_per_launch", 0.0)
    if not found:
        return None, None
    sc = batch / PMC_FRAMES
    lo_ms = valu * sc / N_SIMD * VALU_CYCLES_VOP2 / (CLK_GHZ * 1e9) * 1e3
    hi_ms = valu * sc / N_SIMD * VALU_CYCLES_VOP3 / (CLK_GHZ * 1e9) * 1e3
    return tot * sc, {"wave_insts_per_step": valu * sc, "cycles_per_inst_measured": {"vop2": VALU_CYCLES_VOP2, "vop3_three_source": VALU_CYCLES_VOP3},
                      "min_ms_if_all_vop2": lo_ms, "min_ms_if_all_vop3": hi_ms, "min_ms_at_full_issue": lo_ms,
                      "profiled_kernel_ms": dur * sc / 1e6, "source": os.path.basename(files[-1])}


# ------------------------------------------------------------------------------------------------ the GPU workload
class Workload:
    """Everything one rank keeps resident, and the step bench.py times (tests/test_bench_step_gpu.py runs the same object)."""

    def __init__(self, scenes, batch, device=0, pose_solver="pnp", orb_only=False, hamming=False, w=640, h=480, rank=0):
        import sdslam_amd
        from sdslam_amd import synth
        from sdslam_amd.capi import DeviceBuffer
        self.sd, self.synth = sdslam_amd, synth
        self.B, self.w, self.h = batch, w, h
        self.pose_solver, self.orb_only, self.hamming = pose_solver, orb_only, hamming
        self.bounds = (0.0, float(w), 0.0, float(h))
        self.K = (synth.FX, synth.FY, synth.CX, synth.CY)
        B = batch
        self.scenes = scenes
        self.nu = nu = max(1, min(len(scenes), B))
        self.idx = [i % nu for i in range(B)]
        cur_frames = np.stack([scenes[i]["cur"] for i in self.idx])
        self.d_cur = DeviceBuffer(cur_frames.nbytes)
        self.d_cur.upload(cur_frames)
        self.cur_frames_host = cur_frames
        self.cur = sdslam_amd.ORBextractor(*CFG, w, h, B, device=device)
        self.ref = sdslam_amd.ORBextractor(*CFG, w, h, B, device=device)
        self.trk = sdslam_amd.Tracker(self.cur, self.ref, max_points=1000, max_batch=B, pnp_max_iterations=PNP["max_iterations"])
        self.trk.set_camera(*self.K, 0.0, self.bounds)
        # ---- untimed setup: what the previous tracking step leaves behind
        ref_u = np.stack([s["ref"] for s in scenes[:nu]])
        rk, rd, rn = self.ref.extract_batch(ref_u)                       # unique last frames first: their keypoints seed the map points
        self.lasts_u = [synth.tracking_case(i, rk[i, :rn[i]], rd[i, :rn[i]]) for i in range(nu)]
        if B > nu:
            d_ref = DeviceBuffer(ref_u[0].nbytes * B)
            d_ref.upload(np.stack([scenes[i]["ref"] for i in self.idx]))
            self.ref.extract_batch_device(d_ref.ptr, B, w, h)
            self.ref.sync()
            d_ref.free()
        self.trk.set_last(0, [self.lasts_u[i] for i in self.idx])
        pert = synth.se3_exp((0.003, -0.002, 0.001), (0.05, 0.02, -0.04))   # motion-model prediction error
        self.T0_u = [pert @ s["T_cur"] for s in scenes[:nu]]
        self.T_ref = [scenes[i]["T_ref"] for i in self.idx]
        self.T0 = [self.T0_u[i] for i in self.idx]
        self.rs = synth.glibc_rand_stream(4 * PNP["max_iterations"])
        self.trk.set_rand(0, np.tile(self.rs, (B, 1)))
        self.trk.set_poses(0, self.T_ref, self.T0)         # last-frame poses + motion-model predictions (resident, like the frames)
        self.locals_u = None
        if pose_solver == "track" and not orb_only:        # the local map of every frame (UpdateLocalMap is the caller's)
            ck, cd, cn = self.cur.extract_batch(np.stack([s_["cur"] for s_ in scenes[:nu]]))
            self.locals_u = [{k: v[:1000] for k, v in synth.local_map_case(500 + i, ck[i, :cn[i]], cd[i, :cn[i]], scenes[i]["T_cur"], scale_factor=CFG[1], nlevels=CFG[2]).items()}
                             for i in range(nu)]
            self.trk.set_local(0, [self.locals_u[i] for i in self.idx])
        if hamming:
            ones = np.ones((B, self.cur.cap), np.uint8)
            self.trk.set_point_flags(0, ones, ones)
        self.pnp_epsilon = PNP["epsilon"]
        self.rec_ptr = [None, None]      # device record buffers (set by attach_records)
        self.k = 0

    def attach_records(self, ptr0, ptr1):
        self.rec_ptr = [ptr0, ptr1]

    def record_source(self):
        return 4 if (self.orb_only or self.hamming) else RECORD_SOURCE[self.pose_solver]

    def step(self, d_ptr=None):
        """One pass of the hot path over the resident batch; ends with the pose records packed on the device."""
        B, trk = self.B, self.trk
        self.cur.extract_batch_device(self.d_cur.ptr if d_ptr is None else d_ptr, B, self.w, self.h)
        if self.hamming:
            trk.search_by_points(B, 0.75, True)
        elif self.orb_only:
            pass
        elif self.pose_solver in ("motion_model", "track"):
            trk.track_with_motion_model(B, th=8.0, mono=True, align_mode=0)
            if self.pose_solver == "track":
                trk.track_local_map(B, th=1.0)
        else:
            trk.align(B, 0)
            trk.match(B, 8.0, True, True)
            if self.pose_solver == "pnp":
                trk.pnp(B, PNP["probability"], PNP["min_inliers"], PNP["max_iterations"], PNP["min_set"], self.pnp_epsilon,
                        PNP["th2"], PNP["max_iterations"])
            else:
                trk.pose_opt(B, 0)
        if self.rec_ptr[0] is not None and not self.orb_only:
            trk.pack_records(B, self.record_source(), self.rec_ptr[self.k % 2])
        self.k += 1

    def results(self):
        """Host copies of what the last step left (align, matches, pose solve)."""
        B, trk = self.B, self.trk
        al = trk.get_align(0, B)
        cm, nm = trk.get_matches(0, B)
        if self.pose_solver == "pnp" or self.orb_only or self.hamming:
            pn = trk.get_pnp(0, B)
        elif self.pose_solver == "motion_model":
            po, tw = trk.get_pose_opt(0, B), trk.get_tracked(0, B)
            pn = dict(ok=tw["status"] == 2, n_inliers=tw["nmatches_map"], iterations=po["iterations"], N=po["n_initial"])
        elif self.pose_solver == "track":
            po, tl = trk.get_pose_opt(0, B), trk.get_local_map(0, B)
            pn = dict(ok=tl["status"] == 2, n_inliers=tl["n_inliers"], iterations=po["iterations"], N=po["n_initial"])
        else:
            po = trk.get_pose_opt(0, B)
            pn = dict(ok=po["n_inliers"] >= 10, n_inliers=po["n_inliers"], iterations=po["iterations"], N=po["n_initial"])
        return al, cm, nm, pn


def stress_legs(wl, steps=6):
    """The cases the default scenes do not reach: ImageAlign from an identity prior (worst case of SURVEY C3),
    PnP RANSAC on a planted 40 %-outlier match vector, and PnP RANSAC that can never accept (exactly minInliers exact
    inliers: every refit fails the strict `>`), i.e. all 200 iterations for every frame."""
    import torch
    B, trk, synth = wl.B, wl.trk, wl.synth
    out = {}

    def timed(fn, n):
        fn()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        wl.cur.sync()
        trk.get_tracked(0, 1)          # synchronises the tracking stream
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) / n

    # (a) identity prior: the whole step, alignment starts from I instead of the motion-model prediction
    trk.set_poses(0, wl.T_ref, [np.eye(4)] * B)
    dt = timed(wl.step, steps)
    al = trk.get_align(0, B)
    out["align_identity_prior"] = {"frames_per_s": B / dt, "ms_per_step": dt * 1e3, "mean_gn_iterations": float(al["iters"][:, :8].sum(axis=1).mean()),
                                   "align_ok": int(al["ok"].sum())}
    trk.set_poses(0, wl.T_ref, wl.T0)
    # (b), (c): PnP alone on caller-supplied match vectors (sd_track_set_matches)
    ck, cd, cn = wl.cur.download(0, wl.nu)
    for name, kw, eps in (("pnp_outliers40", dict(n_match=300, outlier_frac=0.40, noise_px=0.5), PNP["epsilon"]),
                          ("pnp_forced_200_iterations", dict(n_match=300, outlier_frac=0.0, n_exact_inliers=84), PNP["epsilon"])):
        cases = [synth.planted_matches(900 + i, ck[i, :cn[i]], wl.scenes[i]["T_cur"], **kw) for i in range(wl.nu)]
        trk.set_last(0, [cases[i][0] for i in wl.idx])
        cmv = np.full((B, wl.cur.cap), -1, np.int32)
        for b, i in enumerate(wl.idx):
            cmv[b, :len(cases[i][1])] = cases[i][1]
        trk.set_matches(0, cmv)
        fn = lambda: trk.pnp(B, PNP["probability"], PNP["min_inliers"], PNP["max_iterations"], 4, eps, PNP["th2"], PNP["max_iterations"])  # noqa: E731
        dt = timed(fn, steps)
        g = trk.get_pnp(0, B)
        out[name] = {"ms_per_launch": dt * 1e3, "frames": B, "mean_iterations": float(g["iterations"].mean()), "max_iterations": int(g["iterations"].max()),
                     "returned": int(g["ok"].sum()), "refined": int(g["refined"].sum()), "mean_inliers": float(g["n_inliers"].mean())}
    trk.set_last(0, [wl.lasts_u[i] for i in wl.idx])
    if wl.pose_solver != "pnp":
        return out
    # (d), (e): the WHOLE step on a hard scene: 40 % of every last frame's map points moved sideways by 4-7 px (times their
    # octave's scale) of reprojection -- inside the matcher's window, outside PnP's chi2 gate, so the matcher itself hands PnP
    # 40 % outliers -- and (e) the same with SetRansacParameters(epsilon = 0.99): minInliers = 0.99 N is never reached, every
    # frame runs all 200 iterations (EPnP + CheckInliers each, no refit)
    hard = []
    for i, l in enumerate(wl.lasts_u):
        rng = np.random.default_rng(7000 + i)
        h = {k: v.copy() for k, v in l.items()}
        idx = np.flatnonzero(h["valid"])
        sel = rng.choice(idx, size=int(0.4 * len(idx)), replace=False)
        ang = rng.uniform(0, 2 * np.pi, len(sel))
        px = rng.uniform(4.0, 7.0, len(sel)) * (CFG[1] ** h["octave"][sel])
        Tr = wl.scenes[i]["T_ref"]
        zc = (h["Xw"][sel] @ Tr[:3, :3].T + Tr[:3, 3])[:, 2]
        d_cam = np.stack([np.cos(ang), np.sin(ang), np.zeros(len(sel))], 1) * (px * zc / wl.K[0])[:, None]
        h["Xw"][sel] += d_cam @ Tr[:3, :3]          # camera-frame offset -> world (R^T d)
        hard.append(h)
    trk.set_last(0, [hard[i] for i in wl.idx])
    for name, eps in (("full_step_outliers40", PNP["epsilon"]), ("full_step_forced_200", 0.99)):
        wl.pnp_epsilon = eps
        dt = timed(wl.step, steps)
        g, (cm, nm), al = trk.get_pnp(0, B), trk.get_matches(0, B), trk.get_align(0, B)
        out[name] = {"frames_per_s": B / dt, "ms_per_step": dt * 1e3, "mean_matches": float(nm.mean()), "mean_pnp_iterations": float(g["iterations"].mean()),
                     "max_pnp_iterations": int(g["iterations"].max()), "pnp_returned": int(g["ok"].sum()), "mean_pnp_inliers": float(g["n_inliers"].mean()),
                     "mean_inlier_fraction": float((g["n_inliers"] / np.maximum(g["N"], 1)).mean()), "align_ok": int(al["ok"].sum())}
    wl.pnp_epsilon = PNP["epsilon"]
    trk.set_last(0, [wl.lasts_u[i] for i in wl.idx])
    return out


def h2d_overlapped_leg(wl, steps=6):
    """The upload of step n + 1 overlapped with step n: two device frame buffers, a copy stream; sd_orb_stream_fence orders the
    extraction of a buffer behind its upload and the next upload into a buffer behind the extraction that read it."""
    import torch
    B = wl.B
    host = torch.from_numpy(wl.cur_frames_host).pin_memory()
    dbuf = [torch.empty_like(host, device="cuda") for _ in range(2)]
    cs = torch.cuda.Stream()
    cur = wl.cur

    def upload(k):
        cur.stream_fence(cs.cuda_stream, 0)            # the extraction that read this buffer (step k - 2) is done
        with torch.cuda.stream(cs):
            dbuf[k % 2].copy_(host, non_blocking=True)

    def run(n):
        upload(0)
        for k in range(n):
            cur.stream_fence(cs.cuda_stream, 1)        # extraction k waits for upload k (the copy stream's last operation)
            upload(k + 1)
            wl.step(dbuf[k % 2].data_ptr())
        cur.sync()
        wl.trk.get_tracked(0, 1)
        torch.cuda.synchronize()

    run(2)
    t0 = time.perf_counter()
    run(steps)
    dt = (time.perf_counter() - t0) / steps
    al = wl.trk.get_align(0, B)
    return {"frames_per_s": B / dt, "ms_per_step": dt * 1e3, "upload_GBps_sustained": host.numel() / dt / 1e9, "align_ok": int(al["ok"].sum()),
            "note": "upload of step n+1 on a copy stream beside step n (two device frame buffers, sd_orb_stream_fence)"}


def drop_in_leg(wl, frames=600, nscenes=8):
    """The drop-in call style, one frame at a time (VERDICT r2 missing #5): tools/dropin_bench.cc drives the C++ facade's
    reference-shaped overloads -- host image in, Frame construction (ORB extraction), ImageAlign::ComputePose,
    ORBmatcher::SearchByProjection, Optimizer::PoseOptimization, pose out -- on a ping-pong sequence of the bench scenes;
    median / p95 per frame over >= 500 frames.  Compiled with g++ against the in-tree library and run as a child process."""
    import struct
    import tempfile
    synth = wl.synth
    ns = min(nscenes, wl.nu)
    ck, cd, cn = wl.cur.download(0, ns)
    pert = synth.se3_exp((0.003, -0.002, 0.001), (0.05, 0.02, -0.04))
    tmp = tempfile.mkdtemp(prefix="sd_dropin_")
    raw, exe = os.path.join(tmp, "scenes.bin"), os.path.join(tmp, "dropin_bench")

    def view(f, img, T, pts):
        f.write(np.ascontiguousarray(img).tobytes())
        f.write(np.ascontiguousarray(T.T).tobytes())
        f.write(np.ascontiguousarray((pert @ T).T).tobytes())
        idx = np.flatnonzero(pts["valid"])
        f.write(struct.pack("<i", len(idx)))
        for i in idx:
            f.write(struct.pack("<i3d", int(i), *pts["Xw"][i]) + pts["desc"][i].tobytes())
    with open(raw, "wb") as f:
        f.write(struct.pack("<i", ns))
        for i in range(ns):
            sc = wl.scenes[i]
            view(f, sc["ref"], sc["T_ref"], wl.lasts_u[i])
            view(f, sc["cur"], sc["T_cur"], synth.keyframe_case(ck[i, :cn[i]], cd[i, :cn[i]], sc["T_cur"], max_points=300))
    libdir = os.path.dirname(wl.sd.lib_path())
    try:
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-I", os.path.join(ROOT, "include"), os.path.join(ROOT, "tools", "dropin_bench.cc"), "-o", exe,
                               "-L", libdir, "-lsdslam_hip", f"-Wl,-rpath,{libdir}"])
        out = subprocess.run([exe, raw, str(frames)], capture_output=True, text=True, timeout=300)
        if out.returncode != 0:
            return {"error": f"dropin_bench exited with {out.returncode}: {out.stderr[-300:]}"}
        r = json.loads(out.stdout.strip().splitlines()[-1])
    except (OSError, subprocess.SubprocessError) as e:
        return {"error": f"could not build / run tools/dropin_bench.cc: {e}"}
    r["frames_per_s"] = 1e3 / r["ms_per_frame_median"]
    r["what"] = ("one frame at a time through the C++ facade (FrameTracker overloads on reference-shaped Frame / MapPoint objects): host image -> "
                 "ORBextractor::operator() -> ImageAlign::ComputePose -> ORBmatcher::SearchByProjection -> Optimizer::PoseOptimization -> pose on the "
                 "host; the reference logs this quantity as 'Tracking time' (src/System.cc:179-184)")
    return r


def h2d_leg(wl, steps=4):
    """Frames in page-locked host memory, uploaded at the start of every step (synchronous copy, then the step)."""
    import torch
    from sdslam_amd.capi import pinned_array, lib, _p
    pf, owner = pinned_array(wl.cur_frames_host.shape)
    pf[...] = wl.cur_frames_host

    def once():
        lib().sd_dev_upload(wl.d_cur.ptr, _p(pf), pf.nbytes)
        wl.step()
    once()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        once()
    wl.cur.sync()
    wl.trk.get_tracked(0, 1)
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / steps
    return {"frames_per_s": wl.B / dt, "ms_per_step": dt * 1e3, "upload_GBps": pf.nbytes / dt / 1e9,
            "note": "synchronous upload from page-locked memory, not overlapped with the previous step"}


DUMP_SAMPLE_FRAMES = 64          # frames whose per-keypoint arrays are written (fixed seed); per-frame arrays cover the batch
DUMP_MAX_BYTES = 64 << 20


def dump_outputs(wl, out_dir, records=None, gathered=None):
    """`--dump-outputs DIR`: what the timed path computed in its last step, as a caller of it receives it -- the packed pose
    records and the stages' read-outs (keypoints, descriptors, alignment, matches, pose solve) -- one DIR/<name>.npy each.
    Floating-point arrays keep their width; integer / boolean ones are stored as float32 when exact there, float64 otherwise.
    Per-keypoint arrays ([frames, cap, ...]) are limited to a fixed, seeded sample of DUMP_SAMPLE_FRAMES frames."""
    B, trk = wl.B, wl.trk
    S = np.sort(np.random.default_rng(0).choice(B, min(B, DUMP_SAMPLE_FRAMES), replace=False))
    k, d, n = wl.cur.download(0, B)
    out = {"sample_frames": S, "n_keypoints": n, "keypoints": np.stack([k[f][S].astype(np.float32) for f in k.dtype.names], -1),   # x y size angle response octave class_id
           "descriptors": d[S]}
    if records is not None:
        out["records"] = records
    if gathered is not None:
        out["records_gathered"] = gathered
    if wl.hamming:
        m, nm = trk.get_point_matches(0, B)
        out.update(point_matches=m[S], n_point_matches=nm)
    elif not wl.orb_only:
        al = trk.get_align(0, B)
        cm, nm = trk.get_matches(0, B)
        out.update(align_T=np.stack(al["T"]), align_ok=al["ok"], align_error=al["error"], align_iterations=al["iters"],
                   align_chi2=al["chi2"], matches=cm[S], n_matches=nm)
        if wl.pose_solver == "pnp":
            g = trk.get_pnp(0, B)
            out.update(pnp_T=g["T"], pnp_ok=g["ok"], pnp_n_inliers=g["n_inliers"], pnp_iterations=g["iterations"],
                       pnp_refined=g["refined"], pnp_inliers=g["inliers"][S])
        else:
            po = trk.get_pose_opt(0, B)
            out.update(pose_opt_T=np.stack(po["T"]), pose_opt_n_inliers=po["n_inliers"], pose_opt_iterations=po["iterations"],
                       pose_opt_outliers=po["outlier"][S])
            if wl.pose_solver in ("motion_model", "track"):
                tw = trk.get_tracked(0, B)
                out.update(tracked_status=tw["status"], tracked_nmatches=tw["nmatches"], tracked_nmatches_map=tw["nmatches_map"])
            if wl.pose_solver == "track":
                tl = trk.get_local_map(0, B)
                out.update(local_map_matches=tl["match"][S], local_map_status=tl["status"], local_map_n_inliers=tl["n_inliers"])
    arrays = {}
    for name, a in out.items():
        a = np.asarray(a)
        if a.dtype.kind != "f":
            a = a.astype(np.float32 if a.size == 0 or np.abs(a.astype(np.int64)).max() < (1 << 24) else np.float64)
        arrays[name] = a
    total = sum(a.nbytes for a in arrays.values())
    assert total <= DUMP_MAX_BYTES, f"--dump-outputs: {total} bytes exceed the {DUMP_MAX_BYTES}-byte limit"
    os.makedirs(out_dir, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + ".npy"), a)


def full_figures(line, args, wl, scenes, rec_host, orb_ms, trk_ms, full_step):
    """`--full` (rank 0): per-stage times and the roofline of the dominant stage, the tracking summary, then the legs that run
    after the timed region -- run-to-run spread, stress, h2d, drop-in, CPU baseline -- added to `line`."""
    import sdslam_amd
    B, cur, trk, nu, world = wl.B, wl.cur, wl.trk, wl.nu, line["n_gpus"]
    al, cm, nm, pn = wl.results()
    if not args.orb_only and not args.hamming:      # the device-packed records equal the per-stage read-outs
        assert np.array_equal(rec_host[:, 17], nm.astype(np.float64)) and np.array_equal(rec_host[:, 18], pn["n_inliers"].astype(np.float64))
    solver_name = "pnp_ransac" if args.pose_solver == "pnp" else "pose_optimization"
    names = cur.stage_names() + ["image_align", "search_by_points" if args.hamming else "search_by_projection", solver_name]
    stage_ms = np.concatenate([orb_ms, trk_ms])
    sbytes = list(cur.stage_bytes())
    # algorithmic bytes of the tracking stages, from what this run actually did
    P = float(np.mean([min(300, int(l["valid"].sum())) for l in wl.lasts_u]))
    its = float(al["iters"][:, :8].sum(axis=1).mean())
    lv = sdslam_amd.plan_info(*CFG, W, H)["levels"]
    px_l = float(sum(lv[l, 0] * lv[l, 1] for l in (2, 3, 4)))
    sbytes += [its * P * (25 + 64) + 2 * px_l,                       # ImageAlign
               2 * 1000 * 32 if args.hamming else P * (32 + 10 * 32),   # brute force: compulsory descriptor reads; windowed: c ~ 10
               float(pn["iterations"].mean()) * (4 * 20 + float(pn["N"].mean()) * 24)]   # PnP
    dom = int(np.argmax(stage_ms))
    achieved = sbytes[dom] * B / (stage_ms[dom] * 1e-3) / 1e9
    traffic, valu = pmc_for_stage(names[dom], B)
    terr = float(np.mean([np.abs(al["T"][b][:3, 3] - scenes[wl.idx[b]]["T_cur"][:3, 3]).max() for b in range(min(B, nu))]))
    line.update({
        "stages_ms_per_step": {nm_: float(ms) for nm_, ms in zip(names, stage_ms)},
        "roofline": {"bound": "hbm", "kernel": names[dom], "achieved": achieved, "peak": HBM_PEAK_GBS,
                     "unit": "GB/s", "frac": achieved / HBM_PEAK_GBS, "traffic": traffic,
                     "algorithmic_bytes_per_frame": float(sbytes[dom]), "ms_per_step": float(stage_ms[dom]),
                     "note": "integer/byte kernel limited by vector-ALU issue, not HBM (DESIGN.md section 6); traffic = HBM bytes per "
                             "step from the committed rocprofv3 FETCH_SIZE/WRITE_SIZE passes (profiles/), scaled to this batch",
                     "valu": valu,
                     "valu_frac": (valu["min_ms_if_all_vop2"] / float(stage_ms[dom])) if valu else None,
                     "valu_frac_at_vop3_rate": (valu["min_ms_if_all_vop3"] / float(stage_ms[dom])) if valu else None},
        "tracking": {"align_ok": int(al["ok"].sum()), "mean_gn_iterations": its, "mean_matches": float(nm.mean()),
                     "pnp_ok": int(np.asarray(pn["ok"]).sum()), "mean_pnp_inliers": float(pn["n_inliers"].mean()),
                     "mean_pnp_iterations": float(pn["iterations"].mean()), "align_translation_err_m": terr},
    })
    if args.hamming:
        m12, n12 = trk.get_point_matches(0, B)
        line["tracking"]["mean_point_matches"] = float(n12.mean())
    if world == 1 and not args.no_extras:
        # run-to-run spread (the headline is one timed region): three more blocks of the same step, each
        # bracketed like the timed region, AFTER it; `value` stays the K-step figure above
        blocks = []
        nb = max(10, min(50, args.steps // 3))
        for _ in range(3):
            cur.sync()
            trk.get_tracked(0, 1)
            tb = time.perf_counter()
            for k in range(nb):
                full_step(k)
            cur.sync()
            trk.get_tracked(0, 1)
            blocks.append(B * nb / (time.perf_counter() - tb))
        line["repeatability"] = {"blocks": 3, "steps_per_block": nb, "frames_per_s": blocks,
                                 "spread": (max(blocks) - min(blocks)) / float(np.median(blocks))}
    if world == 1 and not args.orb_only and not args.hamming and not args.no_extras:
        line["stress"] = stress_legs(wl)
        line["h2d_inclusive"] = h2d_leg(wl)
        line["h2d_overlapped"] = h2d_overlapped_leg(wl)
        if CFG[1:3] == (1.2, 8) and (W, H) == (640, 480):
            line["drop_in"] = drop_in_leg(wl)
    if not args.no_cpu_baseline and world == 1 and not args.orb_only and not args.hamming:
        line["cpu_baseline"] = cpu_baseline(scenes[:min(nu, 8)], wl.lasts_u[:min(nu, 8)], wl.T0_u[:min(nu, 8)], wl.rs, pose_solver=args.pose_solver,
                                            locals_=wl.locals_u)
    else:
        line["cpu_baseline"] = None


def spawn_ranks(args):
    """`python bench.py --gpus N` without a launcher: start N child ranks (fresh processes, nothing GPU-related has run in
    this one), wait for all, fail if any fails."""
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    procs = []
    for r in range(args.gpus):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE=str(args.gpus), MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
        env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
        procs.append(subprocess.Popen([sys.executable, os.path.abspath(__file__)] + sys.argv[1:], env=env))
    rc = 0
    for p in procs:
        rc = rc or p.wait()
    sys.exit(rc)


def main():
    if len(sys.argv) > 1 and sys.argv[1] == "--cpu-worker":
        return cpu_worker_main(sys.argv[2:])
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=150)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batch", type=int, default=1024, help="frames per GPU per step")
    ap.add_argument("--unique", type=int, default=64, help="distinct synthetic scenes (tiled to --batch)")
    ap.add_argument("--full", action="store_true", help="also everything beyond the headline: per-stage timers, roofline, tracking "
                                                        "summary, record checks, run-to-run spread, stress / h2d / drop-in legs, CPU baseline")
    ap.add_argument("--dump-outputs", metavar="DIR", help="write what the last timed step computed as DIR/<name>.npy (float32 / float64)")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--no-extras", action="store_true", help="with --full: skip the spread / stress / h2d / drop-in legs (profiling runs)")
    ap.add_argument("--orb-only", action="store_true", help="time ORB extraction alone (configs[1] without matching)")
    ap.add_argument("--hamming", action="store_true", help="BASELINE configs[1]: ORB extract + brute-force Hamming match "
                                                            "(ORBmatcher::SearchByPoints, 1000 x 1000 per frame pair)")
    ap.add_argument("--pyramid", default="8x1.2", help="LEVELSxSCALE: 8x1.2 = BASELINE configs[1]/[3] (the metric); 5x2.0 = the reference's own "
                                                       "default pyramid (src/Config.cc:48-51), reported beside it")
    ap.add_argument("--option", action="append", default=[], metavar="NAME=VALUE",
                    help="sd_set_option before anything is created (A/B experiments; include/sdslam_hip.h lists the options)")
    ap.add_argument("--res", default="640x480", help="frame size WxH (BASELINE configs[4] uses 1280x720 frames; the metric is quoted at 640x480)")
    ap.add_argument("--pose-solver", choices=["pnp", "poseopt", "motion_model", "track"], default="pnp",
                    help="pnp: PnPsolver RANSAC (the BASELINE metric); poseopt: Optimizer::PoseOptimization, the pose solve the reference's "
                         "TrackWithMotionModel really calls (SURVEY D1); motion_model: the whole Tracking::TrackWithMotionModel as one call; "
                         "track: motion_model followed by Tracking::TrackLocalMap over a ~1000-point local map per frame")
    args = ap.parse_args()
    env_world = os.environ.get("WORLD_SIZE")
    if env_world is None and args.gpus > 1:
        return spawn_ranks(args)
    world = int(env_world or "1")
    if world != args.gpus:
        sys.exit(f"bench.py: --gpus {args.gpus} does not match WORLD_SIZE={world} (launch one rank per GPU, or run without a launcher)")
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    global W, H, BOUNDS, CFG
    CFG = parse_pyramid(args.pyramid)
    pyr_txt = f"{CFG[2]}-level x{CFG[1]:g}"
    W, H = (int(v) for v in args.res.lower().split("x"))
    BOUNDS = (0.0, float(W), 0.0, float(H))
    B = args.batch

    # ---- scenes: generated on the host cores BEFORE anything touches the GPU (fork pool)
    nu = max(1, min(args.unique, B))
    import multiprocessing as mp
    ncpu = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else 4
    nproc = max(1, min(16 // max(1, min(world, 8)), ncpu, nu))
    # under rocprofv3 the preloaded tool library has initialised the GPU before this program starts: no forked helpers then
    profiled = "rocprof" in os.environ.get("LD_PRELOAD", "").lower() or any(k.startswith(("ROCPROF", "ROCPROFILER")) for k in os.environ)
    if nproc > 1 and not profiled:
        with mp.get_context("fork").Pool(nproc) as pool:
            scenes = make_cases(nu, 1000 + 100 * rank, W, H, pool)
    else:
        scenes = make_cases(nu, 1000 + 100 * rank, W, H)

    import torch
    dist = None
    # SD_BENCH_REHEARSAL=1: every rank on GPU 0 with gloo over host memory -- a way to run the N > 1 control flow (rank spawn,
    # shards, per-step gather, max over ranks) on a one-GPU box.  Never a measurement: the line says so.
    rehearsal = bool(os.environ.get("SD_BENCH_REHEARSAL")) and world > 1
    if rehearsal:
        local_rank = 0
    torch.cuda.set_device(local_rank)
    if world > 1:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        if rehearsal:
            dist.init_process_group("gloo", rank=rank, world_size=world)
        else:
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local_rank))
    assert torch.cuda.is_available(), "bench.py needs a GPU (no CPU fallback)"
    dev = torch.device("cuda", local_rank)

    import sdslam_amd
    from sdslam_amd import dist_util
    for ov in args.option:
        name, val = ov.split("=")
        sdslam_amd.set_option(name, int(val))
    wl = Workload(scenes, B, local_rank, args.pose_solver, args.orb_only, args.hamming, W, H, rank)
    cur, trk = wl.cur, wl.trk
    # per-frame records: written by the last tracking kernel (double-buffered), gathered from there
    rec = [torch.zeros((B, dist_util.RECORD_F64), dtype=torch.float64, device=dev) for _ in range(2)]
    gathered = [torch.zeros((B * world, dist_util.RECORD_F64), dtype=torch.float64, device=dev) for _ in range(2)] if world > 1 else None
    wl.attach_records(rec[0].data_ptr(), rec[1].data_ptr())
    stream = torch.cuda.current_stream().cuda_stream

    def full_step(k):
        if dist is not None:
            trk.stream_fence(stream, 1)          # the pack of this step must not overwrite a buffer the last gather still reads
        wl.step()
        if dist is not None and not args.orb_only:
            trk.stream_fence(stream, 0)          # the collective waits for the records
            if rehearsal:                        # gloo: host tensors (the stream fence orders the copy behind the pack kernel)
                gathered[k % 2].copy_(dist_util.all_gather_records(rec[k % 2].cpu(), torch.zeros((B * world, dist_util.RECORD_F64), dtype=torch.float64), dist))
            else:
                dist_util.all_gather_records(rec[k % 2], gathered[k % 2], dist)

    def barrier():
        torch.cuda.synchronize()
        if dist is not None:
            dist.barrier()
        torch.cuda.synchronize()

    red_dev = None if rehearsal else dev

    for k in range(args.warmup):
        full_step(k)
    cur.sync()
    if args.full:                       # per-stage HIP events on the launch streams, inside the timed region
        cur.set_profiling(True)
        trk.set_profiling(True)
    wl.k = 0
    barrier()
    t0 = time.perf_counter()
    for k in range(args.steps):
        full_step(k)                    # every step re-aligns from the predicted pose (Tprior is not overwritten)
    cur.sync()
    trk.get_tracked(0, 1)               # host-side wait for the tracking stream (its work is not on torch's streams)
    barrier()
    dt = time.perf_counter() - t0
    if args.full:
        orb_ms = cur.stage_ms()
        trk_ms = trk.stage_ms() if not args.orb_only else np.zeros(3, np.float32)
        if args.pose_solver == "track" and not args.orb_only and not args.hamming:
            trk_ms[1:] *= 2      # the timers average per call; search and PoseOptimization run twice per step here
        cur.set_profiling(False)
        trk.set_profiling(False)
    dt = dist_util.max_over_ranks(dt, dist, red_dev)                  # MAX over ranks

    last = (args.steps - 1) % 2
    # ---- check what was gathered: every rank's block of the last step equals that rank's own records
    if args.full and world > 1 and not args.orb_only:
        mine = gathered[last][rank * B:(rank + 1) * B]
        assert torch.equal(mine, rec[last]), "gathered records differ from the local ones"
    rec_host = rec[last].cpu().numpy()
    if rank == 0 and args.dump_outputs:
        dump_outputs(wl, args.dump_outputs, None if args.orb_only else rec_host,
                     gathered[last].cpu().numpy() if world > 1 and not args.orb_only else None)

    if rank == 0:
        total_frames = B * args.steps * world
        if args.orb_only:
            workload = f"ORB extract only (BASELINE configs[1] without matching), {W}x{H}, {pyr_txt}"
        elif args.hamming:
            workload = (f"BASELINE configs[1]: {W}x{H} {pyr_txt} pyramid, 1000 kp, ORB extract + brute-force Hamming match "
                        "(ORBmatcher::SearchByPoints, 1000 x 1000 per frame pair, nnratio 0.75, orientation check)")
        else:
            which = "BASELINE configs[3] at the configs[1] pyramid" if CFG[2:0:-1] == (8, 1.2) else "BASELINE configs[3] at the reference's default pyramid (src/Config.cc:48-51)"
            workload = (f"{which}: {W}x{H}, {pyr_txt}, 1000 kp; ORB extract + ImageAlign (levels 4,3,2) + "
                        "SearchByProjection + " + ("PnP RANSAC (maxIts 200; iterations actually run: tracking.mean_pnp_iterations with --full)"
                                                   if args.pose_solver == "pnp" else "Optimizer::PoseOptimization (g2o LM, 4x10 its)") +
                        (", as one Tracking::TrackWithMotionModel call" if args.pose_solver in ("motion_model", "track") else "") +
                        (" + Tracking::TrackLocalMap (th 1, <=1000 local points)" if args.pose_solver == "track" else ""))
        line = {
            "metric": "tracked frames/sec (ORB+ImageAlign+PnP) at 640x480, 1000 kp",
            "value": total_frames / dt, "unit": "frames/s", "n_gpus": world, "steps": args.steps,
            "warmup": args.warmup, "ms_per_step": dt / args.steps * 1e3, "higher_is_better": True,
            "scaling": "weak", "vs_baseline": None, "dtype": "u8", "data": "synthetic",
            "config": {"workload": workload, "pose_solver": args.pose_solver, "pyramid": args.pyramid, "options": args.option,
                       "frames_per_gpu_per_step": B, "unique_scenes": nu, "inputs": "resident in HBM", "timed_region_s": dt,
                       "pose_records": ("REHEARSAL ONLY (SD_BENCH_REHEARSAL): all ranks on one GPU, gloo over host memory -- not a measurement" if rehearsal else
                                        "all-gathered over RCCL every step inside the timed region, straight from the device buffer the "
                                        "last tracking kernel wrote") if world > 1 else "packed on the device every step (single GPU: no collective)"},
        }
        if args.full:
            full_figures(line, args, wl, scenes, rec_host, orb_ms, trk_ms, full_step)
        print(json.dumps(line, default=float))
    if dist is not None:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
