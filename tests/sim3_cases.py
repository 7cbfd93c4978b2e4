"""Seeded cases for the Sim3Solver tests (tests/test_sim3_cpu.py, test_sim3_gpu.py, test_sim3_facade.py, tools/bench_sim3.py).

Keypoints (their count and octaves: all the solver reads of them) come from an extraction of synth frames -- the oracle's on
the CPU, the extractor's on the GPU, which agree bit for bit; map points, poses, flags and match vectors are built here.  One
current keyframe (the same image in every slot, so the batch serves paired and broadcast mode alike) against B candidates,
one of which is the same image.

Scene: the points of KF2 sit in a 3 x 3 x 3 m box 10 m in front of its camera, a planted similarity S12 = (s, R, t) maps them
into KF1's camera frame, and a telephoto K turns a pixel into 2.5 mm at that depth -- so an outlier (1 .. 2 m off)
misses by hundreds of pixels while the hypothesis drawn from any three correspondences stays a moderate transform that keeps
every projected point far in front of the camera (the margin condition of test_sim3_cpu.py (e)).
"""
import numpy as np

import sim3_ref as R3
from sdslam_amd import synth

W, H, NFEAT = 320, 240, 300
PYR = {"p8": (NFEAT, 1.2, 8, 20), "p5": (NFEAT, 2.0, 5, 20)}
K = (4000.0, 4000.0, 160.0, 120.0)
BOUNDS = (0.0, float(W), 0.0, float(H))
B = 10
DEPTH = 10.0
PROB, MIN_INLIERS, MAX_ITS = 0.99, 20, 300      # LoopClosing::ComputeSim3: SetRansacParameters(0.99, 20, 300)
RAND_PER_SLOT = 3 * MAX_ITS
SEED = {"p8": 11, "p5": 11}                      # (e) failed for none of these; a seed that does is replaced here

SLOTS = ["empty", "n19", "n20", "n21_exact", "n70_out30", "n250_out60_s1.7", "n70_all_out", "kf1_is_kf2", "holes_flags", "mixed_octaves"]


def images():
    cur = np.stack([synth.make_image(100, W, H)] * B)
    ref = np.stack([synth.make_image(200 + b, W, H) for b in range(B)])
    ref[SLOTS.index("kf1_is_kf2")] = cur[0]      # KF2 = KF1: here SearchByPoints matches every keypoint to itself
    return cur, ref


def oracle_keypoints(oracle, pyr):
    """-> (oct1 [B, cap], n1 [B], oct2, n2) from the oracle's extraction of images()."""
    cur, ref = images()
    e = oracle.OrbOracle(*PYR[pyr])

    def run(imgs, same):
        octs, ns, k = np.zeros((B, NFEAT), np.int32), np.zeros(B, np.int32), None
        for b in range(B):
            if k is None or not same:
                k = e.extract(imgs[b])[0]
            octs[b, :len(k)], ns[b] = k["octave"], len(k)
        return octs, ns
    return run(cur, True) + run(ref, False)


def rot(axis, deg):
    a = np.asarray(axis, float)
    a = a / np.linalg.norm(a)
    th = np.deg2rad(deg)
    Kx = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(th) * Kx + (1 - np.cos(th)) * Kx @ Kx


def pose(rng, deg=20.0, trans=2.0):
    T = np.eye(4)
    T[:3, :3] = rot(rng.normal(size=3), rng.uniform(-deg, deg))
    T[:3, 3] = rng.uniform(-trans, trans, 3)
    return T


def box_points(rng, n):
    return np.stack([rng.uniform(-1.5, 1.5, n), rng.uniform(-1.5, 1.5, n), rng.uniform(DEPTH - 1.5, DEPTH + 1.5, n)], axis=1)


def to_world(T, Xc):
    return (Xc - T[:3, 3]) @ T[:3, :3]      # R^T (Xc - t)


def make_slot(rng, kind, oct1, n1, oct2, n2, cap=NFEAT, n_override=None, out_override=None):
    """-> dict(kf1, kf2, matches12 [cap], plant=(s, R, t), planted [cap] bool, N).  n_override / out_override: another N and
    outlier fraction for the kind's layout (tools/bench_sim3.py)."""
    n1, n2 = int(n1), int(n2)
    T1, T2 = pose(rng), pose(rng)
    s = 1.7 if kind == "n250_out60_s1.7" else float(rng.uniform(0.8, 1.25))
    Rp, tp = rot(rng.normal(size=3), rng.uniform(3, 10)), rng.uniform(-0.3, 0.3, 3)
    N, out_frac = {"empty": (0, 0), "n19": (19, 0), "n20": (20, 0), "n21_exact": (21, 0), "n70_out30": (70, 0.3),
                   "n250_out60_s1.7": (min(250, n1, n2), 0.6), "n70_all_out": (70, 1.0), "kf1_is_kf2": (60, 0),
                   "holes_flags": (60, 0.4), "mixed_octaves": (64, 0.25)}[kind]
    N = N if n_override is None else min(int(n_override), n1, n2)
    out_frac = out_frac if out_override is None else out_override
    # every keypoint holds some map point; the correspondences overwrite theirs
    X1c, X2c = box_points(rng, cap), box_points(rng, cap)
    has1, has2 = np.zeros(cap, np.uint8), np.zeros(cap, np.uint8)
    has1[:n1], has2[:n2] = 1, 1
    m12 = np.full(cap, -1, np.int32)
    if kind == "mixed_octaves":
        # walk the octaves round-robin so that every threshold 9, 13, 18, ... occurs on both sides
        def spread(octs, n):
            by = [list(np.flatnonzero(octs[:n] == o)) for o in range(int(octs[:n].max()) + 1)]
            pick = []
            while len(pick) < N:
                for l in by:
                    if l and len(pick) < N:
                        pick.append(l.pop(int(rng.integers(len(l)))))
            return np.array(pick)
        i1 = np.sort(spread(oct1, n1))
        i2 = rng.permutation(spread(oct2, n2))
    else:
        i1 = np.sort(rng.choice(n1, N, replace=False))
        i2 = rng.permutation(n2)[:N]
    is_out = np.zeros(N, bool)
    is_out[rng.permutation(N)[:int(round(out_frac * N))]] = True
    if kind == "kf1_is_kf2":
        T2, i2, s, Rp, tp = T1, i1.copy(), 1.0, np.eye(3), np.zeros(3)
        X2c = X1c
    else:
        X1c[i1] = s * (X2c[i2] @ Rp.T) + tp
        d = rng.normal(size=(N, 3))
        d = d / np.linalg.norm(d, axis=1, keepdims=True) * rng.uniform(1.0, 2.0, (N, 1))
        X1c[i1[is_out]] += d[is_out]
    m12[i1] = i2
    planted = np.zeros(cap, bool)
    planted[i1[~is_out]] = True
    if kind == "holes_flags":
        # further matches whose map point is missing or bad on one side: they must not become correspondences
        free1 = np.setdiff1d(np.arange(n1), i1)
        free2 = np.setdiff1d(np.arange(n2), i2)
        e1, e2 = rng.choice(free1, 24, replace=False), rng.choice(free2, 24, replace=False)
        m12[e1] = e2
        has1[e1[:12]] = 0
        has2[e2[12:]] = 0
        # and flags cleared on keypoints nothing matches
        has1[np.setdiff1d(free1, e1)[:30]] = 0
    kf1 = dict(T=T1, Xw=to_world(T1, X1c), has_mp=has1, octave=np.asarray(oct1), n=n1)
    kf2 = dict(T=T2, Xw=(kf1["Xw"] if kind == "kf1_is_kf2" else to_world(T2, X2c)), has_mp=has2, octave=np.asarray(oct2), n=n2)
    return dict(kind=kind, kf1=kf1, kf2=kf2, matches12=m12, plant=(s, Rp, tp), planted=planted, N=N)


def make_batch(pyr, oct1, n1, oct2, n2, seed=None):
    """The B slots of the GPU test and their rand() streams ([B, RAND_PER_SLOT] int32)."""
    rng = np.random.default_rng(SEED[pyr] if seed is None else seed)
    slots = [make_slot(rng, kind, oct1[b], n1[b], oct2[b], n2[b]) for b, kind in enumerate(SLOTS)]
    rand = rng.integers(0, R3.RAND_MAX + 1, size=(B, RAND_PER_SLOT), dtype=np.int64).astype(np.int32)
    return slots, rand


def sigma2(pyr):
    return R3.level_sigma2(PYR[pyr][1], PYR[pyr][2])


def solver(slot, rand_row, pyr, fix_scale, cache=None, K=K):
    s = R3.Sim3Solver(slot["kf1"], slot["kf2"], slot["matches12"], fix_scale, K, sigma2(pyr), rand_row, cache=cache)
    s.set_ransac_parameters(PROB, MIN_INLIERS, MAX_ITS)
    return s


def reference_runs(slots, rand, pyr, fix_scale, chunk=5, K=K):
    """What the GPU test replays, on the restatement: every slot once as find(), and once as iterate(chunk) calls on ALL slots
    until each has returned a matrix or reported bNoMore at least once (a solver that has returned goes on iterating with the
    batch: its state allows it).  -> dict(find=[(result, info8, solver)], rounds=[[(result, info8, R, t, s)] per call],
    stats=[per slot: err_gap, min_z, tie, hypotheses over everything evaluated])."""
    caches = [dict() for _ in slots]
    found = []
    for b, sl in enumerate(slots):
        sv = solver(sl, rand[b], pyr, fix_scale, caches[b], K)
        res = sv.find()
        found.append((res, sv.info8(res), sv))
    solvers = [solver(sl, rand[b], pyr, fix_scale, caches[b], K) for b, sl in enumerate(slots)]
    done, rounds = [False] * len(slots), []
    while not all(done):
        row = []
        for b, sv in enumerate(solvers):
            res = sv.iterate(chunk)
            info = sv.info8(res)
            done[b] = done[b] or bool(info[0]) or bool(info[2])
            row.append((res, info, sv.best_R.copy(), sv.best_t.copy(), float(sv.best_s)))
        rounds.append(row)
    stats = []
    for b in range(len(slots)):
        a, c = found[b][2].stats, solvers[b].stats
        stats.append(dict(err_gap=min(a["err_gap"], c["err_gap"]), min_z=min(a["min_z"], c["min_z"]), tie=a["tie"] or c["tie"],
                          hypotheses=a["hypotheses"] + c["hypotheses"]))
    return dict(find=found, rounds=rounds, stats=stats)


def upload(trk, slots, rand):
    """Everything the solver reads, into slots 0 .. len(slots) - 1 of a Tracker."""
    trk.set_poses(0, [s["kf2"]["T"] for s in slots], [s["kf1"]["T"] for s in slots])
    trk.set_point_flags(0, np.stack([s["kf1"]["has_mp"] for s in slots]), np.stack([s["kf2"]["has_mp"] for s in slots]))
    trk.set_sim3_points(0, np.stack([s["kf1"]["Xw"] for s in slots]), np.stack([s["kf2"]["Xw"] for s in slots]))
    trk.set_point_matches(0, np.stack([s["matches12"] for s in slots]))
    trk.set_rand(0, rand)
