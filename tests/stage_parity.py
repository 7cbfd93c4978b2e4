"""One device-versus-oracle comparison per tracking stage, on a rig of tests/sweep_rig.py (helper, no tests).

Each driver sets the stage's inputs on the rig's tracker, runs the stage, calls the oracle on the same inputs, makes every
parity assertion, puts the rig back (sweep_rig.restore) and returns what the device gave, what the oracle said and the largest
differences.  What varies between the sweeps is an argument: G, a rigid move of the world (tests/world_frames.py; None leaves
every input the very array the rig holds), the runs of a stage's loops, and the floors under the oracle's match counts, which
depend on how many keypoints a sweep's frames have.  What only one sweep can claim (a first-principles bound on the pose, a
planted point's side of a border) it asserts itself on the returned values.

A parity assertion added here reaches every sweep; a new sweep axis calls these drivers from its own test file."""
from contextlib import nullcontext

import numpy as np

import pnp_cases as PC
import sweep_rig as SR
import world_frames as WF
from sdslam_amd import synth

POSE_TOL = 1e-5


def _poses(Ts, G):
    return Ts if G is None else [WF.move_pose(T, G) for T in Ts]


def _lasts(lasts, G):
    return lasts if G is None else [WF.move_last(l, G) for l in lasts]


def _locals(rig, G):
    return [f["local"] if G is None else WF.move_local(f["local"], G) for f in rig["fr"]]


def _uright_rows(rig, urs):
    ur = np.full((rig["B"], rig["cap"]), -1, np.float32)
    for i, u in enumerate(urs):
        ur[i, :len(u)] = u
    return ur


def image_align(oracle, rig, name, G=None, modes=((0, "last"), (1, "last"), (3, "last")), chi2=False):
    """ImageAlign from the perturbed start, for every (mode, key of the last frame it takes): ok and per-level iterations equal,
    error to a relative 1e-7, pose within 1e-5 (mode 3 leaves the pose untouched), and with `chi2` mode 0's chi2 to a relative
    1e-9."""
    trk, B, fr, K = rig["trk"], rig["B"], rig["fr"], rig["cam"].K
    T_ref, T0 = _poses(SR.refs(rig), G), _poses(SR.starts(rig), G)
    out = dict(worst=0.0, worst_error=0.0, got=[], want=[])
    try:
        for mode, which in modes:
            lasts = _lasts([f[which] for f in fr], G)
            trk.set_last(0, lasts)
            trk.set_poses(0, T_ref, T0)
            trk.align(B, mode=mode)
            g, want = trk.get_align(0, B), []
            for i in range(B):
                key = (name, mode, i)
                r = oracle.align(fr[i]["pc"], fr[i]["pr"], fr[i]["tab"]["inv_sf"], fr[i]["tab"]["sf"], lasts[i]["Xw"][lasts[i]["valid"] != 0],
                                 T_ref[i], T0[i], K, mode=mode)
                assert g["ok"][i] == r["ok"] and r["ok"], key
                assert np.array_equal(g["iters"][i][:len(r["iters"])], r["iters"]), (key, g["iters"][i][:len(r["iters"])], r["iters"])
                if mode != 3:
                    d = np.abs(g["T"][i] - r["T"]).max()
                    out["worst"] = max(out["worst"], d)
                    assert d <= POSE_TOL, (key, d)
                else:
                    assert np.abs(g["T"][i] - T0[i]).max() == 0      # pose untouched
                e = abs(g["error"][i] - r["error"]) / max(1.0, abs(r["error"]))
                out["worst_error"] = max(out["worst_error"], e)
                assert e <= 1e-7, (key, e)
                if chi2 and mode == 0:
                    assert abs(g["chi2"][i] - r["chi2"]) <= 1e-9 * max(1.0, abs(r["chi2"])), key
                want.append(r)
            out["got"].append(g)
            out["want"].append(want)
    finally:
        SR.restore(rig)
    return out


def search_by_projection(oracle, rig, name, runs, floors, G=None, depth=None):
    """SearchByProjection(Frame, Frame) for every (mono, th, match_split option or None) of `runs`: the match vector and the
    count equal the oracle's, and the oracle finds at least floors[th] matches.  From the first run that is not mono on, the
    frames carry right coordinates and bf = BF: sampled from the depth maps `depth` by stereo_from_depth (equal to the oracle's
    ComputeStereoFromRGBD, some with and some without depth), or without `depth` planted by sweep_rig.planted_cur_uright."""
    trk, B, fr, cam = rig["trk"], rig["B"], rig["fr"], rig["cam"]
    lasts = _lasts([f["last"] for f in fr], G)
    T_ref, T_cur = _poses(SR.refs(rig), G), _poses(SR.currents(rig), G)
    bf = SR.BF
    mb = np.float32(bf) / np.float32(cam.K[0])
    out = dict(total=0, got=[], want=[])
    try:
        trk.set_last(0, lasts)
        urs = None
        for mono, th, split in runs:
            if not mono and urs is None:
                trk.set_camera(*cam.K, bf, cam.bounds)
                if depth is None:
                    urs = [SR.planted_cur_uright(rig, i, bf) for i in range(B)]
                    trk.set_uright(0, _uright_rows(rig, urs))
                else:
                    trk.stereo_from_depth(depth)
                    ur, _ = trk.get_stereo(0, B)
                    urs = [oracle.stereo_from_rgbd(fr[i]["ck"], fr[i]["ck"], depth[i], bf)[0] for i in range(B)]
                    for i in range(B):
                        assert np.array_equal(ur[i, :len(urs[i])], urs[i]) and (urs[i] > 0).any() and (urs[i] == -1).any()
            trk.set_poses(0, T_ref, T_cur)
            with nullcontext() if split is None else rig["sd"].options({"track.match_split": split}):
                trk.match(B, th=th, mono=mono, check_ori=True)
            cm, nm = trk.get_matches(0, B)
            want = []
            for i in range(B):
                key = (name, mono, th, split, i)
                kw = {} if mono else dict(u_right=urs[i], mbf=bf, mb=mb)
                n, ocm = oracle.search_by_projection(fr[i]["ck"], fr[i]["cd"], fr[i]["tab"]["sf"], cam.bounds, cam.K, T_cur[i], T_ref[i], lasts[i],
                                                     th=th, mono=mono, check_ori=True, **kw)
                assert nm[i] == n, (key, nm[i], n)
                assert np.array_equal(cm[i, :len(ocm)], ocm) and (cm[i, len(ocm):] == -1).all(), key
                assert n >= floors[th], (key, n)
                out["total"] += n
                want.append((n, ocm))
            out["got"].append((cm, nm))
            out["want"].append(want)
    finally:
        SR.restore(rig)
    return out


def local_map_search(oracle, rig, name, floor, G=None, some_out_of_view=True):
    """isInFrustum, PredictScale and the search: every output equals the oracle's; the oracle matches at least `floor` points
    and, with `some_out_of_view`, some points fail isInFrustum."""
    trk, B, fr, cam = rig["trk"], rig["B"], rig["fr"], rig["cam"]
    locals_ = _locals(rig, G)
    T_ref, T_cur = _poses(SR.refs(rig), G), _poses(SR.currents(rig), G)
    out = dict(got=None, want=[])
    try:
        trk.set_poses(0, T_ref, T_cur)
        trk.set_local(0, locals_)
        trk.match_local(B, th=1.0, nnratio=0.8)
        g = out["got"] = trk.get_local(0, B)
        for i in range(B):
            n, M = len(fr[i]["ck"]), len(locals_[i]["cand"])
            r = oracle.search_local_points(fr[i]["ck"], fr[i]["cd"], fr[i]["tab"]["sf"], SR.log_sf(rig), cam.bounds, cam.K, 0.0, T_cur[i], locals_[i],
                                           th=1.0, nnratio=0.8)
            assert np.array_equal(g["in_view"][i, :M], r["in_view"]), (name, i)
            assert np.array_equal(g["proj"][i, :M], r["proj"]) and np.array_equal(g["level"][i, :M], r["level"]), (name, i)
            assert np.array_equal(g["cos"][i, :M], r["cos"]), (name, i)
            assert g["n"][i] == r["n"], (name, i, g["n"][i], r["n"])
            assert np.array_equal(g["match"][i, :n], r["match"]) and (g["match"][i, n:] == -1).all(), (name, i)
            assert r["n"] >= floor, (name, i, r["n"])
            assert not some_out_of_view or r["in_view"].sum() < M, (name, i)
            out["want"].append(r)
    finally:
        SR.restore(rig)
    return out


def features_in_area(oracle, rig, name, queries):
    """Frame::GetFeaturesInArea on the device grid for every disc of `queries` on every frame: the index lists are identical and
    in order, over 100 indices in all.  Returns their number."""
    total = 0
    for i in range(rig["B"]):
        for q in queries:
            got = rig["trk"].features_in_area(i, *q)
            want = oracle.features_in_area(rig["fr"][i]["ck"], rig["cam"].bounds, *q)
            assert np.array_equal(got, want), (name, i, q, got, want)
            total += len(want)
    assert total > 100, (name, total)
    return total


def pose_optimization(oracle, rig, name, G=None, starts=None):
    """The planted 30 %-outlier vector through set_matches, one and four waves per frame, mono and with planted uRight, from
    every (label, start poses) of `starts` (default: the perturbed start): identical flags and counts, pose within 1e-5 of the
    oracle's, no planted inlier flagged and over 95 % of the planted outliers.  got: [(key, get_pose_opt's result)] per run."""
    trk, B, fr, cam = rig["trk"], rig["B"], rig["fr"], rig["cam"]
    cases = [SR.planted_case(rig, i) for i in range(B)]
    lasts = _lasts([c[0] for c in cases], G)
    starts = [("perturbed", SR.starts(rig))] if starts is None else starts
    T_ref = _poses(SR.refs(rig), G)
    out = dict(worst=0.0, got=[], cases=cases)
    try:
        trk.set_last(0, lasts)
        for stereo in (False, True):
            ur = _uright_rows(rig, [SR.planted_uright(rig, i, *cases[i]) for i in range(B)] if stereo else [])
            if stereo:
                trk.set_camera(*cam.K, SR.BF, cam.bounds)
                trk.set_uright(0, ur)
            for start, T0 in starts:
                T0 = _poses(T0, G)
                want = []
                for i in range(B):
                    n = len(fr[i]["ck"])
                    want.append(oracle.pose_optimization(fr[i]["ck"], cases[i][1] >= 0, SR.matched_points(lasts[i], cases[i][1]),
                                                         fr[i]["tab"]["inv_sigma2"], cam.K, T0[i], u_right=ur[i, :n] if stereo else None,
                                                         bf=SR.BF if stereo else 0.0))
                for waves in (1, 4):
                    trk.set_matches(0, np.stack([c[1] for c in cases]))
                    trk.set_poses(0, T_ref, T0)
                    with rig["sd"].options({"track.poseopt_waves": waves}):
                        trk.pose_opt(B, 0)
                        g = trk.get_pose_opt(0, B)
                    for i in range(B):
                        key, r, n, (_, cm, truth) = (name, stereo, start, waves, i), want[i], len(fr[i]["ck"]), cases[i]
                        d = np.abs(g["T"][i] - r["T"]).max()
                        out["worst"] = max(out["worst"], d)
                        assert np.array_equal(g["outlier"][i, :n], r["outlier"]) and not g["outlier"][i, n:].any(), key
                        assert (g["n_inliers"][i], g["n_initial"][i], g["n_bad"][i]) == (r["n_inliers"], r["info"][0], r["info"][1]), key
                        assert d <= POSE_TOL, (key, d)
                        flagged = g["outlier"][i, :n]
                        assert not (truth & flagged).any() and flagged[(cm >= 0) & ~truth].mean() > 0.95, key
                    out["got"].append(((name, stereo, start, waves), g))
    finally:
        SR.restore(rig)
    return out


def pnp_ransac(oracle, rig, name, scenario, G=None, refined=False, ends_ok=False):
    """PnP RANSAC on the planted matches of pnp_cases.SCENARIOS[scenario] through its iterate() call sequence: after every call
    the solver's parameters, ok, iteration and inlier counts, no_more and the inlier flags equal the oracle's, the pose within
    1e-5.  `refined`: the device's refined flag is `ok and not no_more`; `ends_ok`: the oracle's last call returns a pose."""
    trk, B, fr, cam = rig["trk"], rig["B"], rig["fr"], rig["cam"]
    cases = [SR.pnp_case(rig, i, scenario) for i in range(B)]
    lasts = _lasts([c[0] for c in cases], G)
    params, calls = cases[0][3], cases[0][4]
    rs = synth.glibc_rand_stream(PC.rand_needed(params, calls))
    out = dict(worst=0.0, got=[], want=[])
    try:
        trk.set_last(0, lasts)
        trk.set_matches(0, np.stack([c[1] for c in cases]))
        trk.set_rand(0, np.tile(rs, (B, 1)))
        got = out["got"]
        for k, n_it in enumerate(calls):
            if k == 0:
                trk.pnp(B, *params, n_it)
            else:
                trk.pnp_iterate(B, n_it)
            got.append(trk.get_pnp(0, B))
        for i in range(B):
            n = len(fr[i]["ck"])
            res, pr = PC.run_oracle(oracle, fr[i]["ck"], fr[i]["tab"]["sigma2"], lasts[i], cases[i][1], params, calls, rs, K=cam.K)
            for k, r in enumerate(res):
                g, key = got[k], (name, scenario, i, k)
                assert (g["N"][i], g["min_inliers"][i], g["max_its"][i]) == (pr["N"], pr["min_inliers"], pr["max_its"]), key
                assert (bool(g["ok"][i]), int(g["iterations"][i]), int(g["n_inliers"][i]), bool(g["no_more"][i])) == \
                    (r["ok"], r["iterations"], r["n_inliers"], r["no_more"]), key
                if refined:
                    assert bool(g["refined"][i]) == (r["ok"] and not r["no_more"]), key
                assert np.array_equal(g["inliers"][i, :n], r["inliers"]), key
                d = np.abs(g["T"][i] - r["T"]).max()
                out["worst"] = max(out["worst"], d)
                assert d <= POSE_TOL, (key, d)
            if ends_ok:
                assert res[-1]["ok"], (name, scenario, i)
            out["want"].append(res)
    finally:
        SR.restore(rig)
    return out


def epnp_alone(oracle, name, K, trials, tol):
    """compute_pose through debug_epnp on every (Xw, uv, T) of `trials`: R and t within tol(T) of the oracle's.  Returns the
    largest difference and the oracle's (R, t) per trial."""
    from sdslam_amd.capi import debug_epnp
    worst, want = 0.0, []
    for trial, (Xw, uv, T) in enumerate(trials):
        R, t, e = oracle.epnp(Xw, uv, K)
        Rg, tg, eg = debug_epnp(Xw, uv, K)
        d = max(np.abs(R - Rg).max(), np.abs(t - tg).max())
        worst = max(worst, d)
        assert d <= tol(T), (name, trial, len(Xw), d, tol(T))
        want.append((R, t))
    return worst, want


def motion_model_then_local_map(oracle, rig, name, local_floor, G=None, mono=True, th_lm=1.0, sample_depth=None):
    """TrackWithMotionModel and TrackLocalMap chained on the device against the oracle's composition: status, counts, the retried
    flag, match vectors and outlier flags identical, poses within 1e-5; the oracle tracks at both stages and its local-map
    result has r[field] >= floor for local_floor = (field, floor).  RGB-D (mono False): after the camera is set with bf = BF,
    sample_depth() fills mvuRight / mvDepth on the device and returns them, and the chain ends with close_points against the
    host restatement of Tracking::NeedNewKeyFrame's counts.  T_mm: the device's poses after the motion model."""
    trk, B, fr, cam, MP = rig["trk"], rig["B"], rig["fr"], rig["cam"], rig["max_points"]
    lasts = [dict(l) for l in _lasts([f["last"] for f in fr], G)]
    for i, l in enumerate(lasts):       # a third of the last frame's points are not in the map yet
        l["obs"] = (np.arange(len(l["obs"])) % 3 != i % 3).astype(np.int32)
    locals_ = _locals(rig, G)
    T_ref, T0 = _poses(SR.refs(rig), G), _poses(SR.starts(rig), G)
    bf = 0.0 if mono else SR.BF
    mb = np.float32(bf) / np.float32(cam.K[0])
    out = dict(worst=0.0)
    try:
        trk.set_camera(*cam.K, bf, cam.bounds)
        ur = dd = None
        if not mono:
            ur, dd = sample_depth()
        trk.set_last(0, lasts)
        trk.set_local(0, locals_)
        trk.set_poses(0, T_ref, T0)
        trk.align(B, 0)             # the device's aligned poses: the matcher is compared on these
        T_al = trk.get_align(0, B)["T"]
        trk.set_poses(0, T_ref, T0)
        trk.track_with_motion_model(B, th=8.0, mono=mono, align_mode=0)
        tw, gp, (fm, nm), ga = trk.get_tracked(0, B), trk.get_pose_opt(0, B), trk.get_matches(0, B), trk.get_align(0, B)
        T_mm = out["T_mm"] = gp["T"]
        for i in range(B):
            n, key = len(fr[i]["ck"]), (name, mono, "motion model", i)
            kw = {} if mono else dict(u_right=ur[i, :n], mbf=bf, mb=mb)
            r = oracle.track_with_motion_model(fr[i]["pc"], fr[i]["pr"], fr[i]["tab"], fr[i]["ck"], fr[i]["cd"], cam.bounds, cam.K, T_ref[i], T0[i],
                                               lasts[i], 8.0, mono=mono, align_mode=0, T_aligned=T_al[i], **kw)
            assert (tw["status"][i], tw["retried"][i], tw["nmatches"][i], tw["nmatches_map"][i]) == \
                (r["status"], r["retried"], r["nmatches"], r["nmatches_map"]), key
            assert np.array_equal(fm[i, :n], r["match"]) and (fm[i, n:] == -1).all(), key
            d = np.abs(gp["T"][i] - r["T"]).max()
            out["worst"] = max(out["worst"], d)
            assert d <= POSE_TOL, (key, d)
            assert np.abs(ga["T"][i] - r["T"]).max() <= POSE_TOL and not gp["outlier"][i].any(), key
            assert r["status"] == 2, key
        trk.track_local_map(B, th=th_lm, min_inliers=30)
        g, gp, gl = trk.get_local_map(0, B), trk.get_pose_opt(0, B), trk.get_local(0, B)
        for i in range(B):
            n, key = len(fr[i]["ck"]), (name, mono, "local map", i)
            kw = {} if mono else dict(u_right=ur[i, :n], mbf=bf)
            r = oracle.track_local_map(fr[i]["ck"], fr[i]["cd"], fr[i]["tab"], SR.log_sf(rig), cam.bounds, cam.K, T_mm[i], fm[i, :n], lasts[i], locals_[i],
                                       th=th_lm, min_inliers=30, **kw)
            assert np.array_equal(gl["match"][i, :n], r["local_match"]), key
            want = np.where(r["local_match"] >= 0, r["local_match"] + MP, r["frame_match"])
            assert np.array_equal(g["match"][i, :n], want) and (g["match"][i, n:] == -1).all(), key
            assert g["n_points"][i] == r["n_points"] and g["n_local"][i] == r["n_local"], key
            assert np.array_equal(gp["outlier"][i, :n], r["outlier"]), key
            assert g["n_inliers"][i] == r["n_inliers"] and g["status"][i] == r["status"], (key, g["n_inliers"][i], r["n_inliers"])
            d = np.abs(gp["T"][i] - r["T"]).max()
            out["worst"] = max(out["worst"], d)
            assert d <= POSE_TOL, (key, d)
            assert r[local_floor[0]] >= local_floor[1] and r["status"] == 2, key
        out.update(local_map=g, pose_opt=gp)
        if not mono:
            # Tracking::NeedNewKeyFrame's close-point counts on the sampled depths: th_depth is one keypoint's depth exactly
            pos = np.sort(dd[0, :len(fr[0]["ck"])][dd[0, :len(fr[0]["ck"])] > 0])
            th = pos[len(pos) // 2]
            trk.close_points(B, 1, th)
            got = trk.get_close_points(0, B)
            for i in range(B):
                n = len(fr[i]["ck"])
                d, m, ol = dd[i, :n], g["match"][i, :n], gp["outlier"][i, :n].astype(bool)
                obs = np.where(m >= MP, locals_[i]["obs"][np.clip(m - MP, 0, len(locals_[i]["obs"]) - 1)], lasts[i]["obs"][np.clip(m, 0, len(lasts[i]["obs"]) - 1)])
                kept = (m >= 0) & (obs >= 1) & ~ol
                close = (d > 0) & (d < th)
                assert (got["tracked"][i], got["non_tracked"][i]) == ((close & kept).sum(), (close & ~kept).sum()), (name, "close points", i)
                assert got["tracked"][i] > 0 and got["non_tracked"][i] > 0, (name, "close points", i)
    finally:
        SR.restore(rig)
    return out
