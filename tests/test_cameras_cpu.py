"""The oracle alone under the cameras of tests/cameras.py: the cases tests/test_cameras_gpu.py runs are sound (the builders
equal synth's for synth's camera; under every camera ImageAlign converges, the searches find their matches, PoseOptimization
and PnP RANSAC find the planted truth, TrackWithMotionModel tracks), and the sweep has teeth: the oracle called with each
wrong camera of cameras.mutations differs from the oracle called with the right one in something the GPU test asserts, so a
device that effectively used that wrong camera would fail there."""
import numpy as np
import pytest

import cameras as CM
import pnp_cases as PC
import sweep_rig as SR
import world_frames as WF
from sdslam_amd import synth

LOG_SF = np.log(np.float32(CM.CFG[1]))
SWEPT = [n for n in CM.NAMES if n != "synth"]


def _same(a, b):
    assert a.keys() == b.keys()
    for k in a:
        assert np.array_equal(a[k], b[k]), k


def test_builders_equal_synth_for_its_camera(oracle):
    cam = CM.CAMERAS["synth"]
    s, t = CM.make_scene(20, cam, *CM.MOTIONS[1]), synth.make_scene(20, *CM.MOTIONS[1])
    _same(s, t)
    tex = synth.make_image(5, 2 * CM.W, 2 * CM.H)
    assert np.array_equal(CM.render(tex, s["T_cur"], cam), synth.render_plane_view(tex, s["T_cur"]))
    o = oracle.OrbOracle(300, 1.2, 8, 20)
    k, d = o.extract(s["cur"])
    _same(CM.tracking_case(3, k, d, cam, max_points=200), synth.tracking_case(3, k, d, max_points=200))
    _same(CM.keyframe_case(k, d, s["T_cur"], cam, max_points=200), synth.keyframe_case(k, d, s["T_cur"], max_points=200))
    _same(CM.local_map_case(9, k, d, s["T_cur"], cam, n_extra=40), synth.local_map_case(9, k, d, s["T_cur"], n_extra=40))
    a, b = CM.planted_matches(4, k, s["T_cur"], cam, 120, 0.3, noise_px=0.5), synth.planted_matches(4, k, s["T_cur"], 120, 0.3, noise_px=0.5)
    _same(a[0], b[0])
    assert np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    assert np.array_equal(CM.backproject_on_surface(np.stack([k["x"], k["y"]], 1), cam), synth.backproject_on_surface(np.stack([k["x"], k["y"]], 1)))
    assert CM.undistorted(oracle, k, cam) is k and CM.START.tolist() == synth.se3_exp((0.003, -0.002, 0.001), (0.05, 0.02, -0.04)).tolist()


# ---- the stages, with the camera and the keypoints as arguments --------------------------------------------------------
# The inputs of a stage (last frame, local map, planted matches) always come from the rig's own camera and undistorted keypoints:
# a mutation changes only what the stage is CALLED with.  ImageAlign reads no keypoints, so `kps` does not reach it and the
# raw-keypoints mutation cannot move it.
def _align(O, rig, i, cam, kps):
    f, s = rig["fr"][i], rig["scenes"][i]
    return O.align(f["pc"], f["pr"], f["tab"]["inv_sf"], f["tab"]["sf"], f["last"]["Xw"][f["last"]["valid"] != 0], s["T_ref"], CM.START @ s["T_cur"],
                   cam.K, mode=0)


def _match(O, rig, i, cam, kps, T):
    f, s = rig["fr"][i], rig["scenes"][i]
    return O.search_by_projection(kps, f["cd"], f["tab"]["sf"], cam.bounds, cam.K, T, s["T_ref"], f["last"], th=8.0, mono=True, check_ori=True)


def _local(O, rig, i, cam, kps):
    f, s = rig["fr"][i], rig["scenes"][i]
    return O.search_local_points(kps, f["cd"], f["tab"]["sf"], LOG_SF, cam.bounds, cam.K, 0.0, s["T_cur"], f["local"], th=1.0, nnratio=0.8)


def _area(O, rig, i, cam, kps):
    return [O.features_in_area(kps, cam.bounds, *q) for q in CM.area_queries(rig["cam"])]


def _pose_opt(O, rig, i, cam, kps):
    f, s = rig["fr"][i], rig["scenes"][i]
    last, cm, truth = SR.planted_case(rig, i)
    return O.pose_optimization(kps, cm >= 0, SR.matched_points(last, cm), f["tab"]["inv_sigma2"], cam.K, CM.START @ s["T_cur"]), cm, truth


def _pnp(O, rig, i, cam, kps):
    f = rig["fr"][i]
    last, cm, truth, params, calls = SR.pnp_case(rig, i, "out30_c4")
    rs = synth.glibc_rand_stream(PC.rand_needed(params, calls))
    return PC.run_oracle(O, kps, f["tab"]["sigma2"], last, cm, params, calls, rs, K=cam.K)[0], truth


def _track(O, rig, i, cam, kps):
    f, s = rig["fr"][i], rig["scenes"][i]
    return O.track_with_motion_model(f["pc"], f["pr"], f["tab"], kps, f["cd"], cam.bounds, cam.K, s["T_ref"], CM.START @ s["T_cur"], f["last"], 8.0,
                                     mono=True, align_mode=0)


def _pose_err(T, T_true):
    return np.abs(np.asarray(T, np.float64) - T_true).max()


@pytest.mark.parametrize("name", CM.NAMES)
def test_cases_are_sound(oracle, name):
    rig = CM.oracle_rig(oracle, name)
    cam = rig["cam"]
    for i in range(rig["B"]):
        f, s = rig["fr"][i], rig["scenes"][i]
        T_true, kps = s["T_cur"], f["ck"]
        al = _align(oracle, rig, i, cam, kps)
        e0, e1 = _pose_err(CM.START @ T_true, T_true), _pose_err(al["T"], T_true)
        assert al["ok"] and e1 < e0, (name, i, al["ok"], e0, e1)
        nm, cm = _match(oracle, rig, i, cam, kps, al["T"])
        assert nm >= 150, (name, i, nm)
        lm = _local(oracle, rig, i, cam, kps)
        assert lm["n"] >= 150 and lm["in_view"].sum() < len(f["local"]["cand"]), (name, i, lm["n"])
        po, pcm, truth = _pose_opt(oracle, rig, i, cam, kps)
        assert not (truth & po["outlier"]).any() and po["outlier"][(pcm >= 0) & ~truth].mean() > 0.95, (name, i)
        WF.assert_converged(po["T"], T_true, np.eye(4), (name, i, "pose_opt"))
        res, ptruth = _pnp(oracle, rig, i, cam, kps)
        assert all(r["ok"] for r in res) and all(np.array_equal(r["inliers"], ptruth) for r in res), (name, i, [r["n_inliers"] for r in res], ptruth.sum())
        tw = _track(oracle, rig, i, cam, kps)
        assert tw["status"] == 2, (name, i, tw["status"], tw["nmatches"])
        print(f"{name} frame {i}: align {e0:.2e} -> {e1:.2e}, {nm} frame matches, {lm['n']} local matches, pose_opt error "
              f"{_pose_err(po['T'], T_true):.2e}, pnp inliers {res[0]['n_inliers']}, tracked with {tw['nmatches_map']} map matches")
        x0, x1, y0, y1 = cam.bounds
        if name == "window":
            iw, ih = np.float32(64) / np.float32(x1 - x0), np.float32(48) / np.float32(y1 - y0)
            px, py = np.round((kps["x"] - np.float32(x0)) * iw), np.round((kps["y"] - np.float32(y0)) * ih)
            outside = (px < 0) | (px >= 64) | (py < 0) | (py >= 48)
            Xc = f["local"]["Xw"] @ T_true[:3, :3].T + T_true[:3, 3]
            u, v = cam.K[0] * Xc[:, 0] / Xc[:, 2] + cam.K[2], cam.K[1] * Xc[:, 1] / Xc[:, 2] + cam.K[3]
            in_image = (Xc[:, 2] > 0) & (u >= 0) & (u < CM.W) & (v >= 0) & (v < CM.H)
            out_bounds = (u < x0) | (u > x1) | (v < y0) | (v > y1)
            print(f"window frame {i}: {outside.sum()} keypoints outside the grid, {(in_image & out_bounds).sum()} projections inside the image but "
                  "outside the bounds")
            assert outside.sum() >= 20 and (in_image & out_bounds).sum() >= 20, (i, outside.sum(), (in_image & out_bounds).sum())
        if cam.dist is not None:
            d = max(np.abs(f["ck"]["x"] - f["ck_raw"]["x"]).max(), np.abs(f["ck"]["y"] - f["ck_raw"]["y"]).max())
            assert d > 0.5 and x0 != 0 and y0 != 0, (name, d)


def _differs(O, rig, cam, raw):
    """stage -> whether the oracle with camera `cam` (and raw keypoints if `raw`) differs from the oracle with the rig's own
    camera on frame 0 in what the GPU test asserts there: a decision, a vector, or a pose by more than 1e-5."""
    i, right = 0, rig["cam"]
    f = rig["fr"][i]
    k_right, k = f["ck"], (f["ck_raw"] if raw else f["ck"])
    out = {}
    a, b = _align(O, rig, i, right, k_right), _align(O, rig, i, cam, k)
    out["align"] = a["ok"] != b["ok"] or not np.array_equal(a["iters"], b["iters"]) or _pose_err(a["T"], b["T"]) > 1e-5
    a_m, b_m = _match(O, rig, i, right, k_right, a["T"]), _match(O, rig, i, cam, k, a["T"])
    out["match"] = not np.array_equal(a_m[1], b_m[1])
    a_l, b_l = _local(O, rig, i, right, k_right), _local(O, rig, i, cam, k)
    out["match_local"] = any(not np.array_equal(a_l[key], b_l[key]) for key in ("match", "in_view", "level", "proj"))
    out["features_in_area"] = any(not np.array_equal(x, y) for x, y in zip(_area(O, rig, i, right, k_right), _area(O, rig, i, cam, k)))
    a_p, b_p = _pose_opt(O, rig, i, right, k_right)[0], _pose_opt(O, rig, i, cam, k)[0]
    out["pose_opt"] = not np.array_equal(a_p["outlier"], b_p["outlier"]) or _pose_err(a_p["T"], b_p["T"]) > 1e-5
    a_r, b_r = _pnp(O, rig, i, right, k_right)[0], _pnp(O, rig, i, cam, k)[0]
    out["pnp"] = any(x["iterations"] != y["iterations"] or not np.array_equal(x["inliers"], y["inliers"]) or _pose_err(x["T"], y["T"]) > 1e-5
                     for x, y in zip(a_r, b_r))
    a_t, b_t = _track(O, rig, i, right, k_right), _track(O, rig, i, cam, k)
    out["track"] = a_t["status"] != b_t["status"] or not np.array_equal(a_t["match"], b_t["match"]) or _pose_err(a_t["T"], b_t["T"]) > 1e-5
    return out


@pytest.mark.parametrize("name", SWEPT)
def test_every_mutation_is_detected(oracle, name):
    rig = CM.oracle_rig(oracle, name)
    muts = CM.mutations(rig["cam"])
    assert muts
    table = {label: _differs(oracle, rig, cam, raw) for label, cam, raw in muts}
    stages = list(next(iter(table.values())))
    print(f"\n{name}: mutation x stage -> differs / same")
    print(" " * 16 + " ".join(f"{s:>16}" for s in stages))
    for label, row in table.items():
        print(f"{label:>16}" + " ".join(f"{'differs' if row[s] else 'same':>16}" for s in stages))
    for label, row in table.items():
        assert any(row.values()), (name, label)


def test_every_kind_of_mutation_applies_somewhere():
    seen = {label for n in SWEPT for label, _, _ in CM.mutations(CM.CAMERAS[n])}
    assert seen == {"fx<->fy", "cx<->cy", "min->0", "invW<->invH", "raw keypoints"}
