"""CPU (no GPU): tests/ba_ref.py, the numpy restatement of Optimizer::LocalBundleAdjustment, is sound, and the cases of
tests/ba_cases.py are certifiable: their decisions (accept / reject, exits, level-1 set, erase set) do not depend on the order
in which anything is summed, and every value a gate reads is off its threshold by a stated margin.  The file also measures the
noise floor the GPU tolerance is derived from, and checks that the ABI declares the four entry points."""
import os
import re
import subprocess

import numpy as np
import pytest

import ba_cases
import ba_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_ORDERS = 9
MARGIN_CHI2 = 1e-6          # |chi2 - threshold| of every classified edge, and |depth| of every classified edge
MARGIN_RHO = 1e-6           # |rho| of every trial that is not exactly 0


@pytest.fixture(scope="module")
def cases():
    return ba_cases.cases()


@pytest.fixture(scope="module")
def runs(cases):
    """case -> [(result mapped back to the case's own order) for each of the N_ORDERS orders]; order 0 is the case itself"""
    out = {}
    for name in ba_cases.RUN_CASES:
        rs = []
        for seed in range(N_ORDERS):
            q, pp, ep, cp = ba_cases.permuted(cases[name], seed)
            r = ba_ref.run(q)
            back = dict(info16=r["info16"], trace=r["trace"], T=np.empty_like(r["T"]), Xw=np.empty_like(r["Xw"]))
            back["T"][cp] = r["T"]
            back["Xw"][pp] = r["Xw"]
            for k in ("obs_erase", "level1", "chi2", "chi2_r1", "depth", "depth_r1", "stereo", "edge"):
                back[k] = np.empty_like(r[k])
                back[k][ep] = r[k]
            back["point_status"] = np.empty_like(r["point_status"])
            back["point_status"][pp] = r["point_status"]
            rs.append(back)
        out[name] = rs
    return out


def decisions(r):
    return [[[t["accept"] for t in it["trials"]] for it in rnd] for rnd in r["trace"]]


def test_jacobians_agree_with_central_differences():
    rng = np.random.default_rng(0)
    K = (458.654, 457.296, 367.215, 248.375, 47.9)
    q, t = ba_ref.se3_from_T(ba_cases.scene(2, [1], 1, 1)["poses"][0])
    X = np.array([0.4, -0.3, 4.5])
    # a measurement is irrelevant to a Jacobian; the stereo projection's float invz is not differentiable: compare the mono rows
    # of both edge types and the stereo row against the double projection
    def proj(qq, tt, XX):
        pc = ba_ref.q_rotate(qq, XX) + tt
        u = K[0] * pc[0] / pc[2] + K[2]
        return np.array([u, K[1] * pc[1] / pc[2] + K[3], u - K[4] / pc[2]])
    pc = (ba_ref.q_rotate(q, X) + t)[None]
    Jl, Jp = ba_ref.edge_jacobians(pc, ba_ref.q_to_R(q)[None], np.array([True]), K)
    h = 1e-6
    for a in range(3):
        d = np.zeros(3); d[a] = h
        num = -(proj(q, t, X + d) - proj(q, t, X - d)) / (2 * h)          # error = obs - projection
        assert np.allclose(Jl[0, :, a], num, rtol=1e-6, atol=1e-6)
    for a in range(6):
        d = np.zeros(6); d[a] = h
        qp, tp = ba_ref.se3_mul(*ba_ref.se3_exp(d), q, t)
        qm, tm = ba_ref.se3_mul(*ba_ref.se3_exp(-d), q, t)
        num = -(proj(qp, tp, X) - proj(qm, tm, X)) / (2 * h)
        assert np.allclose(Jp[0, :, a], num, rtol=1e-6, atol=1e-5)
    Jl2, Jp2 = ba_ref.edge_jacobians(pc, ba_ref.q_to_R(q)[None], np.array([False]), K)
    # the mono edge's point Jacobian is written another way in g2o (-1 / z * tmp * R): equal up to rounding
    assert np.allclose(Jl2[0, :2], Jl[0, :2], rtol=1e-13, atol=0) and (Jp2[0, :2] == Jp[0, :2]).all() and not Jl2[0, 2].any() and not Jp2[0, 2].any()


def test_exact_start_exits_on_the_first_trial(runs):
    r = runs["exact"][0]
    assert list(r["info16"][:6]) == [0, 3, 2, 40, 160, 0]
    assert list(r["info16"][6:14]) == [1, 1, ba_ref.EXIT_RHO_ZERO, 1, 1, ba_ref.EXIT_RHO_ZERO, 0, 0]
    assert r["trace"][0][0]["chi2"] == 0.0 and r["trace"][0][0]["trials"][0]["rho"] == 0.0
    assert (r["chi2"] == 0).all() and not r["obs_erase"].any()


def test_noise_free_problem_returns_to_the_truth():
    p = ba_cases.scene(21, [1, 1, 1, 2, 0], 60, 4, stereo_share=0.5, pose_noise=0.003, point_noise=0.02)
    r = ba_ref.run(p)
    free = np.flatnonzero(p["roles"] == 1)
    before = np.abs(p["poses"][free] - p["T_true"][free]).max()
    # float32 measurements: 3e-5 px of rounding at 450 px focal length and 5 m is 1e-6 of pose / position
    assert before > 1e-3 and np.abs(r["T"][free] - p["T_true"][free]).max() < 2e-6 and np.abs(r["Xw"] - p["X_true"]).max() < 2e-5
    assert r["info16"][13] == 0


def test_the_special_case_holds_what_it_promises(cases, runs):
    p, r = cases["special"], runs["special"][0]
    off = p["off"]
    assert off[1] - off[0] == 1 and off[2] - off[1] == 70                                  # one observation; two wave passes
    assert r["level1"][off[2]:off[3]].all() and r["point_status"][2] == ba_ref.POINT_OPTIMISED      # every edge of point 2 at level 1
    e4 = off[3] + 3
    assert p["kf"][e4] == 4 and r["depth_r1"][e4] < 0 and r["level1"][e4] and r["obs_erase"][e4]     # behind camera 4
    assert not (p["kf"][r["edge"]] == 5).any() and p["roles"][5] == 1                       # a local keyframe without observations
    assert (r["T"][5] == p["poses"][5]).all()
    assert (r["point_status"][[7, 19]] == ba_ref.POINT_SKIPPED).all() and (r["Xw"][[7, 19]] == p["Xw"][[7, 19]]).all()
    assert p["kf_bad"].sum() == 3 and not r["edge"][p["kf_bad"] == 1].any()
    assert r["info16"][12] >= 4


def test_rejections_and_every_exit_but_qmax_occur(runs):
    exits = {int(r[0]["info16"][k]) for r in runs.values() for k in (8, 11)}
    assert {ba_ref.EXIT_RHO_ZERO, ba_ref.EXIT_ITERATIONS, ba_ref.EXIT_NBAD} <= exits
    assert any(not a for r in runs.values() for rnd in decisions(r[0]) for it in rnd for a in it)       # a rejected trial


@pytest.mark.parametrize("name", ["noisy", "many_points", "special"])
def test_schur_agrees_with_the_dense_solve(cases, runs, name):
    a, b = runs[name][0], ba_ref.run(cases[name], solver="dense")
    assert decisions(a) == decisions(b) and (a["info16"] == b["info16"]).all()
    assert (a["obs_erase"] == b["obs_erase"]).all() and (a["level1"] == b["level1"]).all()
    assert max(np.abs(a["T"] - b["T"]).max(), np.abs(a["Xw"] - b["Xw"]).max()) <= ba_cases.NOISE_FLOOR


def test_decisions_do_not_depend_on_the_order(runs):
    for name, rs in runs.items():
        for r in rs[1:]:
            assert decisions(r) == decisions(rs[0]), name
            assert (r["info16"] == rs[0]["info16"]).all(), name
            assert (r["level1"] == rs[0]["level1"]).all() and (r["obs_erase"] == rs[0]["obs_erase"]).all(), name
            assert (r["point_status"] == rs[0]["point_status"]).all(), name


def test_every_gate_has_a_margin(runs):
    for name, rs in runs.items():
        r = rs[0]
        thr = np.where(r["stereo"], ba_ref.CHI2_STEREO, ba_ref.CHI2_MONO)
        for chi2, depth in ((r["chi2_r1"], r["depth_r1"]), (r["chi2"], r["depth"])):
            assert (np.abs(chi2 - thr)[r["edge"]] > MARGIN_CHI2).all(), name
            assert (np.abs(depth)[r["edge"]] > MARGIN_CHI2).all(), name
        for rnd in r["trace"]:
            for it in rnd:
                for t in it["trials"]:
                    assert t["rho"] == 0.0 or abs(t["rho"]) > MARGIN_RHO, (name, t)
            for a, b in zip(rnd, rnd[1:]):                      # (iniChi - currentChi) * 1e3 < iniChi, read off the next iteration's chi2
                assert abs((a["chi2"] - b["chi2"]) * 1e3 - a["chi2"]) > 1e-6 * a["chi2"], name


def test_noise_floor(runs, cases):
    """The largest deviation of poses and points between the orders, and between the two solvers: what a device that sums in
    another fixed order and factorises S in another block order may legitimately differ by."""
    floor = 0.0
    for name, rs in runs.items():
        for r in rs[1:]:
            floor = max(floor, np.abs(r["T"] - rs[0]["T"]).max(), np.abs(r["Xw"] - rs[0]["Xw"]).max())
    for name in ("noisy", "many_points", "special"):
        d = ba_ref.run(cases[name], solver="dense")
        floor = max(floor, np.abs(d["T"] - runs[name][0]["T"]).max(), np.abs(d["Xw"] - runs[name][0]["Xw"]).max())
    print(f"local BA noise floor: {floor:.3e} (recorded {ba_cases.NOISE_FLOOR:.1e}, GPU bound {ba_cases.GPU_BOUND:.3e})")
    assert 0 < floor <= ba_cases.NOISE_FLOOR
    assert ba_cases.GPU_BOUND == min(64 * ba_cases.NOISE_FLOOR, 1e-5)


def test_refusals(cases):
    for name, status in ba_cases.REFUSED.items():
        p = cases[name]
        r = ba_ref.run(p)
        assert r["status"] == status and list(r["info16"]) == [status] + [0] * 15
        assert (r["T"] == p["poses"]).all() and (r["Xw"] == p["Xw"]).all() and not r["obs_erase"].any()
    r = ba_ref.run(cases["bad_index"])
    assert r["point_status"][41] == ba_ref.POINT_BAD_INDEX and (np.delete(r["point_status"], 41) == ba_ref.POINT_SKIPPED).all()
    assert (cases["max_free"]["roles"] == 1).sum() == ba_ref.MAX_FREE_KF == (cases["too_many"]["roles"] == 1).sum() - 1


def test_the_abi_declares_the_four_functions():
    header = open(os.path.join(ROOT, "include", "sdslam_hip.h")).read()
    from sdslam_amd import capi
    for fn in ("sd_track_set_ba_keyframes", "sd_track_local_ba", "sd_track_get_local_ba", "sd_debug_local_ba"):
        assert re.search(r"\bint\s+%s\s*\(" % fn, header), fn
        assert fn in capi._SIGNATURES, fn
    m = re.search(r"#define\s+SD_BA_MAX_FREE_KF\s+(\d+)", header)
    assert m and int(m.group(1)) == ba_ref.MAX_FREE_KF >= 32
    for name, value in (("SD_BA_OK", 0), ("SD_BA_NOT_RESIDENT", 1), ("SD_BA_TOO_MANY_KF", 2), ("SD_BA_BAD_INDEX", 3),
                        ("SD_BA_POINT_SKIPPED", ba_ref.POINT_SKIPPED), ("SD_BA_POINT_OPTIMISED", ba_ref.POINT_OPTIMISED),
                        ("SD_BA_POINT_BAD_INDEX", ba_ref.POINT_BAD_INDEX)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), header), name


def test_facade_host_part_under_sanitizers(tmp_path):
    """tests/native/facade_local_ba.cc without RUN_ON_GPU: the list building of :418-460, the roles, the CSR lists, the erase
    order, SetPose and SetWorldPos of the C++ facade's Optimizer::LocalBundleAdjustment, as a stand-alone program under ASan + UBSan."""
    exe = str(tmp_path / "sd_facade_local_ba_host")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-ffp-contract=off", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "native", "facade_local_ba.cc"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert out.returncode == 0 and "facade_local_ba OK" in out.stdout, out.stdout + out.stderr
