"""CPU (no GPU): tests/gba_ref.py, the numpy restatement of Optimizer::BundleAdjustment, is sound, and the cases of tests/gba_cases.py
can be certified: their decisions do not depend on the order of the sums, and the two noise floors the GPU tests are held to are
measured here, on the restatement alone."""
import numpy as np
import pytest

import ba_ref
import gba_cases as G
import gba_ref

ORDERS = range(9)                                      # seed 0 is the identity
_RUNS = {}


def run(name, seed=0, solver="schur", **kw):
    key = (name, seed, solver, tuple(sorted(kw.items())))
    if key not in _RUNS:
        _, nit, robust = G.RUNS[name]
        q, pp, ep, cp = G.permuted(G.problem(name), seed)
        _RUNS[key] = (gba_ref.run(q, nit, robust, solver=solver, **kw), pp, cp)
    return _RUNS[key]


def decisions(out):
    return [[t["accept"] for t in it["trials"]] for it in out["trace"]]


def test_noise_free_problem_returns_to_the_truth():
    """The measurements are float32 pixels: rounded by up to 3e-5 px, which at 5 m, fx = 458 and baselines of 0.35 .. 1.4 m moves the
    minimiser's points by up to 3e-5 / 458 * 5 * (5 / 0.35) = 5e-6 along the ray, its poses by an order less.  Bounds: twice that."""
    p = G.scene(8, [2, 1, 1, 1, 2], 80, 4, pose_noise=0.003, point_noise=0.02)
    for robust in (0, 1):
        out = gba_ref.run(p, 20, robust)
        assert out["status"] == 0 and np.abs(out["T"] - p["T_true"]).max() < 1e-6 and np.abs(out["Xw"] - p["X_true"]).max() < 1e-5
        assert np.abs(p["Xw"] - p["X_true"]).max() > 1e-2                  # ... from a start four orders further off


@pytest.mark.parametrize("name", ["noisy_robust", "stereo_mix", "k33"])
def test_schur_equals_dense_equals_blocked(name):
    a = run(name)[0]
    for solver in ("dense", "blocked"):
        b = run(name, solver=solver)[0]
        assert a["info16"].tolist() == b["info16"].tolist() and decisions(a) == decisions(b)
        assert max(np.abs(a["T"] - b["T"]).max(), np.abs(a["Xw"] - b["Xw"]).max()) <= G.NOISE_FLOOR


@pytest.mark.parametrize("n", [n for n in G.SOLVER_SIZES if n <= 390])
def test_blocked_ldlt_equals_ldlt_solve_equals_numpy(n):
    A, b = G.spd(n, n)
    (ok1, x1), (ok2, x2), x3 = ba_ref.ldlt_solve(A, b), gba_ref.blocked_ldlt_solve(A, b), np.linalg.solve(A, b)
    assert ok1 and ok2
    assert max(np.abs(x1 - x2).max(), np.abs(x1 - x3).max(), np.abs(x2 - x3).max()) / np.abs(x1).max() <= G.SOLVER_FLOOR


def test_noise_floor_of_the_solver():
    """Floor (b): measured over every size the GPU test uses; gba_cases.SOLVER_FLOOR is this figure rounded up"""
    worst = 0.0
    for n in G.SOLVER_SIZES:
        A, b = G.spd(n, n)
        xs = [ba_ref.ldlt_solve(A, b)[1], np.linalg.solve(A, b), gba_ref.blocked_ldlt_solve(A, b)[1]]
        worst = max(worst, max(np.abs(x - xs[0]).max() for x in xs) / np.abs(xs[0]).max())
    print(f"solver floor {worst:.3e} (SOLVER_FLOOR {G.SOLVER_FLOOR:.1e})")
    assert worst <= G.SOLVER_FLOOR <= 4 * max(worst, 1e-16)


@pytest.mark.parametrize("panel", [0, 1])
def test_zero_pivot_matrices(panel):
    A, b, at = G.zero_pivot(panel)
    assert at // gba_ref.PANEL == panel and np.array_equal(A, A.T)
    assert ba_ref.ldlt_solve(A, b) == (False, None) and gba_ref.blocked_ldlt_solve(A, b) == (False, None)
    assert ba_ref.ldlt_solve(A[:at, :at], b[:at])[0] and gba_ref.blocked_ldlt_solve(A[:at, :at], b[:at])[0]


@pytest.mark.parametrize("name", list(G.RUNS))
def test_decisions_hold_under_every_order(name):
    base = run(name)[0]
    assert base["status"] == 0
    for it in base["trace"]:
        for t in it["trials"]:
            assert t["rho"] == 0 or abs(t["rho"]) > 1e-6, (name, t["rho"])            # no gate reads a rho it could flip
    for seed in ORDERS:
        out = run(name, seed)[0]
        assert decisions(out) == decisions(base) and out["info16"].tolist() == base["info16"].tolist(), (name, seed)


def test_noise_floor_of_the_whole_problem():
    """Floor (a): the orders and the three solvers of every run case; gba_cases.NOISE_FLOOR is this figure rounded up"""
    worst = 0.0
    for name in G.RUNS:
        base = run(name)[0]
        for seed in ORDERS:
            out, pp, cp = run(name, seed)
            worst = max(worst, np.abs(out["T"] - base["T"][cp]).max(), np.abs(out["Xw"] - base["Xw"][pp]).max())
        for solver in ("dense", "blocked"):
            out = run(name, solver=solver)[0]
            worst = max(worst, np.abs(out["T"] - base["T"]).max(), np.abs(out["Xw"] - base["Xw"]).max())
    print(f"noise floor {worst:.3e} (NOISE_FLOOR {G.NOISE_FLOOR:.1e}, GPU bound {G.GPU_BOUND:.1e})")
    assert worst <= G.NOISE_FLOOR <= 4 * worst


def test_refusals():
    for name, (_, status) in G.REFUSED.items():
        out = gba_ref.run(G.problem(name), 10, 1)
        assert out["status"] == status and out["info16"].tolist() == [status] + [0] * 15, name
        assert np.array_equal(out["T"], G.problem(name)["poses"]) and np.array_equal(out["Xw"], G.problem(name)["Xw"])


def test_special_points():
    p, out = G.problem("special_points"), run("special_points")[0]
    assert out["point_status"][:4].tolist() == [0, 0, 0, 1]
    assert np.array_equal(out["Xw"][:3], p["Xw"][:3]) and np.array_equal(out["T"][4], p["poses"][4]) and not np.array_equal(out["T"][0], p["poses"][0])


def test_rejects_case_takes_rejected_trials_on_the_blocked_path():
    out = run("rejects36")[0]
    assert out["info16"][1] > gba_ref.LDS_FREE_KF and out["info16"][7] > out["info16"][6]
    assert [t["accept"] for t in out["trace"][2]["trials"]] == [False] * 4 + [True]


def test_robust_switch_changes_the_run():
    a, b = run("noisy_robust")[0], run("noisy_plain")[0]
    assert [it["chi2"] for it in a["trace"]] != [it["chi2"] for it in b["trace"]]
    assert a["trace"][0]["chi2"] < b["trace"][0]["chi2"]                     # Huber caps the planted outliers' terms
    assert np.abs(a["T"] - b["T"]).max() > G.GPU_BOUND


def test_first_local_round_is_a_global_run_of_five_robust_iterations():
    """On roles 1 and 2 alone the two callers of ba_ref.levenberg hand it the same graph: local BA's first round (5 iterations, robust,
    every edge on level 0) is BundleAdjustment(5, bRobust) with local BA's sqrt(5.991), step for step and bit for bit."""
    p = G.scene(11, [1, 1, 1, 1, 2, 2], 40, 4, stereo_share=0.3, pix_noise=0.4, pose_noise=0.003, point_noise=0.02)
    g, l = gba_ref.run(p, 5, 1, delta_mono=ba_ref.DELTA_MONO), ba_ref.run(p)
    assert g["status"] == 0 and l["status"] == 0 and len(g["trace"]) == 5 and (~(p["ur"] < 0)).any()
    assert g["trace"] == l["trace"][0]
    assert g["info16"][6:9].tolist() == l["info16"][6:9].tolist()


def test_huber_delta_pins_the_sic_constant():
    """thHuber2D = sqrt(5.99) (Optimizer.cc:87), not local BA's sqrt(5.991): the case tells them apart above the GPU bound"""
    a = run("huber_delta")[0]
    b = run("huber_delta", delta_mono=ba_ref.DELTA_MONO)[0]
    move = max(np.abs(a["T"] - b["T"]).max(), np.abs(a["Xw"] - b["Xw"]).max())
    print(f"sqrt(5.99) against sqrt(5.991): {move:.3e} (GPU bound {G.GPU_BOUND:.1e})")
    assert move > G.GPU_BOUND
