"""Sim3Solver without a GPU: the numpy restatement tests/sim3_ref.py against independent facts, the margin condition that
makes the committed cases of tests/sim3_cases.py decidable on any correct implementation, and the new entry points' link /
NULL-handle behaviour."""
import os
import re

import numpy as np
import pytest

import sim3_cases as SC
import sim3_ref as R3

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_CALLS = ["sd_track_set_sim3_points", "sd_track_set_point_matches", "sd_track_sim3", "sd_track_sim3_iterate", "sd_track_get_sim3"]
F32_EPS = float(np.finfo(np.float32).eps)


@pytest.fixture(scope="module")
def sd():
    import sdslam_amd
    from sdslam_amd import build
    build.build()
    return sdslam_amd


def test_jacobi_matches_eigh():
    """(a) cv::eigen restated: eigenvalues descending, eigenvectors (rows) up to sign, within float precision of LAPACK's."""
    rng = np.random.default_rng(1)
    for trial in range(40):
        A = rng.normal(size=(4, 4)) * 10.0 ** rng.integers(-2, 3)
        A = ((A + A.T) / 2).astype(np.float32)
        W, V = R3.jacobi_eigen(A)
        w, v = np.linalg.eigh(A.astype(np.float64))
        w, v = w[::-1], v[:, ::-1].T
        scale = float(np.abs(w).max())
        assert (np.diff(W) <= 0).all()
        assert np.abs(W - w).max() <= 16 * F32_EPS * scale, trial
        # an eigenvector is defined to (rounding) / (gap to the next eigenvalue)
        for i in range(4):
            gap = min(abs(w[i] - w[j]) for j in range(4) if j != i)
            tol = 32 * F32_EPS * scale / gap
            assert min(np.abs(V[i] - v[i]).max(), np.abs(V[i] + v[i]).max()) <= tol, (trial, i)
        assert np.abs(V.astype(np.float64) @ V.T.astype(np.float64) - np.eye(4)).max() <= 16 * F32_EPS


@pytest.mark.parametrize("fix_scale", [False, True])
def test_three_points_recover_the_plant(fix_scale):
    """(b) exact data: any three non-collinear correspondences give back (s, R, t) to float precision (R passes through a
    CV_32F matrix, coordinates are of order 10: 1e-5)."""
    rng = np.random.default_rng(2)
    for trial in range(30):
        s = 1.0 if fix_scale else float(rng.uniform(0.5, 2.0))
        Rp, tp = SC.rot(rng.normal(size=3), rng.uniform(-170, 170)), rng.uniform(-3, 3, 3)
        # the float Jacobi leaves the quaternion good to (rounding of N) / (gap between its two largest eigenvalues) -- the
        # bound test (a) uses -- and R is quadratic in the quaternion: dR <= 4 dq, plus its own rounding to CV_32F.  A thin
        # triangle closes that gap (collinear points leave the rotation about their line free): those are drawn again.
        while True:
            X2 = SC.box_points(rng, 3)
            X1 = s * (X2 @ Rp.T) + tp
            Pr1, Pr2 = (X1 - X1.mean(0)).T, (X2 - X2.mean(0)).T
            M = Pr2 @ Pr1.T
            N = np.array([[M[0, 0] + M[1, 1] + M[2, 2], M[1, 2] - M[2, 1], M[2, 0] - M[0, 2], M[0, 1] - M[1, 0]],
                          [0, M[0, 0] - M[1, 1] - M[2, 2], M[0, 1] + M[1, 0], M[2, 0] + M[0, 2]],
                          [0, 0, -M[0, 0] + M[1, 1] - M[2, 2], M[1, 2] + M[2, 1]],
                          [0, 0, 0, -M[0, 0] - M[1, 1] + M[2, 2]]])
            w = np.linalg.eigvalsh(N + np.triu(N, 1).T)
            tol = 4 * 32 * F32_EPS * np.abs(w).max() / (w[3] - w[2]) + 2 * F32_EPS
            if tol < 1e-4:
                break
        R, sc, t, T12, T21 = R3.compute_sim3(X1.T.copy(), X2.T.copy(), fix_scale)
        assert np.abs(R - Rp).max() <= tol, trial
        assert abs(float(sc) - s) <= (4 * tol + F32_EPS) * s       # nom / den moves with R; ms12i is a float
        assert np.abs(t - tp).max() <= 2 * tol * s * (SC.DEPTH + 3)   # t = O1 - s R O2, |O2| <= depth + box
        # T21 is built from the same R, s, t in double; what is left is the CV_32F rounding of R (R R^T - I), times |t| in the last column
        assert np.abs(T12 @ T21 - np.eye(4)).max() <= 8 * F32_EPS * (1 + np.abs(t).max())


@pytest.fixture(scope="module")
def runs(oracle):
    """pyr -> (slots, rand, {fix_scale: reference_runs}) for the committed cases."""
    out = {}
    for pyr in SC.PYR:
        slots, rand = SC.make_batch(pyr, *SC.oracle_keypoints(oracle, pyr))
        out[pyr] = (slots, rand, {fix: SC.reference_runs(slots, rand, pyr, fix) for fix in (0, 1)})
    return out


@pytest.mark.parametrize("pyr", list(SC.PYR))
def test_planted_outliers(runs, pyr):
    """(c) with free scale every slot that holds more than minInliers planted inliers returns exactly the planted set and the
    planted transform; the table's other slots end the way their row says."""
    slots, rand, by_fix = runs[pyr]
    find = by_fix[0]["find"]
    for b, sl in enumerate(slots):
        (T12, no_more, inl, n), info, sv = find[b]
        n_planted = int(sl["planted"].sum())
        if sl["kind"] in ("n21_exact", "n70_out30", "n250_out60_s1.7", "holes_flags", "mixed_octaves"):
            s, Rp, tp = sl["plant"]
            assert n == n_planted > SC.MIN_INLIERS and np.array_equal(inl, sl["planted"]) and not no_more, sl["kind"]
            assert np.abs(T12[:3, :3] - s * Rp).max() < 1e-5 and np.abs(T12[:3, 3] - tp).max() < 1e-4, sl["kind"]
            assert abs(float(sv.best_s) - s) < 1e-5 * s
        else:
            assert n == 0 and not T12.any() and not inl.any() and no_more, sl["kind"]
        assert sv.N == sl["N"]
    kinds = {sl["kind"]: find[b] for b, sl in enumerate(slots)}
    assert list(kinds["empty"][1]) == [0, 0, 1, 0, 0, 1, 0, 0]
    assert list(kinds["n19"][1]) == [0, 0, 1, 0, 19, 1, 0, 0]                       # bNoMore at once, no draw
    assert kinds["n19"][2].rpos == 0
    assert list(kinds["n20"][1]) == [0, 0, 1, 1, 20, 1, 20, 0]                      # maxIts = 1; 20 inliers are not > 20
    assert kinds["n70_all_out"][1][3] == kinds["n70_all_out"][1][5] == 196 and kinds["n70_all_out"][1][6] < SC.MIN_INLIERS
    assert kinds["kf1_is_kf2"][1][6] == 0 and np.isnan(kinds["kf1_is_kf2"][2].best_R).all()   # the NaN hypothesis
    # thresholds: the size_t truncation (1.44f * 9.21 = 13.26 -> 13) and every level present in the mixed slot
    # (the 320 x 240 frames leave the 5 x 2.0 pyramid's two smallest levels without keypoints)
    mixed = slots[SC.SLOTS.index("mixed_octaves")]["kf1"]
    levels = sorted(set(mixed["octave"][:mixed["n"]].tolist()))
    thr = sorted(set(kinds["mixed_octaves"][2].max_err1.tolist()))
    assert thr == [float(int(9.210 * float(SC.sigma2(pyr)[o]))) for o in levels] and len(levels) >= 3
    assert pyr != "p8" or (len(levels) == 8 and thr[:3] == [9.0, 13.0, 19.0])


def test_random_reproduces_the_reference_golden():
    """(d)"""
    from sdslam_amd.synth import glibc_rand_stream
    g = np.load(os.path.join(ROOT, "tests", "golden", "ref_random_srand1.npz"))
    mn, sizes, values = int(g["min"]), g["sizes"], g["values"]
    rs = glibc_rand_stream(len(sizes))
    assert [R3.random_int(r, mn, mn + d - 1) for r, d in zip(rs.tolist(), sizes.tolist())] == values.tolist()


@pytest.mark.parametrize("pyr", list(SC.PYR))
def test_margin_condition(runs, pyr):
    """(e) for every hypothesis the restatement evaluates on the committed cases (find() and the chunked replay, both scale
    modes): no err1 / err2 within a relative 1e-3 of its threshold, no projected |z| below 1e-3 of the scene depth, no tied
    pivot choice in the float Jacobi.  A seed that fails is replaced in sim3_cases.SEED."""
    slots, rand, by_fix = runs[pyr]
    total = 0
    for fix in (0, 1):
        for b, st in enumerate(by_fix[fix]["stats"]):
            assert st["err_gap"] >= 1e-3, (fix, slots[b]["kind"], st)
            assert st["min_z"] >= 1e-3 * SC.DEPTH, (fix, slots[b]["kind"], st)
            assert not st["tie"], (fix, slots[b]["kind"])
            total += st["hypotheses"]
    assert total > 1000          # the condition was checked on something


def test_max_its_table():
    assert [R3.ransac_max_its(N, 0.99, 20, 300) for N in (0, 5, 19, 20, 21, 70, 250, 2048)] == [1, 1, 1, 1, 3, 196, 300, 300]
    assert R3.ransac_max_its(40, 0.99, 20, 300) == 35 and R3.ransac_max_its(40, 0.99, 20, 10) == 10


def test_new_calls_are_declared_exported_and_mirrored(sd):
    """(f) header, library and ctypes mirror name the same five calls."""
    hdr = open(os.path.join(ROOT, "include", "sdslam_hip.h")).read()
    L = sd.lib()
    for name in NEW_CALLS:
        assert re.search(rf"^int {name}\(sd_track\* h,", hdr, re.M), name
        assert hasattr(L, name), name
        assert callable(getattr(sd.Tracker, name[len("sd_track_"):])), name


def test_new_calls_refuse_a_null_handle(sd):
    L = sd.lib()
    protos = {"sd_track_set_sim3_points": (None, 0, 1, None, None, 1),
              "sd_track_set_point_matches": (None, 0, 1, None, 1),
              "sd_track_sim3": (None, 1, 0, 0.99, 20, 300, 5),
              "sd_track_sim3_iterate": (None, 1, 5),
              "sd_track_get_sim3": (None, 0, 1, None, None, None, None, None, 0, None)}
    assert set(protos) == set(NEW_CALLS)
    for name, args in protos.items():
        assert getattr(L, name)(*args) == 1, name
