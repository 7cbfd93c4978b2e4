"""SearchForTriangulation / ComputeF12 without a GPU: the numpy restatement tests/triangulation_ref.py against answers worked
out by hand, the proof that every case of tests/triangulation_cases.py reaches the gate it claims (the reference's own
per-gate rejection counts) and keeps a match, the seeds of the extraction test of tests/test_triangulation_gpu.py (the oracle's
keypoints are the device's), the new entry points' link / NULL-handle behaviour and the C++ facade."""
import os
import re
import subprocess

import numpy as np
import pytest

import triangulation_cases as TC
import triangulation_ref as TR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_CALLS = ["sd_track_set_uright_ref", "sd_track_set_f12", "sd_track_search_for_triangulation", "sd_track_get_triangulation_matches",
             "sd_debug_search_for_triangulation"]
F32 = np.float32


@pytest.fixture(scope="module")
def sd():
    import sdslam_amd
    from sdslam_amd import build
    build.build()
    return sdslam_amd


@pytest.fixture(scope="module")
def cases():
    return TC.cases_with_reference()


def _by_name(cases, name):
    return next((c, r) for c, r in cases if c["name"] == name)


def test_unit_cases_give_the_hand_computed_answers(cases):
    seen = 0
    for c, res in cases:
        if c["expect"] is None:
            continue
        for ori in (0, 1):
            n, m, _ = res[ori]
            want = dict(c["expect"])
            if ori and c["name"] == "unit_orientation":
                for rot in (180, 300):                       # the bins of 2 and 1 entries lose to those of 6, 5 and 4
                    for r in c["by_bin"][rot]:
                        want[r] = -1
            assert len(want) == len(c["k1"])
            assert m.tolist() == [want[i] for i in range(len(m))], (c["name"], ori)
            assert n == sum(v >= 0 for v in want.values())
            seen += 1
    assert seen == 2 * 10


def test_tie_takes_the_larger_index_and_the_gates_are_filters(cases):
    c, res = _by_name(cases, "unit_ties")
    m = res[0][1]
    d = lambda i, j: int(np.unpackbits(c["d1"][i] ^ c["d2"][j]).sum())
    assert d(0, 2) == d(0, 4) == 10 and m[0] == 4            # exact tie at the minimum: the larger idx2
    assert d(0, 5) == 3 and c["h2"][5] == 1                  # the closest one holds a map point
    assert d(1, 6) == d(1, 7) == 10 and m[1] == 6            # the larger index fails the epipolar gate
    assert d(2, 8) == 50 and m[2] == 8 and d(3, 9) == 51 and m[3] == -1
    assert c["h1"][4] == 1 and d(4, 10) == 0 and m[4] == -1
    assert d(5, 11) == 0 and c["h2"][11] == 1 and m[5] == 12


def test_ulp_case_sits_one_float_either_side_of_the_threshold(cases):
    c, res = _by_name(cases, "unit_ulp")
    assert set(c["ulp"]) == {0, 3, 7}
    for octave, (r_lo, c_lo, lo, r_hi, c_hi, hi) in c["ulp"].items():
        T = np.float64(3.84) * np.float64(c["sigma2"][octave])
        for r, cd, want in ((r_lo, c_lo, lo), (r_hi, c_hi, hi)):
            a, b, cc, den = TR.epipolar_line(c["k1"]["x"][r], c["k1"]["y"][r], c["F12"])
            assert a == 0 and cc == 0
            dsqr = F32(TR.dsqr_of(a, b, cc, den, c["k2"]["x"][cd], c["k2"]["y"][cd]))
            assert dsqr == F32(want), (octave, r)
        assert np.float64(F32(lo)) < T <= np.float64(F32(hi)) and np.nextafter(F32(lo), F32(np.inf)) == F32(hi)
        assert res[0][1][r_lo] == c_lo and res[0][1][r_hi] == -1


def test_den_zero_and_the_epipoles(cases):
    c, res = _by_name(cases, "unit_den_zero")
    for i in range(len(c["k1"])):
        assert TR.epipolar_line(c["k1"]["x"][i], c["k1"]["y"][i], c["F12"])[3] == 0
    assert res[0][0] == 0 and res[0][2]["den_zero"] == len(c["k1"]) * len(c["k2"])
    assert _by_name(cases, "unit_den_nonzero")[1][0][0] == len(c["k1"])
    c, res = _by_name(cases, "unit_far_epipole")
    assert abs(float(c["epi"][0])) > 1e30 and np.isfinite(c["epi"]).all()
    with np.errstate(over="ignore"):
        assert np.isinf(F32(c["epi"][0] - c["k2"]["x"][0]) ** 2)
    assert res[0][0] == len(c["k1"]) and res[0][2]["epipole"] == 0
    c, res = _by_name(cases, "unit_epipole")
    assert res[0][2]["epipole"] == 3
    c, _ = _by_name(cases, "shape_forward_90x200")
    assert 0 < c["epi"][0] < 640 and 0 < c["epi"][1] < 480


def test_every_case_reaches_its_gates_and_keeps_a_match(cases):
    names = [c["name"] for c, _ in cases]
    for shape in ((70, 40), (5, 600), (300, 513), (0, 50), (50, 0)):
        assert any((len(c["k1"]), len(c["k2"])) == shape for c, _ in cases), shape
    assert any(max(len(c["k1"]), len(c["k2"])) % 64 for c, _ in cases)
    assert any(int((c["h1"] == 0).sum()) > 512 for c, _ in cases)          # more rows than one pass of the workgroup
    for c, res in cases:
        n, m, counts = res[0]
        for gate in c["claims"]:
            assert counts[gate] > 0, (c["name"], gate, counts)
        empty = len(c["k1"]) == 0 or len(c["k2"]) == 0 or c["name"] in ("unit_den_zero", "unit_flags_rows", "unit_flags_cands")
        assert (n == 0) if empty else (n >= 1), (c["name"], n)
        assert n == int((m >= 0).sum())
        assert res[1][0] <= n
    claimed = {g for c, _ in cases for g in c["claims"]}
    assert claimed == set(TR.GATES) - {"accepted"}
    # the rotation check bites somewhere besides the unit case: matches spread over more than three bins
    c, res = _by_name(cases, "shape_300x513")
    bins = {TR.rot_bin(c["k1"]["angle"][i], c["k2"]["angle"][j]) for i, j in TR.pairs_of(res[0][1])}
    assert len(bins) > 3 and res[1][0] < res[0][0]
    assert "unit_orientation" in names


def test_compute_f12_is_a_fundamental_matrix():
    """x1' F12 x2 = 0 for projections of the same point, rank 2, and the float64 / longdouble variants agree to rounding."""
    rng = np.random.default_rng(4)
    for T1, T2 in (TC.SIDEWAYS, TC.FORWARD):
        F = TR.compute_f12(T1, T2, TC.K)
        Fl = TR.compute_f12_longdouble(T1, T2, TC.K)
        assert Fl.dtype == np.longdouble and np.abs(F - Fl.astype(np.float64)).max() <= 1e-12 * np.abs(F).max()
        assert np.linalg.svd(F, compute_uv=False)[2] <= 1e-12 * np.abs(F).max()
        Km = TR.camera_matrix(TC.K)
        X = np.c_[rng.uniform(-1, 1, (50, 2)), rng.uniform(2, 4, 50), np.ones(50)]
        p1, p2 = (Km @ (T1 @ X.T)[:3]).T, (Km @ (T2 @ X.T)[:3]).T
        p1, p2 = p1 / p1[:, 2:], p2 / p2[:, 2:]
        r = np.einsum("ni,ij,nj->n", p1, F, p2)
        assert np.abs(r).max() <= 1e-9 * np.abs(F).max() * 640 * 640
        # the epipole is KF1's centre seen from KF2: every epipolar line passes through it
        e = TR.epipole(T1, T2, TC.K).astype(np.float64)
        lines = p1 @ F
        dist = np.abs(lines[:, 0] * e[0] + lines[:, 1] * e[1] + lines[:, 2]) / np.hypot(lines[:, 0], lines[:, 1])
        assert dist.max() <= 1e-3 * max(1.0, np.abs(e).max())


def test_sequential_walk_equals_one_call_with_rows_removed(cases):
    """The claim behind the batched call (check_ori = 0): a row's result does not depend on the other rows."""
    c, res = _by_name(cases, "shape_300x513")
    full = res[0][1]
    rng = np.random.default_rng(8)
    h1 = c["h1"].copy()
    h1[rng.random(len(h1)) < 0.5] = 1
    c2 = dict(c, h1=h1)
    _, m = TC.reference(c2, 0)
    assert np.array_equal(m, np.where(h1 != 0, -1, full))


def test_extraction_scene_gives_enough_matches(oracle):
    """The seeds of the GPU extraction test, chosen here: the restatement finds >= 20 matches on every pair of the scene."""
    import test_triangulation_gpu as G
    tab = oracle.OrbOracle(*G.RIGS["dense"]["cfg"]).tables()
    assert np.array_equal(tab["sf"], TC.SF) and np.array_equal(tab["sigma2"], TC.SIGMA2)      # the tables the restatement is fed
    for cfg in G.RIGS.values():
        sc = G.scene(cfg, oracle)
        for b in range(G.B):
            for bc in (False, True):
                counts = {}
                n, _ = G.restate(sc, b, bc, 0, sc["F_ref"][bc][b], sc["epi_ref"][bc][b], counts=counts)
                assert n >= (20 if cfg["dense"] else 0), (cfg["name"], b, bc, n)
                if cfg["dense"] and b == 0 and not bc:           # forward motion: the epipole gate rejects something
                    assert counts["epipole"] > 0 and 0 < sc["epi_ref"][0][0][0] < G.W and 0 < sc["epi_ref"][0][0][1] < G.H
        assert (sc["n1"] > 512).all() if cfg["dense"] else (sc["n1"] < 64).all()


def test_library_exports_the_new_entry_points(sd):
    L = sd.lib()
    hdr = open(os.path.join(ROOT, "include", "sdslam_hip.h")).read()
    for name in NEW_CALLS:
        assert getattr(L, name) is not None
        assert re.search(r"\bint %s\(" % name, hdr), name
    assert L.sd_track_search_for_triangulation(None, 1, 0, 0) == 1
    assert L.sd_track_set_f12(None, 0, 1, None) == 1
    assert L.sd_track_set_uright_ref(None, 0, 1, None, 1) == 1
    assert L.sd_track_get_triangulation_matches(None, 0, 1, None, 0, None, None, None) == 1
    assert L.sd_debug_search_for_triangulation(4096, 1, *([None] * 12), 8, 0, None, None) == 3
    assert L.sd_debug_search_for_triangulation(1, 1, *([None] * 12), 8, 0, None, None) == 1


def test_capi_exposes_the_wrappers(sd):
    from sdslam_amd import capi
    for name in ("set_uright_ref", "set_f12", "search_for_triangulation", "get_triangulation_matches"):
        assert callable(getattr(capi.Tracker, name))
    assert callable(capi.debug_search_for_triangulation)


def test_cpp_triangulation_facade_compiles_and_links(sd, tmp_path):
    exe = str(tmp_path / "sd_facade_triangulation")
    libdir = os.path.dirname(sd.lib_path())
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "native", "facade_triangulation.cc"), "-o", exe,
                           "-L", libdir, "-lsdslam_hip", f"-Wl,-rpath,{libdir}"])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "facade triangulation ok" in out.stdout, (out.returncode, out.stdout, out.stderr)
