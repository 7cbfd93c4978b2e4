"""ORBmatcher::Fuse without a GPU: the numpy restatement tests/fuse_ref.py against answers worked out by hand, the proof that
every case of tests/fuse_cases.py reaches the gate it claims (per-gate rejection counts) and keeps a match, the reference's
sequential loops against "search everything first, then walk in order" on a toy map, the seeds of the extraction test of
tests/test_fuse_gpu.py (the oracle's keypoints are the device's), the window statistics behind the kernel's lanes-per-point,
the new entry points' link / NULL-handle behaviour, the C++ facade and the LDS layout under sanitizers."""
import os
import re
import subprocess

import numpy as np
import pytest

import fuse_cases as FC
import fuse_ref as FR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_CALLS = ["sd_track_set_fuse_scw", "sd_track_fuse", "sd_track_get_fuse", "sd_debug_fuse"]


@pytest.fixture(scope="module")
def sd():
    import sdslam_amd
    from sdslam_amd import build
    build.build()
    return sdslam_amd


@pytest.fixture(scope="module")
def cases():
    return FC.cases_with_reference()


def _by_name(cases, name):
    return next((c, r) for c, r in cases if c["name"] == name)


def test_unit_cases_give_the_hand_computed_answers(cases):
    seen = 0
    for c, res in cases:
        if c["expect"] is None:
            continue
        for sim3, want in ((0, c["expect"]), (1, c["expect_sim3"])):
            bi, bd = res[sim3][0], res[sim3][1]
            assert bi.tolist() == [want[i] for i in range(len(bi))], (c["name"], sim3)
            assert all((d <= FC.TH_LOW) == (i >= 0) for i, d in zip(bi, bd))
            seen += 1
    assert seen == 2 * 6


def test_hand_checked_details(cases):
    c, res = _by_name(cases, "unit_th_low_and_ties")
    bi, bd = res[0][0], res[0][1]
    assert bd[0] == 50 and bi[0] >= 0 and bd[1] == 51 and bi[1] == -1
    t = c["ties"]
    assert t["early"] > t["late"] and bi[2] == t["early"] and bd[2] == 3            # two cells: the LARGER index, walked first
    assert t["first"] < t["second"] and bi[3] == t["first"] and bd[3] == 2         # one cell: ascending index
    assert bd[4] == 1                                                               # a strictly smaller distance later in the order
    c, res = _by_name(cases, "unit_image_edges")
    assert res[0][0][0] == -1 and res[0][0][2] >= 0                                 # u == mnMaxX is outside, u == mnMinX inside
    assert res[0][2]["image"] == 4 and c["outside"] not in res[0][0].tolist()       # the keypoint at x = 637 is in no cell
    c, res = _by_name(cases, "unit_chi_square")
    assert res[0][2]["chi2"] == 3 and res[1][2]["chi2"] == 0 and (res[1][0] >= 0).all()
    assert c["uright"][4] == 0.0 and res[0][0][4] == 4 and c["uright"][5] == -1.0 and res[0][0][5] == -1   # mvuRight == 0 is stereo
    c, res = _by_name(cases, "shape_sim3_small_scale")
    R, t, Ow = FR.decompose(res[1][3], True)
    assert abs(np.linalg.det(R) - 1) < 1e-6 and np.allclose(Ow, -c["T"][:3, :3].T @ c["T"][:3, 3], atol=1e-6)


def test_every_case_reaches_its_gates_and_keeps_a_match(cases):
    for shape in ((0, 30), (1, 30), (63, 40), (64, 40), (65, 40), (80, 0), (80, 1), (300, FC.POINTS_PER_PASS + 1), (2048, 2048)):
        assert any((len(c["kps"]), len(c["pts"]["cand"])) == shape for c, _ in cases), shape
    assert any(c["kp_cap"] and c["kp_cap"] % 64 and c["max_points"] % 64 for c, _ in cases)
    c, _ = _by_name(cases, "shape_crowded_cell")
    grid, _, _ = FR.build_grid(c["kps"], c["cam"])
    assert max(len(v) for v in grid.values()) > 8                                   # more entries in one cell than a group has lanes
    c, res = _by_name(cases, "shape_all_cells")
    assert FC.SF[0] * c["th"] > 640 and res[0][2]["level"] + res[0][2]["chi2"] > 1000
    assert any(((c["kps"]["x"] >= 635) | (c["kps"]["y"] >= 475)).any() for c, _ in cases)          # keypoints outside the grid
    claimed = set()
    for c, res in cases:
        for sim3 in (0, 1):
            bi, bd, counts, _ = res[sim3]
            for gate in c["claims"]:
                assert counts[gate] > 0 or (sim3 and gate == "chi2"), (c["name"], gate, counts)
            empty = len(c["kps"]) == 0 or len(bi) <= 1
            assert (bi >= 0).sum() == counts["accepted"] and ((bi >= 0).sum() >= 1 or empty), (c["name"], sim3)
        claimed |= set(c["claims"])
    assert claimed == set(FR.GATES) - {"accepted"}


# ------------------------------------------------------------------------------------------------ the walk
def _scenario():
    """Two target keyframes A, B and six list points; best[kf][i] as the (pure) search returns it.
      p0, p1 -> A:3 (free): p0 is added, p1 then finds p0 there and one replaces the other      (same free keypoint)
      p1 -> B:1: after A, p1 or p0 is bad and is skipped in B although its search found a keypoint (replaced before a later keyframe)
      p2 -> A:5 held by p4, which is LATER in the list and has more observations: p2 is replaced by p4 (pMPinKF later in the list)
      p5 -> A:6 held by foreign q, also seen in B at 7, fewer observations: q.Replace(p5) hands p5 the observation in B, so p5
            is skipped in B although it was a candidate there at upload time                       (gains IsInKeyFrame midway)
      p3 -> B:2 (free), p4 -> B:4 (free): plain additions, p4 after having absorbed p2"""
    A, Bk, X, Y = FR.KeyFrame("kfA", 8), FR.KeyFrame("kfB", 8), FR.KeyFrame("x", 8), FR.KeyFrame("y", 8)
    pts = [FR.MapPoint("p%d" % i) for i in range(6)] + [None]
    q = FR.MapPoint("q")
    for i, p in enumerate(pts[:6]):
        p.AddObservation(X, i)
        X.points[i] = p
    pts[4].AddObservation(A, 5); A.points[5] = pts[4]
    pts[4].AddObservation(Y, 0); Y.points[0] = pts[4]
    pts[5].AddObservation(Y, 1); Y.points[1] = pts[5]
    q.AddObservation(A, 6); A.points[6] = q
    q.AddObservation(Bk, 7); Bk.points[7] = q
    best = {"kfA": {0: 3, 1: 3, 2: 5, 3: -1, 4: 2, 5: 6}, "kfB": {0: -1, 1: 1, 2: 0, 3: 2, 4: 4, 5: 6}}
    return [A, Bk], pts, (lambda kf, i: best[kf.name][i]), q


def test_sequential_loop_equals_batched_search_and_walk():
    kfs_a, pts_a, search, q_a = _scenario()
    want = FR.fuse_sequential(kfs_a, pts_a, search)
    kfs_b, pts_b, search_b, _ = _scenario()
    got = FR.fuse_batched_walk(kfs_b, pts_b, search_b)
    assert got == want == [4, 2]
    assert FR.map_state(kfs_a, pts_a) == FR.map_state(kfs_b, pts_b)
    A, Bk = kfs_a
    p = pts_a
    assert p[0].bad != p[1].bad and A.points[3] in (p[0], p[1])                   # two points, one free keypoint
    assert p[2].bad and p[2].replaced is p[4] and A.points[5] is p[4]             # replaced by a point later in the list
    assert q_a.bad and q_a.replaced is p[5] and Bk.points[7] is p[5] and A.points[6] is p[5]
    assert Bk.points[6] is None                                                   # p5 was in B by then: its search result was not applied
    assert Bk.points[1] is None or not p[1].bad                                   # a bad p1 was not added to B
    assert Bk.points[2] is p[3] and Bk.points[4] is p[4] and Bk.points[0] is None  # p2 (bad) never reached B:0


def test_walk_equals_sequential_on_random_maps():
    """The same claim on 300 random toy maps: keyframes that already hold list points and foreign ones, random search tables."""
    events = 0
    for seed in range(300):
        def make():
            rng = np.random.default_rng(seed)
            kfs = [FR.KeyFrame("kf%d" % k, 6) for k in range(3)]
            pts = [None if rng.random() < 0.1 else FR.MapPoint("p%d" % i) for i in range(8)]
            others = [FR.MapPoint("q%d" % i) for i in range(4)]
            for p in [x for x in pts if x is not None] + others:
                for kf in kfs + [FR.KeyFrame("o%d" % j, 1) for j in range(int(rng.integers(0, 3)))]:
                    idx = int(rng.integers(0, len(kf.points)))
                    if rng.random() < 0.25 and kf.points[idx] is None and not p.IsInKeyFrame(kf):
                        p.AddObservation(kf, idx)
                        kf.points[idx] = p
            table = rng.integers(-1, 6, (3, 8))
            return kfs, pts, (lambda kf, i: int(table[int(kf.name[2:]), i]))
        a, b = make(), make()
        assert FR.fuse_sequential(*a) == FR.fuse_batched_walk(*b)
        assert FR.map_state(a[0], a[1]) == FR.map_state(b[0], b[1])
        events += sum(p is not None and p.bad for p in a[1])
    assert events > 100


# ------------------------------------------------------------------------------------------------ the extraction scenes
def test_extraction_scenes_fuse_enough_points(oracle):
    """The configurations of the GPU extraction test, checked here with the oracle's keypoints: every one, on both rigs, fuses >= 20
    points per slot, the gates all fire somewhere, and the toy-map walk has something to skip."""
    import test_fuse_gpu as G
    tab = oracle.OrbOracle(*G.RIGS["dense"]["cfg"]).tables()
    assert np.array_equal(tab["sf"], FC.SF) and np.array_equal(tab["inv_sigma2"], FC.INV_SIGMA2)   # the tables the restatement is fed
    fired = {g: 0 for g in FR.GATES}
    for cfg in G.RIGS.values():
        sc = G.scene(cfg, oracle)
        low = 10 ** 9
        assert sc["M"] % 64 and sc["cap"] <= 2048
        for conf in G.CONFIGS:
            for f in range(G.B):
                counts = {}
                bi, _ = G.restate(sc, conf, f, counts=counts)
                low = min(low, int((bi >= 0).sum()))
                assert (bi >= 0).sum() >= G.MIN_FUSED, (cfg["name"], conf, f, int((bi >= 0).sum()))
                for g in fired:
                    fired[g] += counts[g]
        print("fewest fused points over the configurations and slots of the %s rig: %d" % (cfg["name"], low))
        if cfg["dense"]:
            kfs, pts = G.toy_map(sc)
            want = FR.fuse_sequential(kfs, pts, G.toy_search(sc))
            assert sum(want) >= 20 and sum(p is not None and p.bad for p in pts) > 0
            # lanes per point (FUSE_GL): grid entries per window column, the run a group walks at a time
            runs = FR.window_run_counts(sc["k2"][0, :sc["n2"][0]], sc["rows"][0], G.TG.T_REF[0], G.CAM9, FC.SF, FC.SCALE)
            print("window column runs: n %d mean %.2f median %d p90 %d p99 %d max %d"
                  % (len(runs), runs.mean(), np.median(runs), np.percentile(runs, 90), np.percentile(runs, 99), runs.max()))
            assert len(runs) > 1000                              # a measurement for the design notes, not a gate
    assert all(fired[g] > 0 for g in FR.GATES), fired


# ------------------------------------------------------------------------------------------------ link, facade, LDS
def test_library_exports_the_new_entry_points(sd):
    L = sd.lib()
    hdr = open(os.path.join(ROOT, "include", "sdslam_hip.h")).read()
    for name in NEW_CALLS:
        assert getattr(L, name) is not None
        assert re.search(r"\bint %s\(" % name, hdr), name
    assert L.sd_track_fuse(None, 1, 0, -1, 3.0, 0) == 1 and b"NULL" in L.sd_last_error()
    assert L.sd_track_set_fuse_scw(None, 0, 1, None) == 1
    assert L.sd_track_get_fuse(None, 0, 1, None, None, 0, None) == 1
    args = [None] * 3 + [1] + [None] * 8 + [0] + [None] * 3 + [8, 1.2, 3.0]
    assert L.sd_debug_fuse(1, *args, 4096, 8, None, None, None, None) == 3
    assert L.sd_debug_fuse(1, *args, 8, 8, None, None, None, None) == 1


def test_capi_exposes_the_wrappers(sd):
    from sdslam_amd import capi
    for name in ("set_fuse_scw", "fuse", "get_fuse", "fuse_pose"):
        assert callable(getattr(capi.Tracker, name))
    assert callable(capi.debug_fuse)


def test_cpp_fuse_facade_compiles_and_links(sd, tmp_path):
    exe = str(tmp_path / "sd_facade_fuse")
    libdir = os.path.dirname(sd.lib_path())
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "native", "facade_fuse.cc"), "-o", exe,
                           "-L", libdir, "-lsdslam_hip", f"-Wl,-rpath,{libdir}"])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "facade fuse ok" in out.stdout, (out.returncode, out.stdout, out.stderr)


def test_fuse_lds_layout_under_sanitizers(tmp_path):
    """LdsFuse for every capacity the launcher can pass: arrays aligned, disjoint, inside the total, swept under AddressSanitizer
    and UBSan in a stand-alone host program."""
    exe = str(tmp_path / "fuse_lds_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined",
                           "-I", os.path.join(ROOT, "sdslam_amd", "csrc"), os.path.join(ROOT, "tests", "native", "fuse_lds_check.cpp"),
                           "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "fuse_lds_check OK" in out.stdout, out.stdout + out.stderr
