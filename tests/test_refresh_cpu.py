"""CPU (no GPU): the numpy restatement of ComputeDistinctiveDescriptors / UpdateNormalAndDepth (tests/refresh_ref.py) against
answers worked out by hand, the coverage of the seeded cases the GPU test runs (tests/refresh_cases.py), the new ABI symbols,
the LDS layout and lifetime checks on the host, and the facade's host part under AddressSanitizer + UBSan.

Descriptors with chosen distances: bits(k) has its first k bits set, so hamming(bits(a), bits(b)) = |a - b|.

On the ranks: the reference takes vDists[0.5 * (N - 1)], rank (N - 1) / 2.  For odd N that IS N / 2, so no N = 3 list can tell
the two apart (its known answer is pinned all the same); N = 4 and N = 6 can, and do below."""
import os
import re
import subprocess

import numpy as np
import pytest

import refresh_cases as RC
import refresh_ref as RR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SAN = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined"]


def bits(k):
    d = np.zeros(256, np.uint8)
    d[:k] = 1
    return np.packbits(d)


def line(*ks):
    return np.stack([bits(k) for k in ks])


def test_hamming_is_the_bit_count():
    assert RR.hamming(bits(0), bits(256)) == 256 and RR.hamming(bits(7), bits(19)) == 12 and RR.hamming(bits(5), bits(5)) == 0
    a = np.random.default_rng(0).integers(0, 256, 32).astype(np.uint8)
    assert RR.hamming(a, ~a) == 256


def test_known_answers():
    assert RR.distinctive_descriptor(line(9)) == (0, 0)                      # N = 1: own descriptor, median 0
    # N = 2: rank 0 of {0, d} is the diagonal for both rows: the first observation, whatever d is
    assert RR.distinctive_descriptor(line(0, 200)) == (0, 0) and RR.distinctive_descriptor(line(200, 0)) == (0, 0)
    # N = 3: rank 1 = the smaller off-diagonal distance; D = |0-10| 10, |0-13| 13, |10-13| 3: rows {0,10,13} {0,3,10} {0,3,13}
    assert RR.distinctive_descriptor(line(0, 10, 13)) == (1, 3)
    # N = 4 on a line at 0, 1, 10, 12: rows sorted {0,1,10,12} {0,1,9,11} {0,2,9,10} {0,2,11,12}.  Rank 1: 1, 1, 2, 2 -> row 0;
    # rank 2 (N / 2) would read 10, 9, 9, 11 -> row 1
    assert RR.distinctive_descriptor(line(0, 1, 10, 12)) == (0, 1)
    assert RR.distinctive_descriptor(line(0, 1, 10, 12), rank_of=lambda N: N // 2) == (1, 9)
    # N = 6 at 0, 2, 4, 20, 21, 22: rank 2 reads 4, 2, 4, 2, 1, 2 -> row 4; rank 3 reads 20, 18, 16, 16, 17, 18 -> row 2
    assert RR.distinctive_descriptor(line(0, 2, 4, 20, 21, 22)) == (4, 1)
    assert RR.distinctive_descriptor(line(0, 2, 4, 20, 21, 22), rank_of=lambda N: N // 2) == (2, 16)
    # a tie broken by order: rows 1, 2 and 3 are one descriptor, sorted {0,0,0,40,80}, rank 2 reads 0; row 0 reads 40, row 4 80
    assert RR.distinctive_descriptor(line(50, 10, 10, 10, 90)) == (1, 0)
    assert RR.distinctive_descriptor(line(10, 50, 10, 10, 90)) == (0, 0)


def test_a_permuted_list_gives_the_permuted_tie_break():
    """Why the order is the caller's: the same four observations in another order elect another descriptor."""
    d = line(0, 1, 10, 12)
    assert RR.distinctive_descriptor(d) == (0, 1)
    perm = [1, 0, 2, 3]
    w, m = RR.distinctive_descriptor(d[perm])
    assert (w, m) == (0, 1) and perm[w] == 1                                 # position 0 again -- now the other keyframe's descriptor
    assert not np.array_equal(d[0], d[perm][w])
    # and the normal's sum is sequential: a permutation changes its last bits on some list
    rng = np.random.default_rng(3)
    moved = 0
    for _ in range(50):
        c, X = rng.uniform(-1, 1, (7, 3)), rng.uniform(-1, 1, 3) + [0, 0, 5]
        a = RR.normal_and_depth(X, c, 0, np.zeros(7, np.int32), RC.SF)[0]
        b = RR.normal_and_depth(X, c[::-1], 6, np.zeros(7, np.int32), RC.SF)[0]
        moved += not np.array_equal(a, b)
        assert np.allclose(a, b, rtol=0, atol=1e-15)
    assert moved > 0


def test_bad_keyframes_are_skipped_by_one_function_only():
    d = line(0, 1, 10, 12)
    assert RR.distinctive_descriptor(d, [1, 0, 0, 0]) == (2, 2)              # rows {0,9,11} {0,2,9} {0,2,11} of list positions 1, 2, 3
    assert RR.distinctive_descriptor(d, [1, 1, 1, 1]) is None
    c = np.array([[0.0, 0, 0], [1, 0, 0], [0, 2, 0]])
    X = np.array([0.0, 0, 4])
    nv, mx, mn = RR.normal_and_depth(X, c, 1, [0, 3, 0], RC.SF)
    t = [(X - ci) / np.sqrt(((X - ci) ** 2).sum()) for ci in c]
    assert np.allclose(nv, (t[0] + t[1] + t[2]) / 3, rtol=0, atol=1e-15)     # n counts all three
    assert mx == np.float32(np.float32(np.sqrt(17.0)) * RC.SF[3]) and mn == np.float32(mx / RC.SF[-1])
    out = RR.refresh_points(np.array([0, 3]), line(0, 5, 9), c, [0, 3, 0], [1], X[None], RC.SF, obs_kf_bad=np.array([1, 1, 1]))
    assert out["status"][0] == RR.NORMAL and np.array_equal(out["normal"][0], nv) and not out["desc"].any()


def test_case_coverage():
    """What the GPU test relies on the cases for."""
    for name, make in RC.ALL.items():
        pts = make()
        c = RC.csr(pts)
        out = RR.refresh_points(fill=RR.empty_outputs(len(pts), seed=1), **{k: c[k] for k in c}, sf=RC.SF)
        for i, p in enumerate(pts):
            if "winner" in p:
                assert out["best_obs"][i] == p["winner"], (name, i)
        if name == "sized":
            assert tuple(len(p["desc"]) for p in pts) == RC.SIZES and (out["status"] == RR.DESC | RR.NORMAL).all()
        if name == "too_many":
            assert out["status"].tolist() == [3, RR.TOO_MANY, 3]
            before = RR.empty_outputs(3, seed=1)
            assert all(np.array_equal(out[k][1], before[k][1]) for k in RR.FIELDS if k != "status")      # untouched
        if name == "complementary":
            assert (out["best_median"] == 0).all()
        if name == "identical":
            assert (out["best_obs"] == 0).all() and (out["best_median"] == 0).all()
        if name == "tied":
            assert any(p["winner"] < 64 <= s for p, s in zip(pts, (80, 90, 64, 64, 255, 200, 70)))
        if name == "bad_keyframes":
            assert out["status"][3] == RR.NORMAL and (out["status"][[0, 1, 2, 4, 5, 6, 7]] == 3).all()
            assert out["best_obs"][6] >= 64                                 # the first 64 observations are bad: mapped back past them
        if name == "skipped":
            assert out["status"].tolist() == [3, RR.SKIPPED, RR.SKIPPED, RR.SKIPPED, 3]
        if name == "ref_octaves":
            assert [int(p["octave"][p["ref_obs"]]) for p in pts] == [0, RC.NLEVELS - 1, 0, RC.NLEVELS - 1]
    assert [len(RC.mixed(n)) for n in (1, 2, 5, 700)] == [1, 2, 5, 700]
    sizes = {len(p["desc"]) for p in RC.mixed(700)}
    assert {0, 63, 64, 65, 129, 256} <= sizes


def test_complementary_rows_reach_256():
    """The row of `a` has the median 256 and loses; read through a byte (256 -> 0) it would have the median 0 and, coming before
    the right winner, win."""
    for p in RC.complementary()[:5]:
        D = [RR.hamming(p["desc"][p["a_row"]], x) for x in p["desc"]]
        rank = (len(D) - 1) // 2
        assert sorted(D)[rank] == 256 and sorted(x & 255 for x in D)[rank] == 0 and p["a_row"] < p["winner"]
        for r in range(p["a_row"]):                                          # nothing before it has the median 0
            assert sorted(RR.hamming(p["desc"][r], x) for x in p["desc"])[rank] > 0


@pytest.fixture(scope="module")
def sd():
    import sdslam_amd
    from sdslam_amd import build
    build.build()          # hipcc cross-compiles gfx950 without a GPU
    return sdslam_amd


def test_abi_symbols(sd):
    import ctypes as C
    from sdslam_amd import capi
    import test_capi_signatures_cpu as SIG
    protos, L = SIG.prototypes(), sd.lib()
    want = {
        "sd_track_set_observations": ("int", [SIG.PTR, "int"] + [SIG.PTR] * 6),
        "sd_track_refresh_points": ("int", [SIG.PTR, "int", "int"]),
        "sd_track_get_refreshed": ("int", [SIG.PTR] * 8 + ["int"]),
        "sd_debug_refresh_points": ("int", ["int"] + [SIG.PTR] * 9 + ["int"] + [SIG.PTR] * 7),
    }
    for name, sig in want.items():
        assert protos[name] == sig and hasattr(L, name), name
        assert capi._SIGNATURES[name][0] is C.c_int and len(capi._SIGNATURES[name][1]) == len(sig[1])
    text = open(SIG.HEADER).read()
    defs = {k: int(v) for k, v in re.findall(r"#define (SD_REFRESH_\w+) (\d+)", text)}
    assert defs == dict(SD_REFRESH_MAX_OBS=256, SD_REFRESH_DESC=1, SD_REFRESH_NORMAL=2, SD_REFRESH_SKIPPED=16, SD_REFRESH_NOT_RESIDENT=32,
                        SD_REFRESH_TOO_MANY=64, SD_REFRESH_BAD_INDEX=128)
    assert (capi.REFRESH_MAX_OBS, capi.REFRESH_DESC, capi.REFRESH_NORMAL, capi.REFRESH_SKIPPED, capi.REFRESH_NOT_RESIDENT,
            capi.REFRESH_TOO_MANY, capi.REFRESH_BAD_INDEX) == (RR.MAX_OBS, RR.DESC, RR.NORMAL, RR.SKIPPED, RR.NOT_RESIDENT, RR.TOO_MANY,
                                                               RR.BAD_INDEX) == (256, 1, 2, 16, 32, 64, 128)
    assert L.sd_track_refresh_points(None, 0, 0) == 1 and b"NULL" in L.sd_last_error()
    assert L.sd_track_set_observations(None, 0, None, None, None, None, None, None) == 1


def _run_native(tmp_path, name, flags, include):
    exe = str(tmp_path / name)
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Werror"] + flags + ["-I", include, os.path.join(ROOT, "tests", "native", name + ".cpp"
                           if os.path.exists(os.path.join(ROOT, "tests", "native", name + ".cpp")) else name + ".cc"), "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and name + " OK" in out.stdout, out.stdout + out.stderr


def test_lds_layout(tmp_path):
    """Every array inside the workgroup's block, the aliasing as claimed, lane-own accesses conflict-free by the bank rules."""
    _run_native(tmp_path, "refresh_lds_check", SAN, os.path.join(ROOT, "sdslam_amd", "csrc"))


def test_result_lifetimes(tmp_path):
    for flags in (["-O2"], SAN):
        _run_native(tmp_path, "refresh_stamps_check", flags, os.path.join(ROOT, "sdslam_amd", "csrc"))


def test_facade_host_part_under_sanitizers(tmp_path):
    """BuildObservationLists / ApplyRefreshed on a toy map: a stand-alone program, AddressSanitizer + UBSan, no library."""
    _run_native(tmp_path, "facade_refresh", SAN, os.path.join(ROOT, "include"))
