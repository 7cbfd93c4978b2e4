"""k_pnp after its LDS was re-laid (csrc/track_pnp_lds.h: padded + rotated rows of the 12 x 12 Jacobi matrix, L and the parked
barycentric coordinates inside the call-local scratch area): the shapes at which a wrong address map shows.

GPU: get_pnp equals the oracle exactly in ok / iterations / n_inliers / inliers / refined and within test_pnp_ransac's pose
tolerance in T; sd_debug_epnp equals the oracle's EPnP.  CPU: the address map itself, every step of a sweep replayed on the
bank rules (tests/native/pnp_lds_check.cpp)."""
import os
import subprocess

import numpy as np
import pytest

import pnp_cases as PC
from sdslam_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CFG = (1000, 1.2, 8, 20)
BOUNDS = (0.0, 640.0, 0.0, 480.0)
POSE_TOL = 1e-5          # tests/test_pnp_ransac.py
EPNP_TOL = 1e-9          # tests/test_track_gpu.py::test_epnp_device_vs_oracle

# name -> (planted kwargs, SetRansacParameters args, iterate() calls, seeds of the B = 3 frames)
CASES = {
    # 70 correspondences, all inliers: the refit runs on more than 64 of them -- two 64-blocks in every ordered sum and in the
    # M^T M staging, the second partial
    "n70_two_blocks": (dict(n_match=70, outlier_frac=0.0, noise_px=0.3), (0.99, 10, 200, 4, 0.28, 5.991), [200], (7, 8, 9)),
    # every refit rejected (exactly minInliers exact inliers), so the loop runs to the end: one chunk with all eight hypotheses
    # in flight ...
    "chunk_full_8": (dict(n_match=60, outlier_frac=0.0, n_exact_inliers=30), (0.99, 10, 8, 4, 0.5, 5.991), [8], (7, 8, 9)),
    # ... and 11 iterations: the second chunk has three hypotheses, five matrices of the work area are absent
    "chunk_partial_11": (dict(n_match=60, outlier_frac=0.0, n_exact_inliers=30), (0.99, 10, 11, 4, 0.5, 5.991), [11], (7, 8, 9)),
    # 40 % outliers of 120: frame 0 (seed 35) has a rejected refit in the first chunk (a 5-inlier hypothesis at iteration 4)
    # and is accepted by a second refit in the third chunk (iteration 17); test_out40_case_is_what_it_claims pins that
    "out40_refits": (dict(n_match=120, outlier_frac=0.4, noise_px=0.5), (0.99, 5, 200, 4, 0.03, 5.991), [200], (35, 36, 37)),
    # k_pnp<true>: minimal sets of five, every hypothesis through the wave-cooperative solver
    "minset5": (dict(n_match=120, outlier_frac=0.3, noise_px=0.5), (0.99, 10, 100, 5, 0.28, 5.991), [100, 3], (7, 8, 9)),
}


@pytest.fixture(scope="module")
def frame(oracle):
    s = synth.make_scene(20)
    oc = oracle.OrbOracle(*CFG)
    ck, cd = oc.extract(s["cur"])
    return dict(scene=s, ck=ck, tab=oc.tables())


@pytest.fixture(scope="module")
def expected(oracle, frame):
    """The oracle's results for every case and frame, computed once."""
    out = {}
    for name, (kw, params, calls, seeds) in CASES.items():
        rs = synth.glibc_rand_stream(PC.rand_needed(params, calls))
        cases = [PC.planted(s, frame["ck"], frame["scene"]["T_cur"], **kw) for s in seeds]
        res = [PC.run_oracle(oracle, frame["ck"], frame["tab"]["sigma2"], c[0], c[1], params, calls, rs) for c in cases]
        out[name] = dict(cases=cases, rs=rs, res=res)
    return out


def test_cases_are_what_they_claim(expected):
    e = expected["n70_two_blocks"]
    for res, pr in e["res"]:
        assert pr["N"] == 70 and res[0]["ok"] and not res[0]["no_more"] and 64 < res[0]["n_inliers"] < 128
    for name, n in (("chunk_full_8", 8), ("chunk_partial_11", 11)):
        for res, pr in expected[name]["res"]:
            assert pr["max_its"] == n and res[0]["iterations"] == n and res[0]["no_more"]
    for res, pr in expected["minset5"]["res"]:
        assert res[0]["ok"]


def test_out40_case_is_what_it_claims(oracle, frame, expected):
    """Frame 0 of out40_refits: stopping the solver after i iterations returns the un-refined best set (ok + bNoMore) as soon as
    a hypothesis has reached minInliers without its refit being accepted."""
    kw, params, calls, seeds = CASES["out40_refits"]
    e = expected["out40_refits"]
    r = e["res"][0][0][0]
    assert r["ok"] and not r["no_more"] and r["iterations"] == 17 and e["res"][0][1]["N"] == 120
    last, cm, _ = e["cases"][0]
    rejected_at = None
    for i in range(1, r["iterations"]):
        ri, _ = PC.run_oracle(oracle, frame["ck"], frame["tab"]["sigma2"], last, cm, params[:2] + (i,) + params[3:], [i], e["rs"])
        assert ri[0]["no_more"]
        if ri[0]["ok"] and rejected_at is None:
            rejected_at = i
    assert rejected_at is not None and rejected_at <= 8 < r["iterations"]   # rejected in the first chunk, accepted in a later one


def test_lds_map_has_no_bank_conflict(tmp_path):
    exe = str(tmp_path / "pnp_lds_check")
    subprocess.check_call([os.environ.get("CXX", "g++"), "-std=c++17", "-O1", "-fsanitize=undefined,address", "-fno-sanitize-recover=all",
                           "-I", os.path.join(ROOT, "sdslam_amd", "csrc"), os.path.join(ROOT, "tests", "native", "pnp_lds_check.cpp"),
                           "-o", exe])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "pnp_lds_check OK" in out.stdout, out.stdout + out.stderr
    assert "worst conflict degree: reads 1, writes 1" in out.stdout


# ------------------------------------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def gpu_rig(frame):
    import sdslam_amd
    if sdslam_amd.device_count() < 1:
        pytest.fail("no HIP device: the gpu-marked tests need a real MI355X")
    B = 3
    cur, ref = sdslam_amd.ORBextractor(*CFG, 640, 480, B), sdslam_amd.ORBextractor(*CFG, 640, 480, B)
    k, d, n = cur.extract_batch(np.stack([frame["scene"]["cur"]] * B))
    ref.extract_batch(np.stack([frame["scene"]["ref"]] * B))
    assert np.array_equal(k[0, :n[0]], frame["ck"])
    trk = sdslam_amd.Tracker(cur, ref, max_points=1000, max_batch=B, pnp_max_iterations=512)
    trk.set_camera(*PC.K, 0.0, BOUNDS)
    return dict(trk=trk, B=B)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(CASES))
def test_hip_pnp_equals_oracle(frame, expected, gpu_rig, name):
    trk, B = gpu_rig["trk"], gpu_rig["B"]
    n = len(frame["ck"])
    kw, params, calls, seeds = CASES[name]
    e = expected[name]
    trk.set_last(0, [c[0] for c in e["cases"]])
    trk.set_matches(0, np.stack([c[1] for c in e["cases"]]))
    trk.set_rand(0, np.tile(e["rs"], (B, 1)))
    for k, nit in enumerate(calls):
        if k == 0:
            trk.pnp(B, *params, nit)
        else:
            trk.pnp_iterate(B, nit)
        g = trk.get_pnp(0, B)
        for b in range(B):
            r = e["res"][b][0][k]
            got = (bool(g["ok"][b]), int(g["iterations"][b]), int(g["n_inliers"][b]), bool(g["refined"][b]))
            print(name, "call", k, "frame", b, "device", got, "oracle", (r["ok"], r["iterations"], r["n_inliers"]),
                  "max |dT|", np.abs(g["T"][b] - r["T"]).max())
            assert got == (r["ok"], r["iterations"], r["n_inliers"], r["ok"] and not r["no_more"]), (name, b, k)
            assert np.array_equal(g["inliers"][b, :n], r["inliers"]), (name, b, k)
            assert np.abs(g["T"][b] - r["T"]).max() <= POSE_TOL, (name, b, k)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [4, 5, 64, 65])
def test_hip_epnp_equals_oracle(oracle, gpu_rig, n):
    """sd_debug_epnp: n = 4 is the minimal-set solver (per-hypothesis views, parked alphas), the others the wave-cooperative
    one at one short block, one full block, one full block + one correspondence."""
    from sdslam_amd.capi import debug_epnp
    rng = np.random.default_rng(100 + n)
    for trial in range(3):
        T = synth.se3_exp(rng.normal(size=3) * 0.1, rng.normal(size=3) * 5.0)
        Xc = np.stack([rng.uniform(-1.5, 1.5, n), rng.uniform(-1.0, 1.0, n), rng.uniform(2.0, 6.0, n)], 1)
        Xw = ((Xc - T[:3, 3]) @ T[:3, :3]).astype(np.float32).astype(np.float64)
        Xc = Xw @ T[:3, :3].T + T[:3, 3]
        uv = np.stack([PC.K[0] * Xc[:, 0] / Xc[:, 2] + PC.K[2], PC.K[1] * Xc[:, 1] / Xc[:, 2] + PC.K[3]], 1)
        uv = (uv + rng.normal(size=uv.shape) * 0.3).astype(np.float32).astype(np.float64)
        R, t, e = oracle.epnp(Xw, uv, PC.K)
        Rg, tg, eg = debug_epnp(Xw, uv, PC.K)
        print("n", n, "trial", trial, "max |dR|", np.abs(R - Rg).max(), "max |dt|", np.abs(t - tg).max())
        assert np.abs(R - Rg).max() <= EPNP_TOL and np.abs(t - tg).max() <= EPNP_TOL, (n, trial)
