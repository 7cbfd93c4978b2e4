"""CPU: the numpy restatement of the reference's motion model (tests/motion_ref.py) is self-consistent on the twists the GPU
tests use, its dense 6x6 filter stays exactly diagonal, and the motion-model calls are declared in the C header, bound in
the Python layer and reachable through the C++ facade."""
import math
import os
import re
import subprocess

import numpy as np
import pytest

import motion_cases as MC
import motion_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["sd_track_motion_predict", "sd_track_motion_update", "sd_track_motion_restart", "sd_track_get_motion", "sd_track_set_motion"]

# Round trips go through (1 - cos t) / t^2 and (t - sin t) / t^3, whose relative error is ~1e-16 / t^2 resp. 1e-16 / t^3 times
# the argument's own magnitude: worst at t = 1e-6, where (1 - cos t) / t^2 carries ~1e-4 relative error, scaled by |Omega| =
# 1e-6 and |upsilon| <= 0.03: 3e-12.  Everything else is a few ulp of values <= 3.
RT_TOL = 1e-11


@pytest.mark.parametrize("name", MC.NAMES)
def test_exp_log_round_trips(name):
    x = MC.TWISTS[name]
    T = R.exp(x)
    assert np.abs(T[:3, :3] @ T[:3, :3].T - np.eye(3)).max() < 1e-14 and np.array_equal(T[3], [0, 0, 0, 1])
    y = R.log(T)
    T2 = R.exp(y)
    assert np.abs(T2[:3, :3] - T[:3, :3]).max() < RT_TOL
    assert np.abs(y[3:] - x[3:]).max() < RT_TOL
    if name != "w_negative":
        assert np.abs(y[:3] - x[:3]).max() < RT_TOL and np.abs(T2 - T).max() < RT_TOL
    else:
        # the reference's quirk: theta < 0 takes the small-angle V_inv, so the translation does not come back
        assert np.abs(y[:3] - x[:3]).max() > 1e-4


def test_twists_reach_every_branch():
    q = {n: R.mat_to_quat(R.exp(x)[:3, :3]) for n, x in MC.TWISTS.items()}
    tr = {n: np.trace(R.exp(x)[:3, :3]) for n, x in MC.TWISTS.items()}
    for n, i in (("rot_x", 0), ("rot_y", 1), ("rot_z", 2)):
        m = R.exp(MC.TWISTS[n])[:3, :3]
        assert tr[n] < 0 and int(np.argmax(np.diag(m))) == i and q[n][0] > 0
    assert tr["w_negative"] < 0 and q["w_negative"][0] < 0
    assert R.rotation_log(R.quat_normalize(q["w_negative"]))[1] < 0             # negative theta
    assert np.array_equal(MC.TWISTS["translation"][3:], np.zeros(3))
    th = {n: np.linalg.norm(x[3:]) for n, x in MC.TWISTS.items()}
    assert 0 < th["rot_1e-11"] < R.SMALL_EPS < th["rot_1e-6"] < 2e-6
    assert abs(th["rot_0.5"] - 0.5) < 1e-12 and th["rot_x"] > math.radians(120)
    assert np.array_equal(R.exp(np.zeros(6)), np.eye(4))                        # what makes the unstarted prior exact
    for n, x in MC.TWISTS.items():                                              # conversions agree with each other
        m = R.exp(x)[:3, :3]
        assert np.abs(R.quat_to_mat(R.quat_normalize(q[n])) - m).max() < 1e-14, n


def test_dense_filter_stays_diagonal():
    """jF = jH = G = I and diagonal Q, R, P0: the off-diagonals of P (and so of S and K) stay exactly 0 over 20 steps, and
    the dense filter equals six scalar filters bit for bit."""
    off = ~np.eye(6, dtype=bool)
    for name in ("sequence", "rot_0.5", "rot_x", "w_negative"):
        f = R.EKF()
        T = R.exp(np.array([0.3, -0.2, 0.1, 0.2, 0.1, -0.3]))
        step = R.exp(MC.TWISTS[name])
        x, p, started = np.zeros(6), np.array([R.COV_V_2] * 3 + [R.COV_W_2] * 3), False
        for t in range(20):
            dt = MC.DTS[t % len(MC.DTS)] if t != 12 else 0.05                    # a single dt = 0 step
            f.predict(T, dt)
            it = dt if started else 0.0
            q = np.array([R.SIGMA_V * R.SIGMA_V * it * it] * 3 + [R.SIGMA_W * R.SIGMA_W * it * it] * 3)
            p = p + q
            T2 = step @ T
            f.update(T2)
            assert (f.P[off] == 0).all(), (name, t)
            if started:
                rot = T[:3, :3].T
                Li = np.eye(4)
                Li[:3, :3], Li[:3, 3] = rot, -(rot @ T[:3, 3])
                Z = R.log(T2 @ Li)
                s = p + q
                k = p * (1.0 / s)
                x = x + k * (Z - x)
                p = p - (k * s) * k
            started = True
            assert np.array_equal(f.X, x) and np.array_equal(np.diag(f.P), p), (name, t)
            T = T2
        assert np.abs(f.X - R.log(step)).max() < 1e-3 or name == "w_negative"  # the filter follows the constant twist


def test_restart_and_zero_last_pose():
    f = R.EKF()
    T = R.exp(MC.TWISTS["sequence"])
    f.predict(np.eye(4), 0.1)
    f.track(T)
    f.predict(T, 0.1)
    f.track(T @ T)
    assert f.started() and f.it_time == 0.1 and np.abs(f.X).max() > 0
    f.track(T, tracked=False)
    assert not f.started() and not f.X.any() and np.array_equal(np.diag(f.P), [R.COV_V_2] * 3 + [R.COV_W_2] * 3)
    f.predict(np.zeros((4, 4)), 0.1)
    f.track(T)                                                                  # isZero(): restart instead of update
    assert not f.started()
    assert f.predict(T, 0.1).tobytes() == T.tobytes() and f.it_time == 0.0      # unstarted: the prior is the last pose


def test_motion_symbols_declared_and_bound():
    """The five calls are in the C header with the documented signatures and bound by the Python layer."""
    hdr = open(os.path.join(ROOT, "include", "sdslam_hip.h")).read()
    for sym, args in (("sd_track_motion_predict", r"sd_track\* h, int n_frames, double dt"),
                      ("sd_track_motion_update", r"sd_track\* h, int n_frames, int source"),
                      ("sd_track_motion_restart", r"sd_track\* h, int frame0, int n_frames"),
                      ("sd_track_get_motion", r"sd_track\* h, int frame0, int n_frames, double\* X6, double\* Pdiag6, int32_t\* started,\s*"
                                              r"double\* it_time,\s*double\* E_cm, double\* last_pose_cm"),
                      ("sd_track_set_motion", r"sd_track\* h, int frame0, int n_frames, const double\* X6, const double\* Pdiag6,\s*"
                                              r"const int32_t\* started,\s*const double\* it_time")):
        assert re.search(r"\bint " + sym + r"\(" + args + r"\);", hdr), sym
    from sdslam_amd import capi
    src = open(capi.__file__).read()
    for sym in SYMBOLS:
        assert sym in src, sym
    for m in ("motion_predict", "motion_update", "motion_restart", "get_motion", "set_motion"):
        assert callable(getattr(capi.Tracker, m, None)), m
    hpp = open(os.path.join(ROOT, "include", "sdslam", "sdslam.hpp")).read()
    for m in ("PredictMotion", "UpdateMotion", "RestartMotion", "MotionState"):
        assert re.search(r"\b" + m + r"\(", hpp), m


def test_motion_symbols_exported():
    from sdslam_amd import build, capi
    build.build()
    L = capi.lib()
    for sym in SYMBOLS:
        assert hasattr(L, sym), sym


def test_cpp_motion_facade_compiles_and_links(tmp_path):
    import sdslam_amd
    from sdslam_amd import build
    build.build()
    exe = str(tmp_path / "sd_facade_motion")
    libdir = os.path.dirname(sdslam_amd.lib_path())
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "native", "facade_motion.cc"), "-o", exe,
                           "-L", libdir, "-lsdslam_hip", f"-Wl,-rpath,{libdir}"])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "facade motion ok" in out.stdout, (out.returncode, out.stdout, out.stderr)
