"""No GPU: tests/imu_ref.py (the numpy restatement of EKF + IMU) pinned from first principles, the float64 / longdouble noise
floor on the inputs of tests/test_imu_gpu.py, and the ABI / facade declarations of the IMU sensor model."""
import os
import re
import subprocess

import numpy as np

import imu_cases as IC
import imu_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["sd_track_set_sensor_model", "sd_track_get_sensor_model", "sd_track_set_measurements", "sd_track_get_imu", "sd_track_set_imu"]
DT = 1.0 / 30.0
P0 = np.diag([R.COV_X_2] * 3 + [R.COV_Q_2] * 4 + [R.COV_V_2] * 3 + [R.COV_W_2] * 3 + [R.COV_A_2] * 3)
_BLK = np.repeat(np.arange(5), [3, 4, 3, 3, 3])
BLOCKS = _BLK[:, None] == _BLK[None, :]                                 # the diagonal blocks of P (x, q, v, w, a)
X0 = np.array([0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0], np.float64)


def run_constant_stream(v, w, a, steps, dt=DT):
    """The filter on a stream with constant v, w in the model's kinematics; per step (prior error, |X_v - v|, |X_w - w|)."""
    x, q = np.array([0.1, -0.2, 0.3]), R.quat_from_angular_velocity(np.array([0.1, 0.05, -0.08]))
    f, T, out = R.EKF(), IC.pose_of(x, q), []
    for _ in range(steps):
        prior = f.predict(T, dt)
        x = x + v * dt
        q = R.quat_mul(q, R.quat_from_angular_velocity(w * dt))
        T = IC.pose_of(x, q)
        err = np.abs(prior - T).max()
        f.track(T, np.concatenate([w, a]))
        out.append((err, np.abs(f.X[7:10] - v).max(), np.abs(f.X[10:13] - w).max()))
    return f, np.array(out)


def test_constant_stream_converges_to_v_and_w():
    """Exact poses and gyro of a constant-(v, w) stream: X[7:13] converges towards (v, w) and the predicted pose error shrinks."""
    v, w = np.array([0.2, -0.1, 0.15]), np.array([0.3, -0.2, 0.25])
    f, out = run_constant_stream(v, w, np.zeros(3), 30)
    assert out[0, 1] == np.abs(v).max() and out[0, 2] == np.abs(w).max()   # InitState: the pose only, no velocities yet
    for col in (0, 1, 2):                                               # prior error, v error, w error: each drops by > 1e3
        assert out[10, col] < out[2, col] * 1e-1 and out[29, col] < out[2, col] * 1e-3, (col, out[:, col])
    assert out[29, 1] < 1e-9 and out[29, 2] < 1e-9 and out[29, 0] < 1e-9
    assert abs(np.linalg.norm(f.X[3:7]) - 1.0) < 1e-6                   # q follows the unit quaternions it is fed


def test_gravity_follows_the_low_pass():
    """Constant a: gravity_ = 0 after the first update (InitState), then g <- alpha g + (1 - alpha) a per update, i.e.
    a (1 - alpha^k) after k further updates; Z's accelerometer part is a - gravity_."""
    a = np.array([0.3, 9.81, -0.2])
    f, T = R.EKF(), np.eye(4)
    alpha = 0.27 / (0.27 + DT)
    for k in range(6):
        f.predict(T, DT)
        f.track(T, np.concatenate([np.zeros(3), a]))
        assert np.allclose(f.gravity, a * (1.0 - alpha ** k), rtol=1e-13, atol=0), k
    assert not np.array_equal(f.gravity, a)


def test_restart_returns_init():
    f, _ = run_constant_stream(np.array([0.1, 0.2, 0.3]), np.array([0.3, 0.1, 0.2]), np.array([0.0, 9.81, 0.0]), 5)
    assert f.started() and f.gravity.any() and not np.array_equal(f.P, P0)
    before = f.P.copy()
    f.restart()
    assert not f.started() and np.array_equal(f.X, X0) and not f.gravity.any()
    # IMU::Init assigns the five diagonal blocks of P; EKF::Restart leaves the off-diagonal blocks as they were
    assert np.array_equal(f.P[BLOCKS], P0[BLOCKS]) and np.array_equal(f.P[~BLOCKS], before[~BLOCKS]) and before[~BLOCKS].any()
    g = R.EKF()
    assert np.array_equal(g.X, X0) and np.array_equal(g.P, P0) and not g.started() and g.it_time == 0.0
    f.predict(np.zeros((4, 4)), DT)
    f.track(np.eye(4), np.ones(6))                                      # last_pose isZero(): restart instead of update
    assert not f.started()
    f.predict(np.eye(4), DT)
    f.track(np.eye(4), np.ones(6), tracked=False)
    assert not f.started() and np.array_equal(f.P[BLOCKS], P0[BLOCKS])


def test_first_update_stores_pose_and_zeroes_gravity():
    poses, meas = IC.stream(9)
    f = R.EKF()
    prior = f.predict(poses[0], DT)
    assert prior.tobytes() == poses[0].tobytes() and f.it_time == 0.0 and np.array_equal(f.X, X0)   # not started: the last pose
    f.gravity[:] = 5.0                                                  # whatever gravity held, InitState zeroes it
    f.track(poses[1], meas[0])
    assert f.started() and not f.gravity.any() and not f.X[7:].any() and np.array_equal(f.P, P0)
    assert np.array_equal(f.X[:7], R.pose_to_vector(poses[1]))
    assert np.abs(R.get_pose(f.X) - poses[1]).max() < 1e-15


def test_dt_zero_step_stays_finite():
    """dt = 0: jF = I, Q = 0, R = 0, S = the sub-block of P; the update puts the measured rows on the measurement."""
    poses, meas = IC.stream(4, [DT, 0.1, DT, 0.0, DT])
    f = R.EKF()
    for k, dt in enumerate([DT, 0.1, DT, 0.0, DT]):
        P_before = f.P.copy()
        prior = f.predict(poses[k], dt)
        if dt == 0.0:
            assert np.array_equal(f.P, P_before) and f.it_time == 0.0
        f.track(poses[k + 1], meas[k])
        assert np.isfinite(f.X).all() and np.isfinite(f.P).all() and np.isfinite(prior).all(), k
        if dt == 0.0:
            assert np.abs(f.X[:7] - R.pose_to_vector(poses[k + 1])).max() < 1e-9 and np.abs(f.P[np.ix_(R.SEL, R.SEL)]).max() < 1e-12


def test_dq_by_dw_matches_a_finite_difference():
    """d(q (x) quat(w t)) / dw by central differences, in longdouble so the step can be small; and the |w| == 0 branch as the
    reference writes it (t / 2 on the vector rows, not multiplied by the quaternion's Jacobian)."""
    L = np.longdouble
    rng = np.random.Generator(np.random.PCG64(5))
    for _ in range(5):
        q = rng.normal(size=4).astype(L)
        q /= np.sqrt((q * q).sum())
        w, t, h = rng.uniform(-1, 1, 3).astype(L), L(rng.uniform(0.02, 0.2)), L(1e-7)
        num = np.zeros((4, 3), L)
        for c in range(3):
            e = np.zeros(3, L)
            e[c] = h
            num[:, c] = (R.quat_mul(q, R.quat_from_angular_velocity((w + e) * t)) - R.quat_mul(q, R.quat_from_angular_velocity((w - e) * t))) / (2 * h)
        assert np.abs(num - R.dq_by_dw(q, w, t)).max() < 1e-11
        assert np.abs(R.dq_by_dw(q.astype(np.float64), w.astype(np.float64), float(t)) - R.dq_by_dw(q, w, t)).max() < 1e-15
    z = R.dq_by_dw(np.array([0.5, 0.5, 0.5, 0.5]), np.zeros(3), 0.1)
    assert np.array_equal(z, np.vstack([np.zeros((1, 3)), np.eye(3) * 0.05]))
    assert np.array_equal(R.quat_from_angular_velocity(np.zeros(3)), [1, 0, 0, 0])


def test_noise_floor_of_the_gpu_inputs():
    """float64 against longdouble on exactly the slot inputs of tests/test_imu_gpu.py, after every step.  Measured here:
    2.36e-15 (slot 30, step 5); the GPU bound is 64 x the figure measured on the machine that runs the test (1.5e-13)."""
    margin = min(IC.trace_margin(IC.stream(i)[0]) for i in range(IC.B))
    assert margin > 1.0, margin                                         # rotation angles under pi / 2: first branch, far from 0
    gap = IC.noise_floor()
    print(f"IMU filter noise floor: float64 vs longdouble gap {gap:.3e}, GPU bound {64 * gap:.3e}, smallest trace(R) {margin:.3f}")
    assert np.isfinite(gap) and gap > 0.0
    kinds = {IC.slot_params(i)["kind"] for i in range(IC.B)}
    assert kinds == set(range(7)) and not IC.slot_params(0)["w"].any() and IC.slot_params(2)["a"][1] > 9.0
    assert not IC.stream(1)[1][:IC.SWITCH, :3].any() and IC.stream(1)[1][IC.SWITCH:, :3].all()
    assert IC.DTS.count(0.0) == 1 and set(IC.DTS) == {0.0, 0.1, 1.0 / 30.0}


def test_imu_symbols_declared_and_bound():
    hdr = open(os.path.join(ROOT, "include", "sdslam_hip.h")).read()
    assert re.search(r"#define SD_SENSOR_CONSTANT_VELOCITY 0\b", hdr) and re.search(r"#define SD_SENSOR_IMU 1\b", hdr)
    for sym, args in (("sd_track_set_sensor_model", r"sd_track\* h, int model"),
                      ("sd_track_get_sensor_model", r"sd_track\* h, int\* model"),
                      ("sd_track_set_measurements", r"sd_track\* h, int frame0, int n_frames, const double\* wa6"),
                      ("sd_track_get_imu", r"sd_track\* h, int frame0, int n_frames, double\* X16, double\* P256, double\* gravity3, int32_t\* started,\s*"
                                           r"double\* it_time,\s*double\* last_pose_cm, double\* measurements6"),
                      ("sd_track_set_imu", r"sd_track\* h, int frame0, int n_frames, const double\* X16, const double\* P256, const double\* gravity3,\s*"
                                           r"const int32_t\* started, const double\* it_time")):
        assert re.search(r"\bint " + sym + r"\(" + args + r"\);", hdr), sym
    assert "and the IMU sensor model" not in hdr
    from sdslam_amd import capi
    for m in ("set_sensor_model", "get_sensor_model", "set_measurements", "get_imu", "set_imu"):
        assert callable(getattr(capi.Tracker, m, None)), m
    hpp = open(os.path.join(ROOT, "include", "sdslam", "sdslam.hpp")).read()
    for m in ("SetSensorModel", "SetMeasurements", "ImuState"):
        assert re.search(r"\b" + m + r"\(", hpp), m


def test_imu_symbols_exported():
    from sdslam_amd import build, capi
    build.build()
    L = capi.lib()
    for sym in SYMBOLS:
        assert hasattr(L, sym), sym


def test_cpp_imu_facade_compiles_and_links(tmp_path):
    import sdslam_amd
    from sdslam_amd import build
    build.build()
    exe = str(tmp_path / "sd_facade_imu")
    libdir = os.path.dirname(sdslam_amd.lib_path())
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-I", os.path.join(ROOT, "include"),
                           os.path.join(ROOT, "tests", "native", "facade_imu.cc"), "-o", exe,
                           "-L", libdir, "-lsdslam_hip", f"-Wl,-rpath,{libdir}"])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "facade imu ok" in out.stdout, (out.returncode, out.stdout, out.stderr)
