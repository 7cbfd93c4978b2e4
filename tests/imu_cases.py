"""Inputs shared by the IMU sensor-model tests (helper, no tests): 70 slots, each a stream with its own constant (v, w, a) in
the model's own kinematics (x += v dt, q <- q (x) quat(w dt)), fed to the filter as exact poses, the gyro reading w and the
accelerometer reading a.  tests/test_imu_cpu.py measures the float64 / longdouble gap on exactly these inputs and
tests/test_imu_gpu.py compares the device on them.

Kinds, by slot % 7:
  0  w = 0 exactly and a pure translation: the state's w stays small, the |w| == 0 branches of dq_by_dw and
     QuaternionFromAngularVelocity run at the first prediction of EVERY slot (InitState leaves w = 0)
  1  no rotation for the first four steps, then w != 0: a state w that becomes non-zero later
  2  a = a gravity-sized constant (0, 9.81, 0) plus a small term: gravity_ follows the low-pass
  3..6  random v, w, a
Rotation angles stay under 1 rad from the identity (start <= 0.3 rad, |w| <= 1 rad/s over 0.53 s), so trace(R) stays far from
the branch boundary of the matrix -> quaternion conversion; trace_margin() is asserted by the tests."""
import numpy as np

import imu_ref as R
from motion_ref import quat_normalize, quat_to_mat

B = 70
# dt per step: 1/30 and 0.1 alternating, one step with dt = 0.  Step 0 is the first update (InitState); the dt = 0 step comes
# after three real updates.
DTS = [1.0 / 30.0, 0.1, 1.0 / 30.0, 0.1, 0.0, 1.0 / 30.0, 0.1, 1.0 / 30.0]
SWITCH = 4                                                       # kind 1: the step from which w != 0


def slot_params(i):
    rng = np.random.Generator(np.random.PCG64(1000 + i))
    v = rng.uniform(-0.5, 0.5, 3)
    w = rng.uniform(-0.55, 0.55, 3)
    a = rng.uniform(-0.3, 0.3, 3)
    ax = rng.normal(size=3)
    q0 = R.quat_from_angular_velocity(ax / np.linalg.norm(ax) * rng.uniform(0.0, 0.3))
    x0 = rng.uniform(-0.5, 0.5, 3)
    kind = i % 7
    if kind == 0:
        w = np.zeros(3)
    if kind == 2:
        a = a + np.array([0.0, 9.81, 0.0])
    return dict(kind=kind, v=v, w=w, a=a, q0=q0, x0=x0)


def pose_of(x, q):
    T = np.eye(4)
    T[:3, :3] = quat_to_mat(quat_normalize(q))
    T[:3, 3] = x
    return T


def stream(i, dts=DTS):
    """(poses [len(dts) + 1], measurements [len(dts)][6]) of slot i: pose k + 1 is the frame tracked at step k, measurement k the
    reading handed over with it."""
    p = slot_params(i)
    x, q = p["x0"].copy(), p["q0"].copy()
    poses, meas = [pose_of(x, q)], []
    for k, dt in enumerate(dts):
        w = np.zeros(3) if (p["kind"] == 1 and k < SWITCH) else p["w"]
        x = x + p["v"] * dt
        q = R.quat_mul(q, R.quat_from_angular_velocity(w * dt))
        poses.append(pose_of(x, q))
        meas.append(np.concatenate([w, p["a"]]))
    return poses, np.array(meas)


def trace_margin(poses):
    """Smallest trace(R) over the poses: > 0 selects the first branch of the matrix -> quaternion conversion."""
    return min(float(np.trace(T[:3, :3])) for T in poses)


_FLOOR = []


def noise_floor():
    """The float64 and the longdouble filter of tests/imu_ref.py on every slot's stream, compared after every predict and
    every update: the largest absolute gap in X, P, gravity and the prior.  Computed once per process."""
    if not _FLOOR:
        gap = 0.0
        for i in range(B):
            poses, meas = stream(i)
            f64, f80 = R.EKF(), R.EKF(np.longdouble)
            for k, dt in enumerate(DTS):
                g = np.abs(f64.predict(poses[k], dt) - f80.predict(poses[k], dt)).max()
                g = max(g, np.abs(f64.X - f80.X).max(), np.abs(f64.P - f80.P).max())
                f64.track(poses[k + 1], meas[k])
                f80.track(poses[k + 1], meas[k])
                g = max(g, np.abs(f64.X - f80.X).max(), np.abs(f64.P - f80.P).max(), np.abs(f64.gravity - f80.gravity).max())
                gap = max(gap, float(g))
        _FLOOR.append(gap)
    return _FLOOR[0]
