"""Numpy restatement of the reference's IMU motion model (helper, no tests): EKF (src/sensors/EKF.cc:44-109) over the IMU
sensor (src/sensors/IMU.cc:26-240) with the helpers and constants of src/sensors/Sensor.cc:24-159, in the dense form: 16 x 16
P, jF and Q, an explicit 13 x 16 jH, 13 x 13 S and numpy.linalg.inv for S^-1.  The device selects rows instead of multiplying
by jH and inverts S by Gauss-Jordan; the comparison against this file checks that the two are the same filter.

`dtype` is numpy.float64 or numpy.longdouble.  In longdouble the inverse starts from the float64 one and is refined by Newton
steps X <- X (2 I - S X); the conversions taken from tests/motion_ref.py (matrix <-> quaternion) stay in float64, as the poses
are.  `dt` stands for the reference's wall-clock timer.  Conventions of the project's loop, not of EKF.cc: predict() of a
filter that is not started returns the last pose and leaves X and P alone (the reference never calls Predict there), and
track() is src/Tracking.cc:243-247 with the Restart() of :221 / :226.  Written for this project; nothing here calls the library."""
import numpy as np

from motion_ref import mat_to_quat, quat_normalize, quat_to_mat

COV_X_2, COV_Q_2, COV_V_2, COV_W_2, COV_A_2 = 0.0025, 0.00001, 0.000625, 0.000625, 0.000625
SIGMA_X, SIGMA_Q, SIGMA_V, SIGMA_W = 0.05, 0.02, 4.0, 6.0
SIGMA_GYRO, SIGMA_ACC = 2.60, 8.94
SEL = [0, 1, 2, 3, 4, 5, 6, 10, 11, 12, 13, 14, 15]      # the row of X each measurement observes (IMU::jH)


def quat_mul(a, b):
    """Eigen's quaternion product, (w, x, y, z)."""
    return np.array([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3],
                     a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                     a[0] * b[2] + a[2] * b[0] + a[3] * b[1] - a[1] * b[3],
                     a[0] * b[3] + a[3] * b[0] + a[1] * b[2] - a[2] * b[1]], dtype=np.result_type(a, b))


def quat_from_angular_velocity(w):
    """Sensor::QuaternionFromAngularVelocity: the rotation by the vector w (already multiplied by the time)."""
    dt = w.dtype.type
    angle = np.sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2])
    if angle > 0:
        s = np.sin(angle / dt(2)) / angle
        return np.array([np.cos(angle / dt(2)), s * w[0], s * w[1], s * w[2]], dtype=w.dtype)
    return np.array([1, 0, 0, 0], dtype=w.dtype)


def quat_jacobian(q):
    w, x, y, z = q
    return np.array([[w, -x, -y, -z], [x, w, z, -y], [y, -z, w, x], [z, y, -x, w]], dtype=q.dtype)


def quat_jacobian_right(q):
    w, x, y, z = q
    return np.array([[w, -x, -y, -z], [x, w, -z, y], [y, z, w, -x], [z, -y, x, w]], dtype=q.dtype)


def dq_by_dw(q, w, time):
    """Sensor::dq_by_dw; the |w| == 0 branch is not multiplied by QuaternionJacobianRight(q), as in the reference."""
    dt = w.dtype.type
    time = dt(time)
    modw = np.sqrt(w[0] * w[0] + w[1] * w[1] + w[2] * w[2])
    beta = modw * time / dt(2)
    res = np.zeros((4, 3), w.dtype)
    if modw == 0:
        res[1:, :] = np.eye(3, dtype=w.dtype) * time / dt(2)
        return res
    sb, cb, m2, ht = np.sin(beta), np.cos(beta), modw * modw, time / dt(2)
    mdw = np.zeros((4, 3), w.dtype)
    for c in range(3):
        mdw[0, c] = -ht * sb * w[c] / modw
    for r in range(3):
        for c in range(3):
            if r == c:
                mdw[1 + r, c] = ht * cb * (w[r] * w[r]) / m2 + sb / modw * (dt(1) - (w[r] * w[r]) / m2)
            else:
                mdw[1 + r, c] = (w[r] * w[c] / m2) * (ht * cb - sb / modw)
    return quat_jacobian_right(q) @ mdw


def get_pose(X):
    """Sensor::GetPose: the rotation of a normalised copy of q, and x."""
    pose = np.eye(4)
    pose[:3, :3] = quat_to_mat(quat_normalize(np.asarray(X[3:7], np.float64)))
    pose[:3, 3] = np.asarray(X[:3], np.float64)
    return pose


def pose_to_vector(pose):
    """Sensor::PoseToVector: (x, normalised q of the rotation)."""
    pose = np.asarray(pose, np.float64)
    return np.concatenate([pose[:3, 3], quat_normalize(mat_to_quat(pose[:3, :3]))])


def inverse(S):
    if S.dtype == np.float64:
        return np.linalg.inv(S)
    X = np.linalg.inv(S.astype(np.float64)).astype(S.dtype)
    two = 2 * np.eye(len(S), dtype=S.dtype)
    for _ in range(4):
        X = X @ (two - S @ X)
    return X


class EKF:
    """EKF over the IMU sensor, one camera stream."""

    def __init__(self, dtype=np.float64):
        self.dtype = dtype
        self.X = np.zeros(16, dtype)
        self.P = np.zeros((16, 16), dtype)
        self.gravity = np.zeros(3, dtype)
        self.it_time = 0.0
        self.last_pose = np.zeros((4, 4))
        self.restart()

    def started(self):
        return self.updated

    def restart(self):
        """EKF::Restart -> IMU::Init: X, the diagonal blocks of P, gravity_."""
        d = self.dtype
        self.updated = False
        self.X[:] = 0
        self.X[3] = 1
        for lo, hi, c in ((0, 3, COV_X_2), (3, 7, COV_Q_2), (7, 10, COV_V_2), (10, 13, COV_W_2), (13, 16, COV_A_2)):
            self.P[lo:hi, lo:hi] = np.eye(hi - lo, dtype=d) * d(c)
        self.gravity[:] = 0

    def jF(self, time):
        d = self.dtype
        t = d(time)
        q, w = self.X[3:7], self.X[10:13]
        J = np.eye(16, dtype=d)
        J[0:3, 7:10] = np.eye(3, dtype=d) * t
        J[7:10, 13:16] = np.eye(3, dtype=d) * t
        J[3:7, 3:7] = quat_jacobian(quat_from_angular_velocity(w * t))
        J[3:7, 10:13] = dq_by_dw(q, w, t)
        return J

    def Q(self, time):
        d = self.dtype
        t = d(time)
        q, w = self.X[3:7], self.X[10:13]
        Pn = np.zeros((9, 9), d)
        Pn[0:3, 0:3] = np.eye(3, dtype=d) * d(SIGMA_V) * d(SIGMA_V) * t * t
        Pn[3:6, 3:6] = np.eye(3, dtype=d) * d(SIGMA_W) * d(SIGMA_W) * t * t
        Pn[6:9, 6:9] = np.eye(3, dtype=d) * d(SIGMA_ACC) * d(SIGMA_ACC) * t * t
        G = np.zeros((16, 9), d)
        G[0:3, 0:3] = np.eye(3, dtype=d) * t
        G[7:10, 0:3] = np.eye(3, dtype=d)
        G[7:10, 6:9] = np.eye(3, dtype=d) * t
        G[10:13, 3:6] = np.eye(3, dtype=d)
        G[13:16, 6:9] = np.eye(3, dtype=d)
        G[3:7, 3:6] = dq_by_dw(q, w, t)
        return G @ Pn @ G.T

    def F(self, time):
        t = self.dtype(time)
        X = self.X.copy()
        x, q, v, w, a = X[0:3], X[3:7], X[7:10], X[10:13], X[13:16]
        self.X[0:3] = x + v * t
        self.X[3:7] = quat_mul(q, quat_from_angular_velocity(w * t))
        self.X[7:10] = v + a * t

    def predict(self, pose, dt):
        """EKF::Predict for a started filter; the last pose for one that is not (see the module docstring)."""
        self.last_pose = np.array(pose, np.float64)
        if not self.updated:
            self.it_time = 0.0
            return self.last_pose.copy()
        self.it_time = float(dt)
        jF, Q = self.jF(self.it_time), self.Q(self.it_time)
        self.F(self.it_time)
        self.P = jF @ self.P @ jF.T + Q
        return get_pose(self.X)

    def update_gravity(self, a, time):
        d = self.dtype
        alpha = d(0.27) / (d(0.27) + d(time))
        self.gravity = alpha * self.gravity + (d(1) - alpha) * a

    def update(self, pose, meas):
        """EKF::Update(pose, params): params = (gyro xyz, accelerometer xyz)."""
        d = self.dtype
        meas = np.asarray(meas, np.float64).astype(d)
        assert meas.shape == (6,)
        t = d(self.it_time)
        self.update_gravity(meas[3:], t)                               # IMU::Z updates gravity first
        Z = np.concatenate([pose_to_vector(pose).astype(d), meas[:3], meas[3:] - self.gravity])
        if not self.updated:
            self.X[:] = 0                                              # IMU::InitState
            self.X[:7] = Z[:7]
            self.gravity[:] = 0
        else:
            jH = np.zeros((13, 16), d)
            jH[np.arange(13), SEL] = 1
            H = self.X[SEL]
            R = np.zeros((13, 13), d)
            for lo, hi, s in ((0, 3, SIGMA_X), (3, 7, SIGMA_Q), (7, 10, SIGMA_GYRO), (10, 13, SIGMA_ACC)):
                R[lo:hi, lo:hi] = np.eye(hi - lo, dtype=d) * d(s) * d(s) * t * t
            Y = Z - H                                                  # quaternions subtracted componentwise
            S = jH @ self.P @ jH.T + R
            K = self.P @ jH.T @ inverse(S)
            self.X = self.X + K @ Y
            self.P = self.P - K @ S @ K.T                              # no symmetrisation
        self.updated = True

    def track(self, pose, meas, tracked=True):
        if tracked and not (np.abs(self.last_pose) <= 1e-12).all():      # Matrix4d::isZero()
            self.update(pose, meas)
        else:
            self.restart()
