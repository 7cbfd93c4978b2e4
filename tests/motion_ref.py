"""Numpy float64 restatement of the reference's motion model (helper, no tests): EKF (src/sensors/EKF.cc) in its dense 6x6
matrix form with Predict / Update / Restart, and ConstantVelocity (src/sensors/ConstantVelocity.cc; constants
src/sensors/Sensor.cc:24-32) with Exp / Log / RotationExp / RotationLog and the two conversions the reference takes from
Eigen (matrix -> quaternion, quaternion -> matrix).  The dense form is deliberate: the device keeps only the diagonal of P
and runs six scalar filters, and the comparison against this file checks that the two are the same filter.  `dt` stands for
the reference's wall-clock timer.  Written for this project; nothing here calls the library."""
import math

import numpy as np

SMALL_EPS = 1e-10
COV_V_2 = 0.000625
COV_W_2 = 0.000625
SIGMA_V = 4.0
SIGMA_W = 6.0


def mat_to_quat(m):
    """Eigen::Quaterniond(Matrix3d): (w, x, y, z)."""
    q = [0.0, 0.0, 0.0]
    t = m[0, 0] + m[1, 1] + m[2, 2]
    if t > 0.0:
        t = math.sqrt(t + 1.0)
        w = 0.5 * t
        t = 0.5 / t
        q[0] = (m[2, 1] - m[1, 2]) * t
        q[1] = (m[0, 2] - m[2, 0]) * t
        q[2] = (m[1, 0] - m[0, 1]) * t
    else:
        i = 0
        if m[1, 1] > m[0, 0]:
            i = 1
        if m[2, 2] > m[i, i]:
            i = 2
        j = (i + 1) % 3
        k = (j + 1) % 3
        t = math.sqrt(m[i, i] - m[j, j] - m[k, k] + 1.0)
        q[i] = 0.5 * t
        t = 0.5 / t
        w = (m[k, j] - m[j, k]) * t
        q[j] = (m[j, i] + m[i, j]) * t
        q[k] = (m[k, i] + m[i, k]) * t
    return np.array([w, q[0], q[1], q[2]])


def quat_to_mat(q):
    """QuaternionBase::toRotationMatrix()."""
    w, x, y, z = (float(v) for v in q)
    tx, ty, tz = 2.0 * x, 2.0 * y, 2.0 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return np.array([[1.0 - (tyy + tzz), txy - twz, txz + twy],
                     [txy + twz, 1.0 - (txx + tzz), tyz - twx],
                     [txz - twy, tyz + twx, 1.0 - (txx + tyy)]])


def quat_normalize(q):
    w, x, y, z = (float(v) for v in q)
    n2 = ((x * x + y * y) + z * z) + w * w
    if n2 > 0.0:
        return np.array([w, x, y, z]) / math.sqrt(n2)
    return np.array([w, x, y, z])


def hat(v):
    return np.array([[0.0, -v[2], v[1]], [v[2], 0.0, -v[0]], [-v[1], v[0], 0.0]])


def rotation_exp(omega):
    theta = math.sqrt((omega[0] * omega[0] + omega[1] * omega[1]) + omega[2] * omega[2])
    half_theta = 0.5 * theta
    real_factor = math.cos(half_theta)
    if theta < SMALL_EPS:
        theta_sq = theta * theta
        theta_po4 = theta_sq * theta_sq
        imag_factor = 0.5 - 0.0208333 * theta_sq + 0.000260417 * theta_po4
    else:
        imag_factor = math.sin(half_theta) / theta
    return np.array([real_factor, imag_factor * omega[0], imag_factor * omega[1], imag_factor * omega[2]]), theta


def rotation_log(q):
    n = math.sqrt((q[1] * q[1] + q[2] * q[2]) + q[3] * q[3])
    w = float(q[0])
    squared_w = w * w
    if n < SMALL_EPS:
        f = 2.0 / w - 2.0 * (n * n) / (w * squared_w)
    else:
        if abs(w) < SMALL_EPS:
            f = math.pi / n if w > 0 else -math.pi / n
        ratio = n / w if w != 0.0 else math.copysign(math.inf, w)       # IEEE division, as the C++ performs it
        f = 2.0 * math.atan(ratio) / n                                  # unconditional: overwrites the branch above
    return f * np.asarray(q[1:4], np.float64), f * n


def exp(update):
    update = np.asarray(update, np.float64)
    upsilon, omega = update[:3], update[3:]
    q, theta = rotation_exp(omega)
    Omega = hat(omega)
    Omega_sq = Omega @ Omega
    if theta < SMALL_EPS:
        V = quat_to_mat(q)
    else:
        theta_sq = theta * theta
        V = np.eye(3) + (1.0 - math.cos(theta)) / theta_sq * Omega + (theta - math.sin(theta)) / (theta_sq * theta) * Omega_sq
    pose = np.eye(4)
    pose[:3, :3] = quat_to_mat(quat_normalize(q))
    pose[:3, 3] = V @ upsilon
    return pose


def log(pose):
    pose = np.asarray(pose, np.float64)
    q = quat_normalize(mat_to_quat(pose[:3, :3]))
    omega, theta = rotation_log(q)
    Omega = hat(omega)
    if theta < SMALL_EPS:
        V_inv = np.eye(3) - 0.5 * Omega + (1.0 / 12.0) * (Omega @ Omega)
    else:
        V_inv = np.eye(3) - 0.5 * Omega + (1.0 - theta / (2.0 * math.tan(theta / 2.0))) / (theta * theta) * (Omega @ Omega)
    return np.concatenate([V_inv @ pose[:3, 3], omega])


def prior_product(V, L):
    """V @ L summed k = 0..3 in order, every product and sum rounded on its own (the device's product)."""
    P = V[:, 0:1] * L[0:1, :]
    for k in range(1, 4):
        P = P + V[:, k:k + 1] * L[k:k + 1, :]
    return P


def noise(time):
    """ConstantVelocity::Q / R at `time`."""
    Q = np.zeros((6, 6))
    Q[:3, :3] = np.eye(3) * SIGMA_V * SIGMA_V * time * time
    Q[3:, 3:] = np.eye(3) * SIGMA_W * SIGMA_W * time * time
    return Q


class EKF:
    """EKF over the ConstantVelocity sensor, one camera stream."""

    def __init__(self):
        self.X = np.zeros(6)
        self.P = np.zeros((6, 6))
        self.it_time = 0.0
        self.last_pose = np.zeros((4, 4))
        self.E = np.zeros((4, 4))
        self.restart()

    def started(self):
        return self.updated

    def restart(self):
        """EKF::Restart -> ConstantVelocity::Init: X and the two diagonal blocks of P."""
        self.updated = False
        self.X[:] = 0.0
        self.P[:3, :3] = np.eye(3) * COV_V_2
        self.P[3:, 3:] = np.eye(3) * COV_W_2

    def predict(self, pose, dt):
        self.it_time = float(dt) if self.updated else 0.0
        self.last_pose = np.array(pose, np.float64)
        jF = np.eye(6)
        self.P = jF @ self.P @ jF.T + noise(self.it_time)
        self.E = exp(self.X)
        return prior_product(self.E, self.last_pose)

    def update(self, pose):
        pose = np.asarray(pose, np.float64)
        rot = self.last_pose[:3, :3].T
        last_i = np.eye(4)
        last_i[:3, :3] = rot
        last_i[:3, 3] = -(rot @ self.last_pose[:3, 3])
        Z = log(pose @ last_i)
        if not self.updated:
            self.X[:] = 0.0                            # ConstantVelocity::InitState ignores Z
        else:
            jH = np.eye(6)
            S = jH @ self.P @ jH.T + noise(self.it_time)
            K = self.P @ jH.T @ np.linalg.inv(S)
            self.X = self.X + K @ (Z - self.X)
            self.P = self.P - K @ S @ K.T
        self.updated = True

    def track(self, pose, tracked=True):
        """src/Tracking.cc:243-247 with the Restart() of :221 / :226 for a frame that was not tracked."""
        if tracked and not (np.abs(self.last_pose) <= 1e-12).all():      # Matrix4d::isZero()
            self.update(pose)
        else:
            self.restart()
