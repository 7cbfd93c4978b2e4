// The quaternion conversions the reference's sensor models take from Eigen, written out: one operation sequence for both
// filters (track_motion.hip, track_imu.hip), every product and sum in Eigen's order.
#pragma once
#include <hip/hip_runtime.h>

namespace sd {

// Eigen::Quaterniond(Matrix3d) (Eigen/src/Geometry/Quaternion.h, quaternionbase_assign_impl<Other, 3, 3>); m row-major [r][c]
__device__ __forceinline__ void mat_to_quat(const double (&m)[3][3], double& w, double& x, double& y, double& z) {
  double t = m[0][0] + m[1][1] + m[2][2];
  if (t > 0.0) {
    t = sqrt(t + 1.0);
    w = 0.5 * t;
    t = 0.5 / t;
    x = (m[2][1] - m[1][2]) * t;
    y = (m[0][2] - m[2][0]) * t;
    z = (m[1][0] - m[0][1]) * t;
  } else if (m[2][2] > (m[1][1] > m[0][0] ? m[1][1] : m[0][0])) {   // i = 2, j = 0, k = 1
    t = sqrt(m[2][2] - m[0][0] - m[1][1] + 1.0);
    z = 0.5 * t;
    t = 0.5 / t;
    w = (m[1][0] - m[0][1]) * t;
    x = (m[0][2] + m[2][0]) * t;
    y = (m[1][2] + m[2][1]) * t;
  } else if (m[1][1] > m[0][0]) {                                   // i = 1, j = 2, k = 0
    t = sqrt(m[1][1] - m[2][2] - m[0][0] + 1.0);
    y = 0.5 * t;
    t = 0.5 / t;
    w = (m[0][2] - m[2][0]) * t;
    z = (m[2][1] + m[1][2]) * t;
    x = (m[0][1] + m[1][0]) * t;
  } else {                                                          // i = 0, j = 1, k = 2
    t = sqrt(m[0][0] - m[1][1] - m[2][2] + 1.0);
    x = 0.5 * t;
    t = 0.5 / t;
    w = (m[2][1] - m[1][2]) * t;
    y = (m[1][0] + m[0][1]) * t;
    z = (m[2][0] + m[0][2]) * t;
  }
}

// QuaternionBase::toRotationMatrix()
__device__ __forceinline__ void quat_to_mat(double w, double x, double y, double z, double (&r)[3][3]) {
  const double tx = 2.0 * x, ty = 2.0 * y, tz = 2.0 * z;
  const double twx = tx * w, twy = ty * w, twz = tz * w;
  const double txx = tx * x, txy = ty * x, txz = tz * x;
  const double tyy = ty * y, tyz = tz * y, tzz = tz * z;
  r[0][0] = 1.0 - (tyy + tzz);
  r[0][1] = txy - twz;
  r[0][2] = txz + twy;
  r[1][0] = txy + twz;
  r[1][1] = 1.0 - (txx + tzz);
  r[1][2] = tyz - twx;
  r[2][0] = txz - twy;
  r[2][1] = tyz + twx;
  r[2][2] = 1.0 - (txx + tyy);
}

// QuaternionBase::normalize(): coefficients / sqrt(squaredNorm), left alone for a zero quaternion
__device__ __forceinline__ void quat_normalize(double& w, double& x, double& y, double& z) {
  const double n2 = ((x * x + y * y) + z * z) + w * w;   // coefficient order x, y, z, w
  if (n2 > 0.0) {
    const double n = sqrt(n2);
    w /= n; x /= n; y /= n; z /= n;
  }
}

}  // namespace sd
