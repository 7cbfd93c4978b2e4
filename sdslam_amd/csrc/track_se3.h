// SE3Quat of g2o (types/se3quat.h) on the device: quaternion (x, y, z, w) and translation, with the Eigen 3.3 pieces it uses
// restated (oracle/src/poseopt_oracle.cc holds the host restatement).  Shared by k_pose_opt (track_poseopt.hip) and the local
// bundle adjustment (track_ba.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace sd {

struct Se3q {
  double q[4];   // x, y, z, w
  double t[3];
};

__device__ __forceinline__ void q_normalize(double* q) {
  if (q[3] < 0)
    for (int i = 0; i < 4; i++) q[i] *= -1;
  const double n = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  for (int i = 0; i < 4; i++) q[i] /= n;
}

__device__ __forceinline__ void q_from_R(const double m[3][3], double* q) {   // Eigen QuaternionBase::operator=(MatrixBase)
  double t = m[0][0] + m[1][1] + m[2][2];
  if (t > 0) {
    t = sqrt(t + 1.0);
    q[3] = 0.5 * t;
    t = 0.5 / t;
    q[0] = (m[2][1] - m[1][2]) * t;
    q[1] = (m[0][2] - m[2][0]) * t;
    q[2] = (m[1][0] - m[0][1]) * t;
  } else {
    // i = index of the largest diagonal entry, written without run-time indexing
    const bool i1 = m[1][1] > m[0][0];
    const bool i2 = m[2][2] > (i1 ? m[1][1] : m[0][0]);
    if (i2) {          // i = 2, j = 0, k = 1
      t = sqrt(m[2][2] - m[0][0] - m[1][1] + 1.0);
      q[2] = 0.5 * t;
      t = 0.5 / t;
      q[3] = (m[1][0] - m[0][1]) * t;
      q[0] = (m[0][2] + m[2][0]) * t;
      q[1] = (m[1][2] + m[2][1]) * t;
    } else if (i1) {   // i = 1, j = 2, k = 0
      t = sqrt(m[1][1] - m[2][2] - m[0][0] + 1.0);
      q[1] = 0.5 * t;
      t = 0.5 / t;
      q[3] = (m[0][2] - m[2][0]) * t;
      q[2] = (m[2][1] + m[1][2]) * t;
      q[0] = (m[0][1] + m[1][0]) * t;
    } else {           // i = 0, j = 1, k = 2
      t = sqrt(m[0][0] - m[1][1] - m[2][2] + 1.0);
      q[0] = 0.5 * t;
      t = 0.5 / t;
      q[3] = (m[2][1] - m[1][2]) * t;
      q[1] = (m[1][0] + m[0][1]) * t;
      q[2] = (m[2][0] + m[0][2]) * t;
    }
  }
}

__device__ __forceinline__ void q_mul(const double* a, const double* b, double* r) {
  const double w = a[3] * b[3] - a[0] * b[0] - a[1] * b[1] - a[2] * b[2];
  const double x = a[3] * b[0] + a[0] * b[3] + a[1] * b[2] - a[2] * b[1];
  const double y = a[3] * b[1] + a[1] * b[3] + a[2] * b[0] - a[0] * b[2];
  const double z = a[3] * b[2] + a[2] * b[3] + a[0] * b[1] - a[1] * b[0];
  r[0] = x; r[1] = y; r[2] = z; r[3] = w;
}

__device__ __forceinline__ void q_rotate(const double* q, const double* v, double* r) {
  double uv[3] = {q[1] * v[2] - q[2] * v[1], q[2] * v[0] - q[0] * v[2], q[0] * v[1] - q[1] * v[0]};
  for (int i = 0; i < 3; i++) uv[i] += uv[i];
  const double c[3] = {q[1] * uv[2] - q[2] * uv[1], q[2] * uv[0] - q[0] * uv[2], q[0] * uv[1] - q[1] * uv[0]};
  for (int i = 0; i < 3; i++) r[i] = v[i] + q[3] * uv[i] + c[i];
}

__device__ __forceinline__ Se3q se3_from_Rt(const double R[3][3], const double* t) {
  Se3q s;
  q_from_R(R, s.q);
  for (int i = 0; i < 3; i++) s.t[i] = t[i];
  q_normalize(s.q);
  return s;
}

__device__ __forceinline__ Se3q se3q_mul(const Se3q& a, const Se3q& b) {
  Se3q r = a;
  double rt[3];
  q_rotate(a.q, b.t, rt);
  for (int i = 0; i < 3; i++) r.t[i] += rt[i];
  q_mul(a.q, b.q, r.q);
  q_normalize(r.q);
  return r;
}

__device__ __noinline__ Se3q se3q_exp(const double* update) {   // SE3Quat::exp
  const double omega[3] = {update[0], update[1], update[2]}, upsilon[3] = {update[3], update[4], update[5]};
  const double theta = sqrt(omega[0] * omega[0] + omega[1] * omega[1] + omega[2] * omega[2]);
  const double Om[3][3] = {{0, -omega[2], omega[1]}, {omega[2], 0, -omega[0]}, {-omega[1], omega[0], 0}};
  double Om2[3][3], R[3][3], V[3][3];
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) Om2[i][j] = Om[i][0] * Om[0][j] + Om[i][1] * Om[1][j] + Om[i][2] * Om[2][j];
  if (theta < 0.00001) {
    for (int i = 0; i < 3; i++)
      for (int j = 0; j < 3; j++) V[i][j] = R[i][j] = ((i == j ? 1.0 : 0.0) + Om[i][j]) + Om2[i][j];
  } else {
    const double a = sin(theta) / theta, b = (1 - cos(theta)) / (theta * theta), c = (theta - sin(theta)) / pow(theta, 3.0);
    for (int i = 0; i < 3; i++)
      for (int j = 0; j < 3; j++) {
        R[i][j] = ((i == j ? 1.0 : 0.0) + a * Om[i][j]) + b * Om2[i][j];
        V[i][j] = ((i == j ? 1.0 : 0.0) + b * Om[i][j]) + c * Om2[i][j];
      }
  }
  double t[3];
  for (int i = 0; i < 3; i++) t[i] = V[i][0] * upsilon[0] + V[i][1] * upsilon[1] + V[i][2] * upsilon[2];
  return se3_from_Rt(R, t);
}

}  // namespace sd
