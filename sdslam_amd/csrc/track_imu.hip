// IMU sensor model of sequential tracking on the device: the 16-state EKF of Monocular-IMU tracking as per-slot state of the
// tracker (reference src/sensors/EKF.cc:44-109, src/sensors/IMU.cc:26-240, src/sensors/Sensor.cc:24-159), the second of the
// reference's two motion models (Tracking picks its Sensor at construction, src/Tracking.cc:134-138):
//   motion_model_->Predict(mLastFrame.GetPose())             src/Tracking.cc:661     -> k_imu_predict
//   motion_model_->Update(pose, measurements_)               src/Tracking.cc:243-247 -> k_imu_update
//   motion_model_->Restart()                                 src/Tracking.cc:221, :226, :247 -> k_imu_update / k_imu_init
//
// State X = (x 3, q 4 as w x y z, v 3, w 3, a 3), measurements Z = (x 3, q 4, gyro 3, accelerometer - gravity 3).  P is a dense
// 16 x 16, jF and Q depend on X through dq_by_dw, every update inverts the dense 13 x 13 S.  Unlike ConstantVelocity nothing
// here is diagonal, so this is small dense linear algebra per slot:
//  * one wavefront (one 64-lane workgroup) per slot; P and the working matrices live in the workgroup's LDS, every lane owns
//    fixed output entries of each product (entry e = lane + 64 k).  The barriers are those of a single-wave workgroup.
//  * lane 0 does the scalar part (quaternion algebra, dq_by_dw, Z, gravity) with compile-time indices, in registers.
//  * jH selects rows {0..6, 10..15} of X: jH P jH^T is exactly that sub-block of P (products with 1, sums with 0), P jH^T those
//    columns.  jF and G are stored dense and multiplied dense: the exact zeros add nothing, the sums run k = 0.. in order.
//  * S^-1 by Gauss-Jordan on [S | I] with partial pivoting; the pivot search is a wave reduction (largest |entry|, lowest row
//    on a tie).  A singular S gives inf / nan, as a division by zero does in the reference.
// Quirks of the reference that are kept: P = P - (K S) K^T without symmetrisation; Y = Z - h(X) subtracts the quaternions
// componentwise; R = sigma^2 time^2, so a zero time gives S = the sub-block of P; Z() low-passes gravity before InitState
// zeroes it on the first update; Restart = IMU::Init assigns only the diagonal blocks of P; GetPose normalises a copy of q and the state's q is never normalised; in dq_by_dw the |w| == 0
// branch is NOT multiplied by QuaternionJacobianRight(q); QuaternionFromAngularVelocity branches on angle > 0.
// dt replaces the wall-clock timer_ as in track_motion.hip.  A slot that is not started is not predicted at all (the reference
// never calls Predict for it: it runs TrackReferenceKeyFrame from the last pose): Tprior = Tcur = Tref bit for bit, X and P
// untouched, it_time = 0 (EKF::Predict's own value for a filter that is not started), last_pose = Tref.
#include <hip/hip_runtime.h>

#include "orb_internal.h"
#include "sd_quat.h"
#include "track_internal.h"

namespace sd {

static constexpr double IM_COV_X_2 = 0.0025, IM_COV_Q_2 = 0.00001, IM_COV_V_2 = 0.000625, IM_COV_W_2 = 0.000625;   // Sensor::COV_*
static constexpr double IM_COV_A_2 = 0.000625;                                                                     // IMU::COV_A_2
static constexpr double IM_SIGMA_X = 0.05, IM_SIGMA_Q = 0.02, IM_SIGMA_V = 4.0, IM_SIGMA_W = 6.0;                  // Sensor::SIGMA_*
static constexpr double IM_SIGMA_GYRO = 2.60, IM_SIGMA_ACC = 8.94;                                                 // IMU::SIGMA_*

// row of X that measurement m observes (IMU::jH)
__device__ __forceinline__ int im_sel(int m) { return m < 7 ? m : m + 3; }

// IMU::Init diagonal of P
__device__ __forceinline__ double im_p0(int i) {
  return i < 3 ? IM_COV_X_2 : (i < 7 ? IM_COV_Q_2 : (i < 10 ? IM_COV_V_2 : (i < 13 ? IM_COV_W_2 : IM_COV_A_2)));
}

// IMU::R diagonal entry m at `time`: sigma * sigma * time * time, left to right
__device__ __forceinline__ double im_r(int m, double time) {
  const double s = m < 3 ? IM_SIGMA_X : (m < 7 ? IM_SIGMA_Q : (m < 10 ? IM_SIGMA_GYRO : IM_SIGMA_ACC));
  return s * s * time * time;
}

// the block of X (x, q, v, w, a) that row i belongs to
__device__ __forceinline__ int im_block(int i) { return i < 3 ? 0 : (i < 7 ? 1 : (i < 10 ? 2 : (i < 13 ? 3 : 4))); }

// EKF::Restart of slot f by the 64 lanes of its wave: IMU::Init (X, P, gravity_), updated_ = false.  IMU::Init assigns the five
// diagonal blocks of P only, so a restarted filter keeps the off-diagonal blocks it had; `full` also zeroes those, which is
// EKF's constructor (P_.setZero() before Init).
__device__ __forceinline__ void im_restart(const TrackBuffers& tb, int f, int lane, bool full) {
  double* P = tb.im_P + (size_t)f * 256;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const int e = lane + 64 * k, i = e >> 4, j = e & 15;
    if (full || im_block(i) == im_block(j)) P[e] = i == j ? im_p0(i) : 0.0;
  }
  if (lane < 16) tb.im_X[(size_t)f * 16 + lane] = lane == 3 ? 1.0 : 0.0;
  if (lane < 3) tb.im_g[(size_t)f * 3 + lane] = 0.0;
  if (lane == 0) tb.im_started[f] = 0;
}

// Sensor::QuaternionFromAngularVelocity
__device__ __forceinline__ void im_quat_from_w(const double (&w)[3], double (&q)[4]) {
  const double angle = sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]);
  if (angle > 0.0) {
    const double s = sin(angle / 2.0) / angle;
    q[0] = cos(angle / 2.0);
    q[1] = s * w[0]; q[2] = s * w[1]; q[3] = s * w[2];
  } else {
    q[0] = 1.0; q[1] = 0.0; q[2] = 0.0; q[3] = 0.0;
  }
}

// Sensor::dq_by_dw(q, w, time), 4 x 3
__device__ __forceinline__ void im_dq_by_dw(const double (&q)[4], const double (&w)[3], double time, double (&res)[4][3]) {
  const double modw = sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]);   // Vector3d::norm()
  const double beta = modw * time / 2.0;
  if (modw == 0.0) {
#pragma unroll
    for (int r = 0; r < 4; r++)
#pragma unroll
      for (int c = 0; c < 3; c++) res[r][c] = r == c + 1 ? time / 2.0 : 0.0;
    return;
  }
  const double sb = sin(beta), cb = cos(beta), m2 = modw * modw, ht = time / 2.0;
  double mdw[4][3];
#pragma unroll
  for (int c = 0; c < 3; c++) mdw[0][c] = -ht * sb * w[c] / modw;
#pragma unroll
  for (int r = 0; r < 3; r++)
#pragma unroll
    for (int c = 0; c < 3; c++) {
      if (r == c) mdw[1 + r][c] = ht * cb * (w[r] * w[r]) / m2 + sb / modw * (1.0 - (w[r] * w[r]) / m2);
      else mdw[1 + r][c] = (w[r] * w[c] / m2) * (ht * cb - sb / modw);
    }
  // Sensor::QuaternionJacobianRight(q) * mdw
  const double qw = q[0], qx = q[1], qy = q[2], qz = q[3];
  const double J[4][4] = {{qw, -qx, -qy, -qz}, {qx, qw, -qz, qy}, {qy, qz, qw, -qx}, {qz, -qy, qx, qw}};
#pragma unroll
  for (int r = 0; r < 4; r++)
#pragma unroll
    for (int c = 0; c < 3; c++) res[r][c] = ((J[r][0] * mdw[0][c] + J[r][1] * mdw[1][c]) + J[r][2] * mdw[2][c]) + J[r][3] * mdw[3][c];
}

// Eigen::Quaterniond(Matrix3d) and normalize() on the rotation of a column-major pose
__device__ __forceinline__ void im_pose_quat(const double (&T)[16], double (&q)[4]) {
  const double m[3][3] = {{T[0], T[4], T[8]}, {T[1], T[5], T[9]}, {T[2], T[6], T[10]}};
  mat_to_quat(m, q[0], q[1], q[2], q[3]);
  quat_normalize(q[0], q[1], q[2], q[3]);
}

// EKF::Restart (full 0) or a newly constructed EKF (full 1) for slots frame0 .. frame0 + n - 1, one wave per slot
__global__ __launch_bounds__(64) void k_imu_init(TrackBuffers tb, int frame0, int n, int full) {
  if ((int)blockIdx.x >= n) return;
  im_restart(tb, frame0 + blockIdx.x, threadIdx.x, full != 0);
}

// EKF::Predict(Tref) for slot blockIdx.x < n.  Not started: last_pose = Tprior = Tcur = Tref, it_time = 0.  Started: it_time =
// dt; jF, Q on the old X; X = F(X); P = jF P jF^T + Q; Tprior = Tcur = Sensor::GetPose(X).
__global__ __launch_bounds__(64) void k_imu_predict(TrackBuffers tb, int n, double dt) {
  __shared__ double sP[256], sF[256], sA[256], sG[16 * 9];
  const int f = blockIdx.x, lane = threadIdx.x;
  if (f >= n) return;
  const bool started = tb.im_started[f] != 0;   // wave-uniform
  if (lane < 16) {
    const double v = tb.Tref[(size_t)f * 16 + lane];
    tb.im_last[(size_t)f * 16 + lane] = v;
    if (!started) {
      tb.Tprior[(size_t)f * 16 + lane] = v;
      tb.Tcur[(size_t)f * 16 + lane] = v;
    }
  }
  if (lane == 0) tb.im_it[f] = started ? dt : 0.0;
  if (!started) return;
  double* gP = tb.im_P + (size_t)f * 256;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const int e = lane + 64 * k;
    sP[e] = gP[e];
    sF[e] = (e >> 4) == (e & 15) ? 1.0 : 0.0;
  }
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const int e = lane + 64 * k;
    if (e < 144) sG[e] = 0.0;
  }
  __syncthreads();
  if (lane == 0) {
    double X[16];
#pragma unroll
    for (int i = 0; i < 16; i++) X[i] = tb.im_X[(size_t)f * 16 + i];
    const double q[4] = {X[3], X[4], X[5], X[6]}, w[3] = {X[10], X[11], X[12]};
    const double wt[3] = {w[0] * dt, w[1] * dt, w[2] * dt};
    double qwt[4], D[4][3];
    im_quat_from_w(wt, qwt);
    im_dq_by_dw(q, w, dt, D);
    // jF: I, I * time at (0, 7) and (7, 13), Sensor::QuaternionJacobian(qwt) at (3, 3), dq_by_dw at (3, 10)
    const double J[4][4] = {{qwt[0], -qwt[1], -qwt[2], -qwt[3]}, {qwt[1], qwt[0], qwt[3], -qwt[2]},
                            {qwt[2], -qwt[3], qwt[0], qwt[1]}, {qwt[3], qwt[2], -qwt[1], qwt[0]}};
#pragma unroll
    for (int r = 0; r < 3; r++) {
      sF[r * 16 + 7 + r] = dt;
      sF[(7 + r) * 16 + 13 + r] = dt;
      // G: I * time at (0, 0) and (7, 6), I at (7, 0), (10, 3), (13, 6), dq_by_dw at (3, 3)
      sG[r * 9 + r] = dt;
      sG[(7 + r) * 9 + r] = 1.0;
      sG[(7 + r) * 9 + 6 + r] = dt;
      sG[(10 + r) * 9 + 3 + r] = 1.0;
      sG[(13 + r) * 9 + 6 + r] = 1.0;
    }
#pragma unroll
    for (int r = 0; r < 4; r++) {
#pragma unroll
      for (int c = 0; c < 4; c++) sF[(3 + r) * 16 + 3 + c] = J[r][c];
#pragma unroll
      for (int c = 0; c < 3; c++) {
        sF[(3 + r) * 16 + 10 + c] = D[r][c];
        sG[(3 + r) * 9 + 3 + c] = D[r][c];
      }
    }
    // IMU::F: x += v t; q = q * qwt (Eigen's quaternion product); v += a t
    double Xn[16];
#pragma unroll
    for (int i = 0; i < 3; i++) {
      Xn[i] = X[i] + X[7 + i] * dt;
      Xn[7 + i] = X[7 + i] + X[13 + i] * dt;
      Xn[10 + i] = X[10 + i];
      Xn[13 + i] = X[13 + i];
    }
    Xn[3] = q[0] * qwt[0] - q[1] * qwt[1] - q[2] * qwt[2] - q[3] * qwt[3];
    Xn[4] = q[0] * qwt[1] + q[1] * qwt[0] + q[2] * qwt[3] - q[3] * qwt[2];
    Xn[5] = q[0] * qwt[2] + q[2] * qwt[0] + q[3] * qwt[1] - q[1] * qwt[3];
    Xn[6] = q[0] * qwt[3] + q[3] * qwt[0] + q[1] * qwt[2] - q[2] * qwt[1];
#pragma unroll
    for (int i = 0; i < 16; i++) tb.im_X[(size_t)f * 16 + i] = Xn[i];
    // Sensor::GetPose: the rotation of a normalised copy of q, column-major
    double pw = Xn[3], px = Xn[4], py = Xn[5], pz = Xn[6], R[3][3];
    quat_normalize(pw, px, py, pz);
    quat_to_mat(pw, px, py, pz, R);
    const double T[16] = {R[0][0], R[1][0], R[2][0], 0.0, R[0][1], R[1][1], R[2][1], 0.0,
                          R[0][2], R[1][2], R[2][2], 0.0, Xn[0], Xn[1], Xn[2], 1.0};
#pragma unroll
    for (int i = 0; i < 16; i++) {
      tb.Tprior[(size_t)f * 16 + i] = T[i];
      tb.Tcur[(size_t)f * 16 + i] = T[i];
    }
  }
  __syncthreads();
  // A = jF * P
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const int e = lane + 64 * k, i = e >> 4, j = e & 15;
    double acc = 0.0;
    for (int m = 0; m < 16; m++) acc += sF[i * 16 + m] * sP[m * 16 + j];
    sA[e] = acc;
  }
  __syncthreads();
  // P = A * jF^T + (G * P_n) * G^T, P_n = diag(SIGMA_V^2 t^2 x3, SIGMA_W^2 t^2 x3, SIGMA_ACC^2 t^2 x3)
  const double pn0 = IM_SIGMA_V * IM_SIGMA_V * dt * dt, pn1 = IM_SIGMA_W * IM_SIGMA_W * dt * dt, pn2 = IM_SIGMA_ACC * IM_SIGMA_ACC * dt * dt;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const int e = lane + 64 * k, i = e >> 4, j = e & 15;
    double acc = 0.0, qq = 0.0;
    for (int m = 0; m < 16; m++) acc += sA[i * 16 + m] * sF[j * 16 + m];
    for (int m = 0; m < 9; m++) qq += (sG[i * 9 + m] * (m < 3 ? pn0 : (m < 6 ? pn1 : pn2))) * sG[j * 9 + m];
    gP[e] = acc + qq;
  }
}

// src/Tracking.cc:243-247 and the Restart() of :221 / :226 for slot blockIdx.x < n.  Tracked (source -1: always; 0: tw_info
// status 2; 1: tl_info status 2) and last_pose not zero: EKF::Update(Tcur, measurements); otherwise EKF::Restart.
__global__ __launch_bounds__(64) void k_imu_update(TrackBuffers tb, int n, int source) {
  __shared__ double sP[256], sS[169], sM[13 * 26], sK[208], sKS[208], sY[13], sCol[13];
  const int f = blockIdx.x, lane = threadIdx.x;
  if (f >= n) return;
  const bool tracked = slot_tracked(tb, source, f);
  const bool nz = lane < 16 && !(fabs(tb.im_last[(size_t)f * 16 + lane]) <= 1e-12);   // !Matrix4d::isZero()
  if (!tracked || __ballot(nz) == 0ull) {
    im_restart(tb, f, lane, false);
    return;
  }
  const bool started = tb.im_started[f] != 0;   // wave-uniform
  const double it = tb.im_it[f];
  if (lane == 0) {
    // IMU::Z: UpdateGravity first, then (x, normalised q of the pose, w, a - gravity_)
    double T[16], Z[13], g[3];
#pragma unroll
    for (int i = 0; i < 16; i++) T[i] = tb.Tcur[(size_t)f * 16 + i];
    const double alpha = 0.27 / (0.27 + it);
#pragma unroll
    for (int i = 0; i < 3; i++) {
      const double a = tb.im_meas[(size_t)f * 6 + 3 + i];
      g[i] = alpha * tb.im_g[(size_t)f * 3 + i] + (1.0 - alpha) * a;
      Z[i] = T[12 + i];
      Z[7 + i] = tb.im_meas[(size_t)f * 6 + i];
      Z[10 + i] = a - g[i];
    }
    double q[4];
    im_pose_quat(T, q);
#pragma unroll
    for (int i = 0; i < 4; i++) Z[3 + i] = q[i];
    if (!started) {   // IMU::InitState: X = 0, the pose part of Z, gravity_ = 0
#pragma unroll
      for (int i = 0; i < 16; i++) tb.im_X[(size_t)f * 16 + i] = i < 7 ? Z[i] : 0.0;
#pragma unroll
      for (int i = 0; i < 3; i++) tb.im_g[(size_t)f * 3 + i] = 0.0;
      tb.im_started[f] = 1;
    } else {
#pragma unroll
      for (int i = 0; i < 3; i++) tb.im_g[(size_t)f * 3 + i] = g[i];
#pragma unroll
      for (int m = 0; m < 13; m++) sY[m] = Z[m] - tb.im_X[(size_t)f * 16 + (m < 7 ? m : m + 3)];   // Y = Z - h(X)
    }
  }
  if (!started) return;
  double* gP = tb.im_P + (size_t)f * 256;
#pragma unroll
  for (int k = 0; k < 4; k++) sP[lane + 64 * k] = gP[lane + 64 * k];
  __syncthreads();
  // S = jH P jH^T + R; the working copy [S | I]
#pragma unroll
  for (int k = 0; k < 3; k++) {
    const int e = lane + 64 * k;
    if (e < 169) {
      const int a = e / 13, b = e - a * 13;
      const double v = sP[im_sel(a) * 16 + im_sel(b)] + (a == b ? im_r(a, it) : 0.0);
      sS[e] = v;
      sM[a * 26 + b] = v;
      sM[a * 26 + 13 + b] = a == b ? 1.0 : 0.0;
    }
  }
  __syncthreads();
  // Gauss-Jordan with partial pivoting: after step c column c of the left half is e_c
  for (int c = 0; c < 13; c++) {
    double best = lane >= c && lane < 13 ? fabs(sM[lane * 26 + c]) : -1.0;
    int row = lane;
#pragma unroll
    for (int o = 8; o >= 1; o >>= 1) {
      const double ob = __shfl_xor(best, o);
      const int orow = __shfl_xor(row, o);
      if (ob > best || (ob == best && orow < row)) { best = ob; row = orow; }
    }
    int p = __shfl(row, 0);
    if (p < c || p > 12) p = c;   // only when the column holds a nan: stay inside the matrix
    if (p != c && lane < 26) {
      const double a = sM[c * 26 + lane], b = sM[p * 26 + lane];
      sM[c * 26 + lane] = b;
      sM[p * 26 + lane] = a;
    }
    __syncthreads();
    const double piv = sM[c * 26 + c];
    if (lane < 13) sCol[lane] = sM[lane * 26 + c];
    __syncthreads();
    if (lane < 26) sM[c * 26 + lane] = sM[c * 26 + lane] / piv;
    __syncthreads();
#pragma unroll
    for (int k = 0; k < 6; k++) {
      const int e = lane + 64 * k;
      if (e < 338) {
        const int r = e / 26, j = e - r * 26;
        if (r != c) sM[e] = sM[e] - sCol[r] * sM[c * 26 + j];
      }
    }
    __syncthreads();
  }
  // K = (P jH^T) S^-1, 16 x 13
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const int e = lane + 64 * k;
    if (e < 208) {
      const int i = e / 13, m = e - i * 13;
      double acc = 0.0;
      for (int a = 0; a < 13; a++) acc += sP[i * 16 + im_sel(a)] * sM[a * 26 + 13 + m];
      sK[e] = acc;
    }
  }
  __syncthreads();
  // K S, and X = X + K Y
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const int e = lane + 64 * k;
    if (e < 208) {
      const int i = e / 13, m = e - i * 13;
      double acc = 0.0;
      for (int a = 0; a < 13; a++) acc += sK[i * 13 + a] * sS[a * 13 + m];
      sKS[e] = acc;
    }
  }
  if (lane < 16) {
    double acc = 0.0;
    for (int a = 0; a < 13; a++) acc += sK[lane * 13 + a] * sY[a];
    tb.im_X[(size_t)f * 16 + lane] = tb.im_X[(size_t)f * 16 + lane] + acc;
  }
  __syncthreads();
  // P = P - (K S) K^T
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const int e = lane + 64 * k, i = e >> 4, j = e & 15;
    double acc = 0.0;
    for (int a = 0; a < 13; a++) acc += sKS[i * 13 + a] * sK[j * 13 + a];
    gP[e] = sP[e] - acc;
  }
}

int launch_imu_init(const TrackBuffers& tb, int frame0, int n_frames, int full, hipStream_t s) {
  hipLaunchKernelGGL(k_imu_init, dim3(n_frames), dim3(64), 0, s, tb, frame0, n_frames, full);
  SD_HIP_CHECK(hipGetLastError());
  return SD_OK;
}

int launch_imu_predict(const TrackBuffers& tb, int n_frames, double dt, hipStream_t s) {
  hipLaunchKernelGGL(k_imu_predict, dim3(n_frames), dim3(64), 0, s, tb, n_frames, dt);
  SD_HIP_CHECK(hipGetLastError());
  return SD_OK;
}

int launch_imu_update(const TrackBuffers& tb, int n_frames, int source, hipStream_t s) {
  hipLaunchKernelGGL(k_imu_update, dim3(n_frames), dim3(64), 0, s, tb, n_frames, source);
  SD_HIP_CHECK(hipGetLastError());
  return SD_OK;
}

}  // namespace sd
