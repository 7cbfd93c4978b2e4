// Motion model of sequential tracking on the device: EKF + ConstantVelocity as per-slot state of the tracker
// (reference src/sensors/EKF.cc, src/sensors/ConstantVelocity.cc, constants src/sensors/Sensor.cc:24-32), so the prior of
// every frame comes from the poses the slots obtained, without a host round trip:
//   motion_model_->Predict(mLastFrame.GetPose())           src/Tracking.cc:661   -> k_motion_predict
//   motion_model_->Update(mCurrentFrame.GetPose(), ...)    src/Tracking.cc:243-247 -> k_motion_update
//   motion_model_->Restart()                               src/Tracking.cc:221, :226, :247 -> k_motion_update / k_motion_init
//
// Facts of the reference that shape these kernels:
//  * jF = jH = G = I, and Q, R and the initial P are diagonal.  P, S = P + R and K = P * S^-1 therefore stay exactly diagonal
//    in the reference's dense 6x6 products (every off-diagonal term is a sum of products with an exact zero), so the filter is
//    six independent scalar filters.  Only the diagonal of P is stored.
//  * Eigen's S.inverse() of a diagonal matrix is 1 / s_i, so k_i = p_i * (1 / s_i), x_i += k_i * (z_i - x_i),
//    p_i -= (k_i * s_i) * k_i -- in that association, K * S first.
//  * Exp / Log / RotationExp / RotationLog keep the reference's branches and its quirks: SMALL_EPS = 1e-10; below it the Taylor
//    imag_factor 0.5 - 0.0208333 t^2 + 0.000260417 t^4 and V = toRotationMatrix() of the NOT yet normalised quaternion;
//    q.normalize() before the final toRotationMatrix(); in RotationLog the unconditional 2 * atan(n / w) / n that overwrites
//    what the |w| < SMALL_EPS branch computed, so a negative w gives a negative theta and Log then takes its small-angle V_inv
//    (theta < SMALL_EPS holds for every negative theta).
//  * The two conversions the reference takes from Eigen are written out in sd_quat.h (mat_to_quat, quat_to_mat).
//  * Tracking.cc:244 tests mLastFrame.GetPose().isZero(): Eigen's default precision, every |entry| <= 1e-12.  The pose read is
//    the one Predict stored (SetLastPose), which is mLastFrame's.
//  * dt replaces the reference's wall-clock timer_ (Stop() in Predict, Start() in Update): one double per call, the same for
//    every slot of the step -- the batch advances in lock-step.  Per-slot timestamps are not supported.
//
// One lane per slot, everything in registers: all 3x3 / 4x4 loops are unrolled with compile-time indices.  The trigonometry is
// the device library's double-precision sin / cos / atan / tan / sqrt.  Not here: which slots run TrackReferenceKeyFrame
// instead (not started, mnLastRelocFrameId), its retry after a failed TrackWithMotionModel, and relocalisation -- the statuses
// that name those slots stay with the caller.  A slot that is not started gets Exp(0) = I and so Tprior = Tref bit for bit:
// the pose TrackReferenceKeyFrame starts from.
#include <hip/hip_runtime.h>

#include "orb_internal.h"
#include "sd_quat.h"
#include "track_internal.h"

namespace sd {

static constexpr double MO_SMALL_EPS = 1e-10;
static constexpr double MO_COV_V_2 = 0.000625, MO_COV_W_2 = 0.000625;   // Sensor::COV_V_2, COV_W_2
static constexpr double MO_SIGMA_V = 4.0, MO_SIGMA_W = 6.0;             // Sensor::SIGMA_V, SIGMA_W

// ConstantVelocity::Q / R diagonal entry i at `time`: Identity * SIGMA * SIGMA * time * time, left to right
__device__ __forceinline__ double mo_noise(int i, double time) {
  const double s = i < 3 ? MO_SIGMA_V : MO_SIGMA_W;
  return s * s * time * time;
}

// ConstantVelocity::Init: X = 0, the diagonal of P to its initial values (the off-diagonals are never written: exactly 0)
__device__ __forceinline__ void mo_restart(const TrackBuffers& tb, int f) {
  tb.mo_started[f] = 0;
#pragma unroll
  for (int i = 0; i < 6; i++) {
    tb.mo_X[(size_t)f * 6 + i] = 0.0;
    tb.mo_P[(size_t)f * 6 + i] = i < 3 ? MO_COV_V_2 : MO_COV_W_2;
  }
}

// ConstantVelocity::RotationHat and its square, row-major
__device__ __forceinline__ void mo_hat(const double (&v)[3], double (&O)[3][3], double (&O2)[3][3]) {
  O[0][0] = 0.0;   O[0][1] = -v[2]; O[0][2] = v[1];
  O[1][0] = v[2];  O[1][1] = 0.0;   O[1][2] = -v[0];
  O[2][0] = -v[1]; O[2][1] = v[0];  O[2][2] = 0.0;
#pragma unroll
  for (int r = 0; r < 3; r++)
#pragma unroll
    for (int c = 0; c < 3; c++) O2[r][c] = (O[r][0] * O[0][c] + O[r][1] * O[1][c]) + O[r][2] * O[2][c];
}

// ConstantVelocity::Exp (src/sensors/ConstantVelocity.cc:161-189) with RotationExp (:213-229); E column-major 4x4
__device__ __forceinline__ void mo_exp(const double (&X)[6], double (&E)[16]) {
  const double ups[3] = {X[0], X[1], X[2]}, om[3] = {X[3], X[4], X[5]};
  const double theta = sqrt((om[0] * om[0] + om[1] * om[1]) + om[2] * om[2]);
  const double half_theta = 0.5 * theta;
  double imag;
  double qw = cos(half_theta);
  if (theta < MO_SMALL_EPS) {
    const double theta_sq = theta * theta, theta_po4 = theta_sq * theta_sq;
    imag = (0.5 - 0.0208333 * theta_sq) + 0.000260417 * theta_po4;
  } else {
    imag = sin(half_theta) / theta;
  }
  double qx = imag * om[0], qy = imag * om[1], qz = imag * om[2];
  double O[3][3], O2[3][3], V[3][3];
  mo_hat(om, O, O2);
  if (theta < MO_SMALL_EPS) {
    quat_to_mat(qw, qx, qy, qz, V);
  } else {
    const double theta_sq = theta * theta;
    const double a = (1.0 - cos(theta)) / theta_sq, b = (theta - sin(theta)) / (theta_sq * theta);
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
      for (int c = 0; c < 3; c++) V[r][c] = ((r == c ? 1.0 : 0.0) + a * O[r][c]) + b * O2[r][c];
  }
  double R[3][3];
  quat_normalize(qw, qx, qy, qz);
  quat_to_mat(qw, qx, qy, qz, R);
#pragma unroll
  for (int r = 0; r < 3; r++) {
#pragma unroll
    for (int c = 0; c < 3; c++) E[c * 4 + r] = R[r][c];
    E[12 + r] = (V[r][0] * ups[0] + V[r][1] * ups[1]) + V[r][2] * ups[2];
    E[r * 4 + 3] = 0.0;
  }
  E[15] = 1.0;
}

// ConstantVelocity::Log (:191-211) with RotationLog (:239-263) of the pose whose rows 0..2 are S (row-major 3x4)
__device__ __forceinline__ void mo_log(const double (&S)[3][4], double (&Z)[6]) {
  const double rot[3][3] = {{S[0][0], S[0][1], S[0][2]}, {S[1][0], S[1][1], S[1][2]}, {S[2][0], S[2][1], S[2][2]}};
  double w, x, y, z;
  mat_to_quat(rot, w, x, y, z);
  quat_normalize(w, x, y, z);
  const double n = sqrt((x * x + y * y) + z * z);
  double f;
  if (n < MO_SMALL_EPS) f = 2.0 / w - 2.0 * (n * n) / (w * (w * w));
  else f = 2.0 * atan(n / w) / n;   // also for |w| < SMALL_EPS: the reference overwrites that branch's +-pi / n
  const double theta = f * n;
  const double om[3] = {f * x, f * y, f * z};
  double O[3][3], O2[3][3];
  mo_hat(om, O, O2);
  // theta < SMALL_EPS includes every negative theta (w < 0)
  const double c2 = theta < MO_SMALL_EPS ? 1.0 / 12.0 : (1.0 - theta / (2.0 * tan(theta / 2.0))) / (theta * theta);
#pragma unroll
  for (int r = 0; r < 3; r++) {
    double vi[3];
#pragma unroll
    for (int c = 0; c < 3; c++) vi[c] = ((r == c ? 1.0 : 0.0) - 0.5 * O[r][c]) + c2 * O2[r][c];
    Z[r] = (vi[0] * S[0][3] + vi[1] * S[1][3]) + vi[2] * S[2][3];
    Z[3 + r] = om[r];
  }
}

// EKF::Restart for slots frame0 .. frame0 + n - 1 (a new handle, sd_track_motion_restart)
__global__ __launch_bounds__(64) void k_motion_init(TrackBuffers tb, int frame0, int n) {
  const int t = blockIdx.x * 64 + threadIdx.x;
  if (t >= n) return;
  mo_restart(tb, frame0 + t);
}

// EKF::Predict(Tref) (src/sensors/EKF.cc:44-66) for slots < n: it_time = updated ? dt : 0; last_pose = Tref; P += Q(it_time);
// E = Exp(X); Tprior = Tcur = E * Tref through k_set_prior's product.  Tref is left alone.
__global__ __launch_bounds__(64) void k_motion_predict(TrackBuffers tb, int n, double dt) {
  const int f = blockIdx.x * 64 + threadIdx.x;
  if (f >= n) return;
  const double it = tb.mo_started[f] ? dt : 0.0;
  tb.mo_it[f] = it;
  double L[16], X[6], E[16];
#pragma unroll
  for (int i = 0; i < 16; i++) L[i] = tb.Tref[(size_t)f * 16 + i];
#pragma unroll
  for (int i = 0; i < 16; i++) tb.mo_last[(size_t)f * 16 + i] = L[i];
#pragma unroll
  for (int i = 0; i < 6; i++) {
    X[i] = tb.mo_X[(size_t)f * 6 + i];
    tb.mo_P[(size_t)f * 6 + i] = tb.mo_P[(size_t)f * 6 + i] + mo_noise(i, it);
  }
  mo_exp(X, E);
#pragma unroll
  for (int c = 0; c < 4; c++)
#pragma unroll
    for (int r = 0; r < 4; r++) {
      const double v = pose_product_entry(E, L, r, c);
      tb.mo_E[(size_t)f * 16 + c * 4 + r] = E[c * 4 + r];
      tb.Tprior[(size_t)f * 16 + c * 4 + r] = v;
      tb.Tcur[(size_t)f * 16 + c * 4 + r] = v;
    }
}

// src/Tracking.cc:243-247 and the Restart() of :221 / :226 for slots < n.  Tracked (source -1: always; 0: tw_info status 2;
// 1: tl_info status 2) and last_pose not zero: EKF::Update(Tcur) (src/sensors/EKF.cc:68-104) with Z = Log(Tcur *
// inverse(last_pose)) (ConstantVelocity::Z, :105-122); otherwise EKF::Restart.
__global__ __launch_bounds__(64) void k_motion_update(TrackBuffers tb, int n, int source) {
  const int f = blockIdx.x * 64 + threadIdx.x;
  if (f >= n) return;
  const bool tracked = slot_tracked(tb, source, f);
  double L[16];
  bool zero = true;
#pragma unroll
  for (int i = 0; i < 16; i++) {
    L[i] = tb.mo_last[(size_t)f * 16 + i];
    zero = zero && fabs(L[i]) <= 1e-12;   // Matrix4d::isZero()
  }
  if (!tracked || zero) {
    mo_restart(tb, f);
    return;
  }
  if (!tb.mo_started[f]) {   // ConstantVelocity::InitState ignores Z
#pragma unroll
    for (int i = 0; i < 6; i++) tb.mo_X[(size_t)f * 6 + i] = 0.0;
    tb.mo_started[f] = 1;
    return;
  }
  // last_pose_i: rot = R^T, t = -(rot * t_last), bottom row of the identity
  double Li[3][4];
#pragma unroll
  for (int r = 0; r < 3; r++) {
#pragma unroll
    for (int c = 0; c < 3; c++) Li[r][c] = L[r * 4 + c];   // (R^T)[r][c] = R[c][r] = L[r * 4 + c]
    Li[r][3] = -((Li[r][0] * L[12] + Li[r][1] * L[13]) + Li[r][2] * L[14]);
  }
  // se3 = pose * last_pose_i, rows 0..2; the k = 3 terms multiply the exact 0 / 1 of last_pose_i's bottom row
  double T[16], S[3][4], Z[6];
#pragma unroll
  for (int i = 0; i < 16; i++) T[i] = tb.Tcur[(size_t)f * 16 + i];
#pragma unroll
  for (int r = 0; r < 3; r++) {
#pragma unroll
    for (int c = 0; c < 3; c++) S[r][c] = (T[r] * Li[0][c] + T[4 + r] * Li[1][c]) + T[8 + r] * Li[2][c];
    S[r][3] = ((T[r] * Li[0][3] + T[4 + r] * Li[1][3]) + T[8 + r] * Li[2][3]) + T[12 + r];
  }
  mo_log(S, Z);
  const double it = tb.mo_it[f];
#pragma unroll
  for (int i = 0; i < 6; i++) {
    const double x = tb.mo_X[(size_t)f * 6 + i], p = tb.mo_P[(size_t)f * 6 + i];
    const double s = p + mo_noise(i, it);
    const double k = p * (1.0 / s);
    tb.mo_X[(size_t)f * 6 + i] = x + k * (Z[i] - x);
    tb.mo_P[(size_t)f * 6 + i] = p - (k * s) * k;
  }
}

int launch_motion_init(const TrackBuffers& tb, int frame0, int n_frames, hipStream_t s) {
  hipLaunchKernelGGL(k_motion_init, dim3((n_frames + 63) / 64), dim3(64), 0, s, tb, frame0, n_frames);
  SD_HIP_CHECK(hipGetLastError());
  return SD_OK;
}

int launch_motion_predict(const TrackBuffers& tb, int n_frames, double dt, hipStream_t s) {
  hipLaunchKernelGGL(k_motion_predict, dim3((n_frames + 63) / 64), dim3(64), 0, s, tb, n_frames, dt);
  SD_HIP_CHECK(hipGetLastError());
  return SD_OK;
}

int launch_motion_update(const TrackBuffers& tb, int n_frames, int source, hipStream_t s) {
  hipLaunchKernelGGL(k_motion_update, dim3((n_frames + 63) / 64), dim3(64), 0, s, tb, n_frames, source);
  SD_HIP_CHECK(hipGetLastError());
  return SD_OK;
}

}  // namespace sd
