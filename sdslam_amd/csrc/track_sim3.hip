// Sim3Solver (Horn RANSAC between two keyframes' map points) on MI355X, one wavefront per loop candidate.
//
// Replaces SD_SLAM::Sim3Solver (reference src/Sim3Solver.cc) in full: the constructor's gather (:59-101), SetRansacParameters
// (:112-135), iterate / find (:137-203), ComputeCentroid / ComputeSim3 (:205-318), CheckInliers (:321-341), Project /
// FromCameraToImage (:356-393), the three getters (:344-354), and SD_SLAM::Random (src/extra/utils.cc:23-26).  Its one caller is
// LoopClosing::ComputeSim3 (src/LoopClosing.cc:255-283), right after ORBmatcher::SearchByPoints (track_bf.hip), whose match
// vector this kernel reads where that one left it.
//
// Parallel shape (that of k_pnp): the three draws of an iteration depend only on the rand() stream, so up to 64 consecutive
// iterations are evaluated with one lane each (Horn's closed form: fp64 centroids and M, OpenCV 3.2's float Jacobi on the 4x4 N,
// fp64 Rodrigues); CheckInliers then goes hypothesis by hypothesis with the lanes over the correspondences (T12 / T21 broadcast
// from the owning lane, the mask kept as ballots, the count as popcounts), and the reference's sequential best-so-far / early
// return logic runs in iteration order between them.  An iteration consumes exactly 3 rand() values, so the stream position
// is 3 * mnIterations.  The numeric definitions (which operations are float, which double, and their order) are DESIGN.md §3.
//
// Host side at the end of the file: the five sd_track_* entry points.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <climits>
#include <cmath>

#include "sd_wave.h"
#include "track_handle.h"

namespace sd {

#define S3_MAXN 2048            // = the tracker's keypoint capacity limit (sd_track_create)
#define S3_WORDS (S3_MAXN / 64)   // ballots per inlier mask: word b lives in lane b

// value of lane `src` (wave-uniform) in every lane
__device__ __forceinline__ double s3_bcast(double v, int src) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), src), hi = __builtin_amdgcn_readlane(__double2hiint(v), src);
  return __hiloint2double(hi, lo);
}

// SD_SLAM::Random(0, size - 1) from one raw rand() value
__device__ __forceinline__ int s3_random(int r, int size) { return (int)(((double)r / ((double)RAND_MAX + 1.0)) * (double)size + 0.0); }

// ---- cv::eigen on a symmetric 4x4 CV_32F matrix = OpenCV 3.2 JacobiImpl_<float> (modules/core/src/lapack.cpp): the pivot is
// the largest off-diagonal of the upper triangle found through the per-row / per-column maxima indR / indC (strict `<`, so the
// first of equals wins; only the two touched indices are refreshed after a rotation), rotations in its order, at most n*n*30
// sweeps, stop at |p| <= FLT_EPSILON.  All indices are compile-time after unrolling (the pivot dispatches to one of six
// instantiations), so A, V, W, indR, indC stay in registers.
__device__ __forceinline__ float s3_hypot(float a, float b) {   // cv's own template, not libm
  a = fabsf(a);
  b = fabsf(b);
  if (a > b) {
    b /= a;
    return a * sqrtf(1 + b * b);
  }
  if (b > 0) {
    a /= b;
    return b * sqrtf(1 + a * a);
  }
  return 0;
}

struct S3Jacobi {
  float A[4][4], V[4][4], W[4];
  int indR[4], indC[4];
};

template <int IDX>
__device__ __forceinline__ void s3_refresh(S3Jacobi& J) {
  if (IDX < 3) {
    int m = IDX + 1;
    float mv = fabsf(J.A[IDX][IDX + 1 < 4 ? IDX + 1 : 3]);
#pragma unroll
    for (int i = IDX + 2; i < 4; i++) {
      const float val = fabsf(J.A[IDX][i]);
      if (mv < val) mv = val, m = i;
    }
    J.indR[IDX] = m;
  }
  if (IDX > 0) {
    int m = 0;
    float mv = fabsf(J.A[0][IDX]);
#pragma unroll
    for (int i = 1; i < IDX; i++) {
      const float val = fabsf(J.A[i][IDX]);
      if (mv < val) mv = val, m = i;
    }
    J.indC[IDX] = m;
  }
}

#define S3_ROT(v0, v1)          \
  {                             \
    const float a0 = v0, b0 = v1; \
    v0 = a0 * c - b0 * s;       \
    v1 = a0 * s + b0 * c;       \
  }

template <int K, int L>
__device__ __forceinline__ void s3_rotate(S3Jacobi& J) {
  const float p = J.A[K][L];
  const float y = (float)((J.W[L] - J.W[K]) * 0.5);
  float t = fabsf(y) + s3_hypot(p, y);
  float s = s3_hypot(p, t);
  const float c = t / s;
  s = p / s;
  t = (p / t) * p;
  if (y < 0) s = -s, t = -t;
  J.A[K][L] = 0;
  J.W[K] -= t;
  J.W[L] += t;
#pragma unroll
  for (int i = 0; i < K; i++) S3_ROT(J.A[i][K], J.A[i][L]);
#pragma unroll
  for (int i = K + 1; i < L; i++) S3_ROT(J.A[K][i], J.A[i][L]);
#pragma unroll
  for (int i = L + 1; i < 4; i++) S3_ROT(J.A[K][i], J.A[L][i]);
#pragma unroll
  for (int i = 0; i < 4; i++) S3_ROT(J.V[K][i], J.V[L][i]);
  s3_refresh<K>(J);
  s3_refresh<L>(J);
}

// element j (runtime, 0..3) of a register row
__device__ __forceinline__ float s3_pick(const float (&r)[4], int j) { return j == 0 ? r[0] : (j == 1 ? r[1] : (j == 2 ? r[2] : r[3])); }

// evec.row(0) of cv::eigen(N): the eigenvector of the largest eigenvalue (the descending sort's first pass: strict `<`, the
// first of equal eigenvalues stays in front)
__device__ __forceinline__ void s3_eigen_top(const float (&N)[4][4], float (&q)[4]) {
  S3Jacobi J;
#pragma unroll
  for (int i = 0; i < 4; i++) {
#pragma unroll
    for (int j = 0; j < 4; j++) {
      J.A[i][j] = N[i][j];
      J.V[i][j] = i == j ? 1.f : 0.f;
    }
    J.W[i] = N[i][i];
  }
  J.indR[3] = 3;
  J.indC[0] = 0;
  s3_refresh<0>(J);
  s3_refresh<1>(J);
  s3_refresh<2>(J);
  s3_refresh<3>(J);
  for (int iters = 0; iters < 4 * 4 * 30; iters++) {
    int k = 0;
    float mv = fabsf(s3_pick(J.A[0], J.indR[0]));
#pragma unroll
    for (int i = 1; i < 3; i++) {
      const float val = fabsf(s3_pick(J.A[i], J.indR[i]));
      if (mv < val) mv = val, k = i;
    }
    int l = k == 0 ? J.indR[0] : (k == 1 ? J.indR[1] : J.indR[2]);
#pragma unroll
    for (int i = 1; i < 4; i++) {
      const int r = J.indC[i];
      const float val = fabsf(r == 0 ? J.A[0][i] : (r == 1 ? J.A[1][i] : J.A[2][i]));
      if (mv < val) mv = val, k = r, l = i;
    }
    if (mv <= FLT_EPSILON) break;   // |p| <= eps (mv = |p|)
    switch (k * 4 + l) {
      case 1: s3_rotate<0, 1>(J); break;
      case 2: s3_rotate<0, 2>(J); break;
      case 3: s3_rotate<0, 3>(J); break;
      case 6: s3_rotate<1, 2>(J); break;
      case 7: s3_rotate<1, 3>(J); break;
      default: s3_rotate<2, 3>(J); break;
    }
  }
  int m = 0;
  float wm = J.W[0];
#pragma unroll
  for (int i = 1; i < 4; i++)
    if (wm < J.W[i]) wm = J.W[i], m = i;
#pragma unroll
  for (int j = 0; j < 4; j++) q[j] = m == 0 ? J.V[0][j] : (m == 1 ? J.V[1][j] : (m == 2 ? J.V[2][j] : J.V[3][j]));
}

// One hypothesis: what ComputeSim3 leaves in mR12i, ms12i, mt12i, mT12i, mT21i.  Matrices row-major [r * 3 + c].
struct S3Hyp {
  double R[9], sR[9], t[3], sRi[9], ti[3];
  float s;
};

// P1 / P2: the three drawn points as columns, [r][c] = coordinate r of draw c
__device__ __forceinline__ void s3_compute_sim3(const double (&P1)[3][3], const double (&P2)[3][3], int fix_scale, S3Hyp& H) {
  // Step 1 (ComputeCentroid): Eigen's unrolled row sum of three is a0 + (a1 + a2); then / 3
  double O1[3], O2[3], Pr1[3][3], Pr2[3][3];
#pragma unroll
  for (int r = 0; r < 3; r++) {
    O1[r] = (P1[r][0] + (P1[r][1] + P1[r][2])) / 3.0;
    O2[r] = (P2[r][0] + (P2[r][1] + P2[r][2])) / 3.0;
#pragma unroll
    for (int c = 0; c < 3; c++) {
      Pr1[r][c] = P1[r][c] - O1[r];
      Pr2[r][c] = P2[r][c] - O2[r];
    }
  }
  // Step 2: M = Pr2 * Pr1^T
  double M[3][3];
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) M[i][j] = (Pr2[i][0] * Pr1[j][0] + Pr2[i][1] * Pr1[j][1]) + Pr2[i][2] * Pr1[j][2];
  // Step 3: N, converted to float by Converter::toCvMat
  const double N11 = M[0][0] + M[1][1] + M[2][2], N12 = M[1][2] - M[2][1], N13 = M[2][0] - M[0][2], N14 = M[0][1] - M[1][0];
  const double N22 = M[0][0] - M[1][1] - M[2][2], N23 = M[0][1] + M[1][0], N24 = M[2][0] + M[0][2];
  const double N33 = -M[0][0] + M[1][1] - M[2][2], N34 = M[1][2] + M[2][1], N44 = -M[0][0] - M[1][1] + M[2][2];
  const float Nf[4][4] = {{(float)N11, (float)N12, (float)N13, (float)N14},
                          {(float)N12, (float)N22, (float)N23, (float)N24},
                          {(float)N13, (float)N23, (float)N33, (float)N34},
                          {(float)N14, (float)N24, (float)N34, (float)N44}};
  // Step 4: quaternion -> angle-axis (float) -> cv::Rodrigues (double) -> CV_32F
  float q[4];
  s3_eigen_top(Nf, q);
  double nrm2 = 0.0;
#pragma unroll
  for (int i = 1; i < 4; i++) nrm2 += (double)q[i] * (double)q[i];
  const double nrm = sqrt(nrm2);                       // cv::norm of a CV_32F row accumulates in double
  const double ang = atan2(nrm, (double)q[0]);
  const float alpha = (float)((2 * ang) * (1. / nrm));   // MatExpr: scalar * vec / scalar folds into one float scale
  double rx = (double)(q[1] * alpha), ry = (double)(q[2] * alpha), rz = (double)(q[3] * alpha);
  const double theta = sqrt(rx * rx + ry * ry + rz * rz);
  double Rd[9];
  if (theta < DBL_EPSILON) {
#pragma unroll
    for (int k = 0; k < 9; k++) Rd[k] = (k % 4 == 0) ? 1.0 : 0.0;
  } else {
    const double c = cos(theta), s = sin(theta), c1 = 1. - c, itheta = theta ? 1. / theta : 0.;
    rx *= itheta;
    ry *= itheta;
    rz *= itheta;
    const double rrt[9] = {rx * rx, rx * ry, rx * rz, rx * ry, ry * ry, ry * rz, rx * rz, ry * rz, rz * rz};
    const double rxm[9] = {0, -rz, ry, rz, 0, -rx, -ry, rx, 0};
#pragma unroll
    for (int k = 0; k < 9; k++) Rd[k] = (c * ((k % 4 == 0) ? 1.0 : 0.0) + c1 * rrt[k]) + s * rxm[k];
  }
#pragma unroll
  for (int k = 0; k < 9; k++) H.R[k] = (double)(float)Rd[k];
  // Step 5: P3 = R * Pr2
  double P3[3][3];
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) P3[i][j] = (H.R[i * 3] * Pr2[0][j] + H.R[i * 3 + 1] * Pr2[1][j]) + H.R[i * 3 + 2] * Pr2[2][j];
  // Step 6: scale.  nom = cv::Mat::dot of the float-converted matrices (double accumulator, four products per step in
  // row-major element order); den = the plain double loop
  if (!fix_scale) {
    double pr[9], den = 0.0;
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
      for (int j = 0; j < 3; j++) {
        pr[i * 3 + j] = (double)(float)Pr1[i][j] * (double)(float)P3[i][j];
        den += P3[i][j] * P3[i][j];
      }
    double nom = 0.0;
    nom += ((pr[0] + pr[1]) + pr[2]) + pr[3];
    nom += ((pr[4] + pr[5]) + pr[6]) + pr[7];
    nom += pr[8];
    H.s = (float)(nom / den);
  } else {
    H.s = 1.0f;
  }
  // Steps 7, 8 (order fixed in DESIGN.md §3)
  const double sd = (double)H.s, si = 1.0 / sd;
#pragma unroll
  for (int k = 0; k < 9; k++) H.sR[k] = sd * H.R[k];
#pragma unroll
  for (int i = 0; i < 3; i++) H.t[i] = O1[i] - ((H.sR[i * 3] * O2[0] + H.sR[i * 3 + 1] * O2[1]) + H.sR[i * 3 + 2] * O2[2]);
#pragma unroll
  for (int i = 0; i < 3; i++)
#pragma unroll
    for (int j = 0; j < 3; j++) H.sRi[i * 3 + j] = si * H.R[j * 3 + i];
#pragma unroll
  for (int i = 0; i < 3; i++) H.ti[i] = ((-H.sRi[i * 3]) * H.t[0] + (-H.sRi[i * 3 + 1]) * H.t[1]) + (-H.sRi[i * 3 + 2]) * H.t[2];
}

// Project / FromCameraToImage (:356-393) of the camera-frame point (x, y, z): invz, x, y are float, fx * x + cx is a float
// expression (all operands float) that the Vector2d then holds as a double
__device__ __forceinline__ void s3_to_image(double x, double y, double z, const TrackCam& cam, float* u, float* v) {
  const float invz = (float)(1 / z);
  const float xf = (float)(x * (double)invz);
  const float yf = (float)(y * (double)invz);
  *u = cam.ffx * xf + cam.fcx;
  *v = cam.ffy * yf + cam.fcy;
}

__global__ __launch_bounds__(64) void k_sim3(const sd_keypoint* __restrict__ kps1_all, const int32_t* __restrict__ n1_all,
                                             const sd_keypoint* __restrict__ kps2_all, const int32_t* __restrict__ n2_all, TrackBuffers tb,
                                             TrackCam cam, const float* __restrict__ sigma2, int nlevels,
                                             const int32_t* __restrict__ max_its_tab, Sim3Params sp) {
  const int f = blockIdx.x, lane = threadIdx.x;
  const unsigned long long lt = lanemask_lt(lane);
  const int K = tb.kp_cap;
  const size_t fK = (size_t)f * K;
  double* __restrict__ GX = tb.s3_X + fK * 6;
  float* __restrict__ GF = tb.s3_F + fK * 6;
  uint16_t* __restrict__ gidx = tb.s3_idx + fK;
  int32_t* st = tb.s3_state + (size_t)f * 8;
  uint8_t* inl_out = tb.s3_inliers + fK;
  double* T_out = tb.s3_T + (size_t)f * 16;

  // iterate(): vbInliers = vector<bool>(mN1, false), the returned matrix defaults to Zero()
  for (int i = lane; i < K; i += 64) inl_out[i] = 0;
  if (lane < 16) T_out[lane] = 0.0;

  int N, max_its, its, best;
  unsigned long long best_mask = 0;
  if (!sp.resume) {
    // ---- constructor: compact the valid correspondences in i1 order
    const int fc = tb.cur_bcast >= 0 ? tb.cur_bcast : f;
    const sd_keypoint* kps1 = kps1_all + (size_t)fc * K;
    const sd_keypoint* kps2 = kps2_all + fK;
    const int N1 = min(n1_all[fc], K), N2 = min(n2_all[f], K);
    const int32_t* m12 = tb.sp_match + fK;
    const uint8_t *v1 = tb.sp_valid1 + fK, *v2 = tb.sp_valid2 + fK;
    const double *T1 = tb.Tcur + (size_t)f * 16, *T2 = tb.Tref + (size_t)f * 16;
    const double *Xw1 = tb.s3_Xw1 + fK * 3, *Xw2 = tb.s3_Xw2 + fK * 3;
    int n = 0;
    for (int i0 = 0; i0 < K; i0 += 64) {
      const int i1 = i0 + lane;
      int m = -1;
      bool ok = false;
      if (i1 < N1) {
        m = m12[i1];
        ok = m >= 0 && m < N2 && v1[i1] != 0 && v2[m] != 0;
      }
      const int pos = wave_append(ok, lt, n);
      if (ok) {
        const int o1 = min(max(kps1[i1].octave, 0), nlevels - 1), o2 = min(max(kps2[m].octave, 0), nlevels - 1);
        // mvnMaxError is a vector<size_t>: 9.210 * sigma2 (double) is truncated
        GF[4 * K + pos] = (float)(unsigned long long)(9.210 * (double)sigma2[o1]);
        GF[5 * K + pos] = (float)(unsigned long long)(9.210 * (double)sigma2[o2]);
        gidx[pos] = (uint16_t)i1;
        double c1[3], c2[3];
#pragma unroll
        for (int r = 0; r < 3; r++) {
          const double *a = Xw1 + (size_t)i1 * 3, *bb = Xw2 + (size_t)m * 3;
          c1[r] = ((T1[r] * a[0] + T1[4 + r] * a[1]) + T1[8 + r] * a[2]) + T1[12 + r];
          c2[r] = ((T2[r] * bb[0] + T2[4 + r] * bb[1]) + T2[8 + r] * bb[2]) + T2[12 + r];
          GX[r * K + pos] = c1[r];
          GX[(3 + r) * K + pos] = c2[r];
        }
        s3_to_image(c1[0], c1[1], c1[2], cam, &GF[0 * K + pos], &GF[1 * K + pos]);
        s3_to_image(c2[0], c2[1], c2[2], cam, &GF[2 * K + pos], &GF[3 * K + pos]);
      }
    }
    N = n;
    max_its = max_its_tab[N];
    its = 0;
    best = 0;
    // GetEstimated* before any iteration: zeros here (uninitialised members in the reference)
    if (lane < 16) tb.s3_bestT[(size_t)f * 16 + lane] = 0.0;
    if (lane < 9) tb.s3_R[(size_t)f * 9 + lane] = 0.0;
    if (lane < 3) tb.s3_t[(size_t)f * 3 + lane] = 0.0;
    if (lane == 0) tb.s3_s[f] = 0.0;
  } else {
    its = st[0];
    best = st[1];
    N = min(max(st[2], 0), K);
    max_its = st[3];
    if (lane < S3_WORDS) best_mask = tb.s3_best_mask[(size_t)f * S3_WORDS + lane];
  }
  __threadfence();   // the gathered arrays and the cleared outputs are read / rewritten by other lanes below

  bool returned = false;
  int n_inliers = 0;
  const bool enough = N >= sp.min_inliers;
  if (enough) {
    const int32_t* rs = tb.rand_stream + (size_t)f * sp.rand_per_frame;
    int done = 0;
    while (its < max_its && done < sp.n_iterations && !returned) {
      const int chunk = min(min(sp.n_iterations - done, max_its - its), 64);
      S3Hyp H;
#pragma unroll
      for (int k = 0; k < 9; k++) H.R[k] = H.sR[k] = H.sRi[k] = 0.0;
#pragma unroll
      for (int k = 0; k < 3; k++) H.t[k] = H.ti[k] = 0.0;
      H.s = 0.f;
      if (lane < chunk) {
        // the three draws without replacement (swap with back, pop), resolved on the at most two displaced positions
        const int32_t* r3 = rs + (size_t)3 * (its + lane);
        const int r0 = min(s3_random(r3[0], N), N - 1), r1 = min(s3_random(r3[1], N - 1), N - 2), r2 = min(s3_random(r3[2], N - 2), N - 3);
        const int id0 = r0;
        const int id1 = r1 == r0 ? N - 1 : r1;
        const int back1 = (N - 2 == r0) ? N - 1 : N - 2;   // what the second swap moves into position r1
        const int id2 = r2 == r1 ? back1 : (r2 == r0 ? N - 1 : r2);
        const int ids[3] = {max(id0, 0), max(id1, 0), max(id2, 0)};
        double P1[3][3], P2[3][3];
#pragma unroll
        for (int c = 0; c < 3; c++)
#pragma unroll
          for (int r = 0; r < 3; r++) {
            P1[r][c] = GX[r * K + ids[c]];
            P2[r][c] = GX[(3 + r) * K + ids[c]];
          }
        s3_compute_sim3(P1, P2, sp.fix_scale, H);
      }
      for (int h = 0; h < chunk; h++) {
        // ---- CheckInliers of hypothesis h
        double A[12], Bm[12];   // T12 = [sR | t], T21 = [sRinv | tinv], rows
#pragma unroll
        for (int k = 0; k < 9; k++) {
          A[(k / 3) * 4 + k % 3] = s3_bcast(H.sR[k], h);
          Bm[(k / 3) * 4 + k % 3] = s3_bcast(H.sRi[k], h);
        }
#pragma unroll
        for (int k = 0; k < 3; k++) {
          A[k * 4 + 3] = s3_bcast(H.t[k], h);
          Bm[k * 4 + 3] = s3_bcast(H.ti[k], h);
        }
        int cnt = 0;
        unsigned long long my_mask = 0;
        for (int j0 = 0; j0 < N; j0 += 64) {
          const int j = j0 + lane;
          bool in = false;
          if (j < N) {
            const double x1 = GX[j], y1 = GX[K + j], z1 = GX[2 * K + j], x2 = GX[3 * K + j], y2 = GX[4 * K + j], z2 = GX[5 * K + j];
            float u, v;
            // vP2im1 = Project(mvX3Dc2, T12, K1)
            s3_to_image(((A[0] * x2 + A[1] * y2) + A[2] * z2) + A[3], ((A[4] * x2 + A[5] * y2) + A[6] * z2) + A[7],
                        ((A[8] * x2 + A[9] * y2) + A[10] * z2) + A[11], cam, &u, &v);
            const double d1x = (double)GF[j] - (double)u, d1y = (double)GF[K + j] - (double)v;
            // vP1im2 = Project(mvX3Dc1, T21, K2)
            s3_to_image(((Bm[0] * x1 + Bm[1] * y1) + Bm[2] * z1) + Bm[3], ((Bm[4] * x1 + Bm[5] * y1) + Bm[6] * z1) + Bm[7],
                        ((Bm[8] * x1 + Bm[9] * y1) + Bm[10] * z1) + Bm[11], cam, &u, &v);
            const double d2x = (double)u - (double)GF[2 * K + j], d2y = (double)v - (double)GF[3 * K + j];
            const float err1 = (float)(d1x * d1x + d1y * d1y), err2 = (float)(d2x * d2x + d2y * d2y);
            in = err1 < GF[4 * K + j] && err2 < GF[5 * K + j];   // a NaN hypothesis has no inlier
          }
          const unsigned long long b = __ballot(in);
          if (lane == (j0 >> 6)) my_mask = b;
          cnt += __popcll(b);
        }
        // ---- the sequential part of iterate(), iteration its + 1
        its++;
        done++;
        if (cnt >= best) {
          best = cnt;
          best_mask = my_mask;
          if (lane == h) {
#pragma unroll
            for (int c = 0; c < 3; c++) {
#pragma unroll
              for (int r = 0; r < 3; r++) {
                tb.s3_bestT[(size_t)f * 16 + c * 4 + r] = H.sR[r * 3 + c];
                tb.s3_R[(size_t)f * 9 + c * 3 + r] = H.R[r * 3 + c];
              }
              tb.s3_bestT[(size_t)f * 16 + c * 4 + 3] = 0.0;
              tb.s3_bestT[(size_t)f * 16 + 12 + c] = H.t[c];
              tb.s3_t[(size_t)f * 3 + c] = H.t[c];
            }
            tb.s3_bestT[(size_t)f * 16 + 15] = 1.0;
            tb.s3_s[f] = (double)H.s;
          }
          if (cnt > sp.min_inliers) {
            returned = true;
            n_inliers = cnt;
            if (lane == h) {
#pragma unroll
              for (int c = 0; c < 3; c++) {
#pragma unroll
                for (int r = 0; r < 3; r++) T_out[c * 4 + r] = H.sR[r * 3 + c];
                T_out[c * 4 + 3] = 0.0;
                T_out[12 + c] = H.t[c];
              }
              T_out[15] = 1.0;
            }
            break;   // the later hypotheses of the chunk were never drawn
          }
        }
      }
    }
    if (returned) {
      for (int j0 = 0; j0 < N; j0 += 64) {
        const int j = j0 + lane;
        const unsigned int lo = (unsigned int)__builtin_amdgcn_readlane((int)(unsigned int)best_mask, j0 >> 6);
        const unsigned int hi = (unsigned int)__builtin_amdgcn_readlane((int)(unsigned int)(best_mask >> 32), j0 >> 6);
        const unsigned long long w = ((unsigned long long)hi << 32) | lo;
        if (j < N && ((w >> lane) & 1ull)) inl_out[min((int)gidx[j], K - 1)] = 1;
      }
    }
  }
  const bool no_more = !enough || (!returned && its >= max_its);
  if (lane < S3_WORDS) tb.s3_best_mask[(size_t)f * S3_WORDS + lane] = best_mask;
  if (lane == 0) {
    st[0] = its;
    st[1] = best;
    st[2] = N;
    st[3] = max_its;
    st[4] = sp.min_inliers;
    st[5] = sp.fix_scale;
    int32_t* info = tb.s3_info + (size_t)f * 8;
    info[0] = returned;
    info[1] = n_inliers;
    info[2] = no_more;
    info[3] = its;
    info[4] = N;
    info[5] = max_its;
    info[6] = best;
    info[7] = 0;
  }
}

int launch_sim3(const sd_orb* cur, const sd_orb* ref, const TrackBuffers& tb, const TrackCam& cam, const float* d_sigma2,
                const int32_t* d_max_its, const Sim3Params& sp, int n_frames, hipStream_t s) {
  SD_REQUIRE(tb.kp_cap <= S3_MAXN, SD_ERR_CAPACITY, "Sim3Solver supports at most 2048 keypoints per keyframe");
  hipLaunchKernelGGL(k_sim3, dim3(n_frames), dim3(64), 0, s, keys_un(cur), cur->d_nout, keys_un(ref), ref->d_nout, tb, cam, d_sigma2, cur->nlevels, d_max_its, sp);
  SD_HIP_CHECK(hipGetLastError());
  return SD_OK;
}

}  // namespace sd

using namespace sd;

// mRansacMaxIts for N correspondences (src/Sim3Solver.cc:122-132), with the host's libm.  epsilon is a float, pow and log are
// the double overloads.  N < minInliers makes the logarithm's argument negative: ceil(NaN) converted to int is INT_MIN on
// x86-64 (the reference's platform), which min / max turn into 1; the same is written out here for a quotient outside int.
static int sim3_max_its(int N, double probability, int min_inliers, int max_iterations) {
  int n_it;
  if (min_inliers == N) {
    n_it = 1;
  } else {
    const float epsilon = (float)min_inliers / N;
    const double v = std::ceil(std::log(1 - probability) / std::log(1 - std::pow((double)epsilon, 3.0)));
    n_it = (v >= -2147483648.0 && v < 2147483648.0) ? (int)v : INT_MIN;
  }
  return std::max(1, std::min(n_it, max_iterations));
}

// every slot must have been given the rand() values the call can consume: 3 per iteration, from the start of the stream
static int sim3_check_rand(sd_track* h, int n_frames, long long iterations) {
  const long long need = 3 * iterations;
  SD_REQUIRE(need <= h->rand_per_frame, SD_ERR_CAPACITY, "iterations exceed the rand() values a slot holds (4 x pnp_max_iterations)");
  for (int f = 0; f < n_frames; f++)
    SD_REQUIRE(h->rand_len[f] >= need, SD_ERR_INVALID_ARG, "sd_track_set_rand supplied fewer rand() values than the iterations can consume (3 per iteration)");
  return SD_OK;
}

static int run_sim3(sd_track* h, int n_frames, const Sim3Params& sp) {
  return run_stage(h, true, false, STAGE_SOLVE, [&](hipStream_t s) {
    return launch_sim3(h->cur, h->ref, h->tb, h->cam, h->d_sigma2, h->d_sim3_max_its, sp, n_frames, s);
  });
}

extern "C" {

int sd_track_set_sim3_points(sd_track* h, int frame0, int n_frames, const double* Xw_cur, const double* Xw_ref, int cap) {
  TRACK_RANGE(h, frame0, n_frames);
  SD_REQUIRE(Xw_cur && Xw_ref && cap >= 1 && cap <= h->kp_cap, SD_ERR_INVALID_ARG, "bad point arrays (cap must be 1..keypoint capacity)");
  END_RESULTS(h, "sd_track_set_sim3_points");
  hipStream_t s = h->cur->stream;
  const size_t K3 = (size_t)h->kp_cap * 3;
  SD_TRY(upload_rows(h->tb.s3_Xw1, K3, Xw_cur, (size_t)cap * 3, frame0, n_frames, s));
  SD_TRY(upload_rows(h->tb.s3_Xw2, K3, Xw_ref, (size_t)cap * 3, frame0, n_frames, s));
  return wait_for(s);
}

int sd_track_set_point_matches(sd_track* h, int frame0, int n_frames, const int32_t* matches12, int cap) {
  TRACK_RANGE(h, frame0, n_frames);
  SD_REQUIRE(matches12 && cap >= 1 && cap <= h->kp_cap, SD_ERR_INVALID_ARG, "bad match array (cap must be 1..keypoint capacity)");
  for (size_t i = 0; i < (size_t)n_frames * cap; i++)
    SD_REQUIRE(matches12[i] >= -1 && matches12[i] < h->kp_cap, SD_ERR_INVALID_ARG, "match index outside [-1, keypoint capacity)");
  END_RESULTS(h, "sd_track_set_point_matches");
  hipStream_t s = h->cur->stream;
  const size_t K = h->kp_cap;
  SD_HIP_CHECK(hipMemsetAsync(h->tb.sp_match + (size_t)frame0 * K, 0xFF, (size_t)n_frames * K * sizeof(int32_t), s));   // the rest: NULL
  SD_TRY(upload_rows(h->tb.sp_match, K, matches12, cap, frame0, n_frames, s));
  return wait_for(s);
}

int sd_track_sim3(sd_track* h, int n_frames, int fix_scale, double probability, int min_inliers, int max_iterations, int n_iterations) {
  SD_TRY(check_ready(h, n_frames));
  SD_TRY(require_ref_frames(h, n_frames, false, true));
  SD_REQUIRE(probability > 0.0 && probability < 1.0, SD_ERR_INVALID_ARG, "probability must lie in (0, 1)");
  SD_REQUIRE(min_inliers >= 3 && max_iterations >= 1 && n_iterations >= 1, SD_ERR_INVALID_ARG,
             "bad RANSAC parameters (min_inliers >= 3, max_iterations >= 1, n_iterations >= 1)");
  END_RESULTS(h, "sd_track_sim3");
  // mnIterations never passes mRansacMaxIts <= max_iterations
  SD_TRY(sim3_check_rand(h, n_frames, std::min(max_iterations, n_iterations)));
  std::vector<int32_t> table((size_t)h->kp_cap + 1);
  for (int N = 0; N <= h->kp_cap; N++) table[N] = sim3_max_its(N, probability, min_inliers, max_iterations);
  SD_TRY(h->sim3_ring.upload(h->d_sim3_max_its, table.data(), table.size(), h->pnp_stream));
  Sim3Params sp;
  sp.fix_scale = fix_scale != 0;
  sp.min_inliers = min_inliers;
  sp.n_iterations = n_iterations;
  sp.rand_per_frame = h->rand_per_frame;
  sp.resume = 0;
  SD_TRY(run_sim3(h, n_frames, sp));
  h->res.sim3.set(n_frames, BIND_SIM3, inputs_now(h));
  h->sim3_params = sp;
  h->sim3_max_its = max_iterations;
  h->sim3_iter_upper = std::min(max_iterations, n_iterations);
  return SD_OK;
}

int sd_track_sim3_iterate(sd_track* h, int n_frames, int n_iterations) {
  SD_TRY(check_ready(h, n_frames));
  SD_REQUIRE(h->res.sim3.live(n_frames, inputs_now(h)), SD_ERR_INVALID_ARG,
             "sd_track_sim3 has not constructed solvers for these slots (or their keyframes, matches, points, flags, poses or rand stream "
             "were replaced since)");
  SD_REQUIRE(n_iterations >= 1, SD_ERR_INVALID_ARG, "bad n_iterations");
  Sim3Params sp = h->sim3_params;
  const long long upper = std::min<long long>(h->sim3_max_its, (long long)h->sim3_iter_upper + n_iterations);
  SD_TRY(sim3_check_rand(h, n_frames, upper));
  sp.n_iterations = n_iterations;
  sp.resume = 1;
  SD_TRY(run_sim3(h, n_frames, sp));
  h->sim3_iter_upper = (int)upper;
  return SD_OK;
}

int sd_track_get_sim3(sd_track* h, int frame0, int n_frames, double* T12_cm, double* R12_cm, double* t12, double* scale, uint8_t* inliers,
                      int cap, int32_t* info8) {
  TRACK_RANGE(h, frame0, n_frames);
  SD_REQUIRE(!inliers || cap >= h->kp_cap, SD_ERR_CAPACITY, "cap smaller than the keypoint capacity");
  hipStream_t s = h->cur->stream;
  const TrackBuffers& tb = h->tb;
  SD_TRY(download(T12_cm, tb.s3_T, frame0, n_frames, 16, s));
  SD_TRY(download(R12_cm, tb.s3_R, frame0, n_frames, 9, s));
  SD_TRY(download(t12, tb.s3_t, frame0, n_frames, 3, s));
  SD_TRY(download(scale, tb.s3_s, frame0, n_frames, 1, s));
  SD_TRY(download_rows(inliers, cap, tb.s3_inliers, frame0, n_frames, h->kp_cap, s));
  SD_TRY(download(info8, tb.s3_info, frame0, n_frames, 8, s));
  return wait_for(s);
}

}  // extern "C"
