// LocalMapping::CreateNewMapPoints after the epipolar search (reference src/LocalMapping.cc:219-419; KeyFrame::UnprojectStereo
// src/KeyFrame.cc:572-585; MapPoint::UpdateNormalAndDepth src/MapPoint.cc:304-343): every match of sd_track_search_for_triangulation
// is triangulated and tested on the device, and the accepted ones become map point rows.  The pairing is the search's: slot f
// pairs KF1 = frame f (or the broadcast frame) of `cur`, pose Tcur[f], with KF2 = frame f of `ref`, pose Tref[f].
//
// k_triangulate, one lane per (slot, idx1); a lane whose row has no match writes verdict 0 and idles.  Operand widths are the
// reference's; every product and sum is rounded on its own (the library is built with -ffp-contract=off), 3-vector products are
// dot3 = (x0 * y0 + x1 * y1) + x2 * y2, Rcw[r][c] = T[c * 4 + r], Rwc = Rcw^T, tcw = T[12..14], Ow[r] = -dot3(Rwc row r, tcw).
//   1. xn = ((double)((x - cx) * invfx), (double)((y - cy) * invfy), 1.0) with float products on mvKeysUn; ray = Rwc * xn by dot3;
//      cosParallaxRays = (float)(dot3(ray1, ray2) / (sqrt(dot3(ray1, ray1)) * sqrt(dot3(ray2, ray2)))).
//   2. cosParallaxStereo{1,2} = cosParallaxRays + 1 (float); `if (bStereo1) ... else if (bStereo2)` (:288-291) sets ONE of them to
//      cosf(2 * atan2f(mb / 2, mvDepth)), all float, cosf = sd_sincosf.h's, atan2f the device library's (within a few ulp of the
//      host's; the value feeds comparisons only).
//   3. :296 chooses linear triangulation; else :318 UnprojectStereo(idx1), :320 UnprojectStereo(idx2), else verdict LOW_PARALLAX.
//      UnprojectStereo reads mvKeys (the distorted keypoint) and mvDepth: z <= 0 gives the zero vector, which goes on through the
//      tests; else x = ((u - cx) * z) * invfx, y likewise (float), Xw[r] = dot3(Rwc row r, (x, y, z)) + Ow[r] -- the order of
//      k_new_points.
//   4. A row 0 = xn1[0] * Tcw1 row 2 - Tcw1 row 0, row 1 with xn1[1] and row 1, rows 2, 3 the same on KF2 (double: one product,
//      one difference), rounded to float (Converter::toCvMat).  cv::SVD::compute on CV_32F is the float instantiation of OpenCV
//      3.2's JacobiSVDImpl_ on At = A^T: matrix and Vt elements float, W and a, b, p, c, s double, products (double)x * y, a new
//      element (float)(c * x + s * y) / (float)(-s * x + c * y), hypot = sd_hypot.h's, eps = FLT_EPSILON * 2, up to 30 sweeps over
//      the pairs (0,1) (0,2) (0,3) (1,2) (1,3) (2,3), a sweep without rotation ends them; W = sqrt of the row norms, selection sort
//      descending (strict <, so the first of equals stays).  The zero-singular-value tail touches only U.  x3D = Vt row 3;
//      x3D[3] == 0 -> verdict W_ZERO; else x3D[k] / x3D[3] in float, widened to double.
//      The six pair rotations are instantiated on compile-time indices, so At, Vt and W stay in registers; the sweep loop runs
//      while a lane of the wave still rotates (a lane that stopped stays stopped: its state would not change).
//   5. z1 = (float)(dot3(Rcw1 row 2, x3D) + tcw1[2]) <= 0 -> Z1; z2 likewise -> Z2.  x1, y1 the same on rows 0, 1; invz1 =
//      (float)(1.0 / (double)z1); u1 = ((fx * x1) * invz1) + cx, v1 likewise, float.  Mono: (double)(ex * ex + ey * ey) >
//      5.991 * (double)sigma2[octave1]; stereo: u1_r = u1 - mbf * invz1, (double)((ex * ex + ey * ey) + er * er) > 7.8 * sigma2
//      -> REPROJ1.  KF2 the same with KF1's mbf (:374) -> REPROJ2.  dist{1,2} = (float)sqrt(dot3(d, d)), d = x3D - Ow{1,2};
//      either == 0 -> DIST_ZERO.  ratioDist = dist2 / dist1, ratioOctave = sf[octave1] / sf[octave2], ratioFactor = 1.5f *
//      mfScaleFactor: ratioDist * ratioFactor < ratioOctave || ratioDist > ratioOctave * ratioFactor -> SCALE.
//   6. Per slot (:225-239): baseline = (float)sqrt(dot3(d, d)), d = Ow2 - Ow1.  Monocular: (double)(baseline / median) < 0.01
//      skips the slot, median = the caller's ComputeSceneMedianDepth(2) of KF2, negative: no gate.  Otherwise baseline < mb does.
//      Every matched row of a skipped slot gets verdict SLOT_GATED.
//
// k_new_points_resolve, one workgroup of 1024.  Broadcast: a KF1 keypoint gets its point from the first slot whose verdict is 1
// (the reference's later neighbours skip it: SearchForTriangulation passes over keypoints that hold a map point, and its rows
// are independent); ids count from next_id[0] over all points.  Paired: every accepted row is a point of its slot, ids count from
// next_id[slot].  Points are numbered in (slot, idx1) order by ballot prefix sums, no atomics.  Per point, the fields Fuse and
// TrackLocalMap read: mNormalVector = (n1 / |n1| + n2 / |n2|) / 2 per component, n = Xw - Ow (a two-term sum: the std::map's
// pointer order does not matter); mfMaxDistance = dist * sf[octave1] with dist = (float)|Xw - Ow1| (pRefKF = KF1), mfMinDistance =
// mfMaxDistance / sf[nlevels - 1]; the descriptor is KF1's (of two observations ComputeDistinctiveDescriptors returns the first
// in pointer order, which the reference leaves to the allocator).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cstring>
#include <string>
#include <vector>

#include "sd_hypot.h"
#include "sd_sincosf.h"
#include "sd_wave.h"
#include "track_handle.h"

namespace sd {

#define TRIANG_THREADS 256
#define RESOLVE_THREADS 1024
#define RESOLVE_KEYS 2048   // the tracker's keypoint limit

struct TriangIn {
  const sd_keypoint *kps1_un, *kps1, *kps2_un, *kps2;   // [.][cap] mvKeysUn / mvKeys of `cur` and `ref`
  const int32_t* match;                                 // [B][cap]
  const float *ur1, *ur2, *dep1, *dep2;                 // [.][cap]; KF1's rows are rows of the cur FRAME
  const double *Tcur, *Tref;                            // [B][16]
  const float* median;                                  // [B]
  const float *sf, *sigma2;
  float fx, fy, cx, cy, invfx, invfy, bf, mb, ratio_factor;
  int nlevels, cap, cur_bcast, monocular;
  uint8_t *verdict, *branch;                            // [B][cap]
  double* Xw;                                           // [B][cap][3]
};

// Rcw row-major, tcw, Ow.  The two poses of a slot live in LDS (lanes 0 and 1 of the workgroup fill them): held in registers they
// are 60 slot-uniform scalars that stay live across the SVD and spill; read from LDS where they are used they cost nothing.
struct PoseData {
  double R[9], t[3], Ow[3];
};
typedef __attribute__((address_space(3))) PoseData LdsPose;
typedef const LdsPose& Pose;
__device__ __forceinline__ void fill_pose(LdsPose* p, const double* __restrict__ T) {
  double R[9], t[3];
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) R[r * 3 + c] = T[c * 4 + r];
    t[r] = T[12 + r];
  }
  for (int i = 0; i < 9; i++) p->R[i] = R[i];
  for (int r = 0; r < 3; r++) {
    p->t[r] = t[r];
    p->Ow[r] = camera_centre(T, r);
  }
}
// Rwc * v
__device__ __forceinline__ void rotate_back(Pose p, const double (&v)[3], double (&out)[3]) {
  for (int r = 0; r < 3; r++) out[r] = dot3(p.R[r], p.R[3 + r], p.R[6 + r], v[0], v[1], v[2]);
}
// Rcw row r * X + tcw[r]
__device__ __forceinline__ double to_camera(Pose p, int r, const double (&X)[3]) {
  return __dadd_rn(dot3(p.R[r * 3], p.R[r * 3 + 1], p.R[r * 3 + 2], X[0], X[1], X[2]), p.t[r]);
}
__device__ __forceinline__ float norm3f(const double (&d)[3]) { return (float)__dsqrt_rn(dot3(d[0], d[1], d[2], d[0], d[1], d[2])); }

// KeyFrame::UnprojectStereo
__device__ __forceinline__ void unproject_stereo(Pose p, const sd_keypoint& kp, float z, const TriangIn& a, double (&X)[3]) {
  if (!(z > 0)) {
    X[0] = X[1] = X[2] = 0.0;
    return;
  }
  const float x = __fmul_rn(__fmul_rn(__fsub_rn(kp.x, a.cx), z), a.invfx);
  const float y = __fmul_rn(__fmul_rn(__fsub_rn(kp.y, a.cy), z), a.invfy);
  const double c[3] = {(double)x, (double)y, (double)z};
  double w[3];
  rotate_back(p, c, w);
  for (int r = 0; r < 3; r++) X[r] = __dadd_rn(w[r], p.Ow[r]);
}

// One (I, J) step of JacobiSVDImpl_<float>'s sweep on registers; true: the rows were rotated
template <int I, int J>
__device__ __forceinline__ bool svd4_pair(float (&At)[4][4], float (&Vt)[4][4], double (&W)[4]) {
  const double eps = (double)(FLT_EPSILON * 2);
  double a = W[I], b = W[J], p = 0;
#pragma unroll
  for (int k = 0; k < 4; k++) p = __dadd_rn(p, __dmul_rn((double)At[I][k], (double)At[J][k]));
  if (fabs(p) <= __dmul_rn(eps, __dsqrt_rn(__dmul_rn(a, b)))) return false;
  p = __dmul_rn(p, 2.0);
  const double beta = __dsub_rn(a, b), gamma = sdsc::hypot_glibc(p, beta);
  double c, s;
  if (beta < 0) {
    const double delta = __dmul_rn(__dsub_rn(gamma, beta), 0.5);
    s = __dsqrt_rn(__ddiv_rn(delta, gamma));
    c = __ddiv_rn(p, __dmul_rn(__dmul_rn(gamma, s), 2.0));
  } else {
    c = __dsqrt_rn(__ddiv_rn(__dadd_rn(gamma, beta), __dmul_rn(gamma, 2.0)));
    s = __ddiv_rn(p, __dmul_rn(__dmul_rn(gamma, c), 2.0));
  }
  a = b = 0;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const float t0 = (float)__dadd_rn(__dmul_rn(c, (double)At[I][k]), __dmul_rn(s, (double)At[J][k]));
    const float t1 = (float)__dadd_rn(__dmul_rn(-s, (double)At[I][k]), __dmul_rn(c, (double)At[J][k]));
    At[I][k] = t0;
    At[J][k] = t1;
    a = __dadd_rn(a, __dmul_rn((double)t0, (double)t0));
    b = __dadd_rn(b, __dmul_rn((double)t1, (double)t1));
  }
  W[I] = a;
  W[J] = b;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    const float t0 = (float)__dadd_rn(__dmul_rn(c, (double)Vt[I][k]), __dmul_rn(s, (double)Vt[J][k]));
    const float t1 = (float)__dadd_rn(__dmul_rn(-s, (double)Vt[I][k]), __dmul_rn(c, (double)Vt[J][k]));
    Vt[I][k] = t0;
    Vt[J][k] = t1;
  }
  return true;
}

// vt.row(3) of cv::SVD::compute(A) for the lanes with `need`; every lane of the wave calls it.  A row-major.
__device__ __forceinline__ void svd4_last_row(const float (&A)[16], bool need, float (&x)[4]) {
  float At[4][4], Vt[4][4];
  double W[4];
#pragma unroll
  for (int i = 0; i < 4; i++) {
    double sd = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      At[i][k] = A[k * 4 + i];
      Vt[i][k] = k == i ? 1.f : 0.f;
      sd = __dadd_rn(sd, __dmul_rn((double)At[i][k], (double)At[i][k]));
    }
    W[i] = sd;
  }
  bool active = need;
  for (int iter = 0; iter < 30 && __ballot(active); iter++) {   // max_iter = max(m, 30)
    if (active) {
      bool changed = svd4_pair<0, 1>(At, Vt, W);
      changed |= svd4_pair<0, 2>(At, Vt, W);
      changed |= svd4_pair<0, 3>(At, Vt, W);
      changed |= svd4_pair<1, 2>(At, Vt, W);
      changed |= svd4_pair<1, 3>(At, Vt, W);
      changed |= svd4_pair<2, 3>(At, Vt, W);
      active = changed;
    }
  }
#pragma unroll
  for (int i = 0; i < 4; i++) {
    double sd = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) sd = __dadd_rn(sd, __dmul_rn((double)At[i][k], (double)At[i][k]));
    W[i] = __dsqrt_rn(sd);
  }
#pragma unroll
  for (int i = 0; i < 3; i++) {   // selection sort, descending; only W and Vt are read afterwards
    int j = i;
    double wj = W[i];
#pragma unroll
    for (int k = i + 1; k < 4; k++)
      if (wj < W[k]) {
        j = k;
        wj = W[k];
      }
#pragma unroll
    for (int jj = i + 1; jj < 4; jj++)
      if (jj == j) {
        const double tw = W[i]; W[i] = W[jj]; W[jj] = tw;
#pragma unroll
        for (int k = 0; k < 4; k++) { const float t = Vt[i][k]; Vt[i][k] = Vt[jj][k]; Vt[jj][k] = t; }
      }
  }
#pragma unroll
  for (int k = 0; k < 4; k++) x[k] = Vt[3][k];
}

// (errX^2 + errY^2 [+ errR^2]) > chi2 * sigma2 of one keyframe; x, y, z: the point in its camera
__device__ __forceinline__ bool reprojection_fails(const TriangIn& a, float x, float y, float z, const sd_keypoint& kp, bool stereo,
                                                   float ur, float sigma2) {
  const float invz = (float)__ddiv_rn(1.0, (double)z);
  const float u = __fadd_rn(__fmul_rn(__fmul_rn(a.fx, x), invz), a.cx);
  const float v = __fadd_rn(__fmul_rn(__fmul_rn(a.fy, y), invz), a.cy);
  const float ex = __fsub_rn(u, kp.x), ey = __fsub_rn(v, kp.y);
  float e2 = __fadd_rn(__fmul_rn(ex, ex), __fmul_rn(ey, ey));
  if (!stereo) return (double)e2 > __dmul_rn(5.991, (double)sigma2);
  const float er = __fsub_rn(__fsub_rn(u, __fmul_rn(a.bf, invz)), ur);
  e2 = __fadd_rn(e2, __fmul_rn(er, er));
  return (double)e2 > __dmul_rn(7.8, (double)sigma2);
}

__global__ __launch_bounds__(TRIANG_THREADS) void k_triangulate(TriangIn a) {
  __shared__ PoseData s_pose[2];
  const int f = blockIdx.y, i1 = blockIdx.x * TRIANG_THREADS + threadIdx.x;
  const int cap = a.cap;
  if (threadIdx.x < 2) fill_pose((LdsPose*)&s_pose[threadIdx.x], (threadIdx.x ? a.Tref : a.Tcur) + (size_t)f * 16);
  __syncthreads();   // before the early return: every wave of the workgroup reaches it
  const size_t row = (size_t)f * cap + min(i1, cap - 1);
  const int fc = a.cur_bcast >= 0 ? a.cur_bcast : f;
  const int i2 = i1 < cap ? a.match[row] : -1;
  const bool matched = i2 >= 0 && i2 < cap;
  if (!__ballot(matched)) {   // wave-uniform
    if (i1 < cap) {
      a.verdict[row] = SD_TRI_NO_MATCH;
      a.branch[row] = 0;
    }
    return;
  }
  Pose P1 = *(const LdsPose*)&s_pose[0], P2 = *(const LdsPose*)&s_pose[1];
  uint8_t verdict = SD_TRI_NO_MATCH, branch = 0;
  double X[3] = {0.0, 0.0, 0.0};
  // ---- 6. the neighbour's baseline
  const double bl[3] = {__dsub_rn(P2.Ow[0], P1.Ow[0]), __dsub_rn(P2.Ow[1], P1.Ow[1]), __dsub_rn(P2.Ow[2], P1.Ow[2])};
  const float baseline = norm3f(bl);
  bool gated;
  if (a.monocular) {
    const float median = a.median[f];
    gated = median >= 0 && (double)__fdiv_rn(baseline, median) < 0.01;
  } else {
    gated = baseline < a.mb;
  }
  const size_t o1 = (size_t)fc * cap + (matched ? i1 : 0), o2 = (size_t)f * cap + (matched ? i2 : 0);
  const sd_keypoint kp1 = a.kps1_un[o1], kp2 = a.kps2_un[o2];
  const float ur1 = a.ur1[o1], ur2 = a.ur2[o2];
  const bool st1 = ur1 >= 0, st2 = ur2 >= 0;
  const int oct1 = min(max(kp1.octave, 0), a.nlevels - 1), oct2 = min(max(kp2.octave, 0), a.nlevels - 1);
  bool live = matched && !gated;
  if (matched && gated) verdict = SD_TRI_SLOT_GATED;
  // ---- 1. rays and parallax
  const double xn1[3] = {(double)__fmul_rn(__fsub_rn(kp1.x, a.cx), a.invfx), (double)__fmul_rn(__fsub_rn(kp1.y, a.cy), a.invfy), 1.0};
  const double xn2[3] = {(double)__fmul_rn(__fsub_rn(kp2.x, a.cx), a.invfx), (double)__fmul_rn(__fsub_rn(kp2.y, a.cy), a.invfy), 1.0};
  double ray1[3], ray2[3];
  rotate_back(P1, xn1, ray1);
  rotate_back(P2, xn2, ray2);
  const double n1 = __dsqrt_rn(dot3(ray1[0], ray1[1], ray1[2], ray1[0], ray1[1], ray1[2]));
  const double n2 = __dsqrt_rn(dot3(ray2[0], ray2[1], ray2[2], ray2[0], ray2[1], ray2[2]));
  const float cos_rays = (float)__ddiv_rn(dot3(ray1[0], ray1[1], ray1[2], ray2[0], ray2[1], ray2[2]), __dmul_rn(n1, n2));
  // ---- 2. stereo cosines
  float cos_st1 = __fadd_rn(cos_rays, 1.f), cos_st2 = cos_st1;
  if (live && st1) cos_st1 = sdsc::cosf_glibc(__fmul_rn(2.f, atan2f(__fdiv_rn(a.mb, 2.f), a.dep1[o1])));
  else if (live && st2) cos_st2 = sdsc::cosf_glibc(__fmul_rn(2.f, atan2f(__fdiv_rn(a.mb, 2.f), a.dep2[o2])));
  const float cos_st = fminf(cos_st1, cos_st2);
  // ---- 3. branch
  const bool svd = live && cos_rays < cos_st && cos_rays > 0 && (st1 || st2 || (double)cos_rays < 0.9998);
  // ---- 4. linear triangulation
  float A[16];
#pragma unroll
  for (int c = 0; c < 4; c++) {
    const double r10 = c < 3 ? P1.R[c] : P1.t[0], r11 = c < 3 ? P1.R[3 + c] : P1.t[1], r12 = c < 3 ? P1.R[6 + c] : P1.t[2];
    const double r20 = c < 3 ? P2.R[c] : P2.t[0], r21 = c < 3 ? P2.R[3 + c] : P2.t[1], r22 = c < 3 ? P2.R[6 + c] : P2.t[2];
    A[c] = (float)__dsub_rn(__dmul_rn(xn1[0], r12), r10);
    A[4 + c] = (float)__dsub_rn(__dmul_rn(xn1[1], r12), r11);
    A[8 + c] = (float)__dsub_rn(__dmul_rn(xn2[0], r22), r20);
    A[12 + c] = (float)__dsub_rn(__dmul_rn(xn2[1], r22), r21);
  }
  float h[4];
  svd4_last_row(A, svd, h);
  if (svd) {
    branch = 1;
    if (h[3] == 0) {
      verdict = SD_TRI_W_ZERO;
      live = false;
    } else {
      for (int k = 0; k < 3; k++) X[k] = (double)__fdiv_rn(h[k], h[3]);
    }
  } else if (live && st1 && cos_st1 < cos_st2) {
    branch = 2;
    unproject_stereo(P1, a.kps1[o1], a.dep1[o1], a, X);
  } else if (live && st2 && cos_st2 < cos_st1) {
    branch = 3;
    unproject_stereo(P2, a.kps2[o2], a.dep2[o2], a, X);
  } else if (live) {
    verdict = SD_TRI_LOW_PARALLAX;
    live = false;
  }
  // ---- 5. depth, reprojection and scale
  if (live) {
    const float z1 = (float)to_camera(P1, 2, X), z2 = (float)to_camera(P2, 2, X);
    const double d1[3] = {__dsub_rn(X[0], P1.Ow[0]), __dsub_rn(X[1], P1.Ow[1]), __dsub_rn(X[2], P1.Ow[2])};
    const double d2[3] = {__dsub_rn(X[0], P2.Ow[0]), __dsub_rn(X[1], P2.Ow[1]), __dsub_rn(X[2], P2.Ow[2])};
    const float dist1 = norm3f(d1), dist2 = norm3f(d2);
    const float ratio_dist = __fdiv_rn(dist2, dist1), ratio_oct = __fdiv_rn(a.sf[oct1], a.sf[oct2]);
    if (z1 <= 0) verdict = SD_TRI_Z1;
    else if (z2 <= 0) verdict = SD_TRI_Z2;
    else if (reprojection_fails(a, (float)to_camera(P1, 0, X), (float)to_camera(P1, 1, X), z1, kp1, st1, ur1, a.sigma2[oct1]))
      verdict = SD_TRI_REPROJ1;
    else if (reprojection_fails(a, (float)to_camera(P2, 0, X), (float)to_camera(P2, 1, X), z2, kp2, st2, ur2, a.sigma2[oct2]))
      verdict = SD_TRI_REPROJ2;
    else if (dist1 == 0 || dist2 == 0) verdict = SD_TRI_DIST_ZERO;
    else if (__fmul_rn(ratio_dist, a.ratio_factor) < ratio_oct || ratio_dist > __fmul_rn(ratio_oct, a.ratio_factor)) verdict = SD_TRI_SCALE;
    else verdict = SD_TRI_ACCEPTED;
  }
  if (i1 < cap) {
    a.verdict[row] = verdict;
    a.branch[row] = branch;
    for (int k = 0; k < 3; k++) a.Xw[row * 3 + k] = X[k];
  }
}

struct ResolveIn {
  const sd_keypoint* kps1_un;   // [.][cap]
  const uint8_t* desc1;         // [.][cap][32]
  const int32_t* match;         // [B][cap]
  const double *Tcur, *Tref;
  const float* sf;
  int nlevels, cap, cur_bcast, n_frames;
  int32_t* next_id;             // [B]
};

__global__ __launch_bounds__(RESOLVE_THREADS) void k_new_points_resolve(ResolveIn a, TriangBuffers nb) {
  constexpr int PT = RESOLVE_KEYS / RESOLVE_THREADS, WAVES = RESOLVE_THREADS / 64;
  __shared__ int s_acc[WAVES], s_new[WAVES];
  __shared__ PoseData s_pose[2];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int cap = a.cap, n = a.n_frames;
  const bool bcast = a.cur_bcast >= 0;
  const unsigned long long lt = lanemask_lt(lane);
  // the first slot that accepts the keypoint
  int first[PT];
#pragma unroll
  for (int e = 0; e < PT; e++) {
    const int i = e * RESOLVE_THREADS + tid;
    first[e] = -1;
    if (bcast && i < cap)
      for (int b = n - 1; b >= 0; b--)
        if (nb.verdict[(size_t)b * cap + i] == SD_TRI_ACCEPTED) first[e] = b;
  }
  int total = 0, id_next = a.next_id[0];
  for (int b = 0; b < n; b++) {
    const int fc = bcast ? a.cur_bcast : b;
    const int id0 = bcast ? id_next : a.next_id[b];
    int in_slot = 0, acc_slot = 0;
    // the lanes that read the previous slot's poses are done with them
    __syncthreads();
    if (tid < 2) fill_pose((LdsPose*)&s_pose[tid], (tid ? a.Tref : a.Tcur) + (size_t)b * 16);
    Pose P1 = *(const LdsPose*)&s_pose[0], P2 = *(const LdsPose*)&s_pose[1];
#pragma unroll
    for (int e = 0; e < PT; e++) {
      const int i = e * RESOLVE_THREADS + tid;
      const size_t row = (size_t)b * cap + min(i, cap - 1);
      const bool acc = i < cap && nb.verdict[row] == SD_TRI_ACCEPTED;
      const bool nw = acc && (!bcast || first[e] == b);
      const unsigned long long ba = __ballot(acc), bn = __ballot(nw);
      __syncthreads();   // the previous round's sums have been read
      if (lane == 0) {
        s_acc[wave] = __popcll(ba);
        s_new[wave] = __popcll(bn);
      }
      __syncthreads();
      int off = 0, sum = 0;
      for (int w = 0; w < WAVES; w++) {
        if (w < wave) off += s_new[w];
        sum += s_new[w];
        acc_slot += s_acc[w];
      }
      if (nw) {
        const int r = in_slot + off + __popcll(bn & lt);
        const size_t g = (size_t)total + r;   // < B * cap: at most one point per (slot, idx1)
        double X[3], d1[3], d2[3];
        for (int k = 0; k < 3; k++) {
          X[k] = nb.Xw[row * 3 + k];
          d1[k] = __dsub_rn(X[k], P1.Ow[k]);
          d2[k] = __dsub_rn(X[k], P2.Ow[k]);
        }
        const double l1 = __dsqrt_rn(dot3(d1[0], d1[1], d1[2], d1[0], d1[1], d1[2]));
        const double l2 = __dsqrt_rn(dot3(d2[0], d2[1], d2[2], d2[0], d2[1], d2[2]));
        for (int k = 0; k < 3; k++) {
          nb.geo[g * 6 + k] = X[k];
          nb.geo[g * 6 + 3 + k] = __ddiv_rn(__dadd_rn(__ddiv_rn(d1[k], l1), __ddiv_rn(d2[k], l2)), 2.0);
        }
        const size_t o1 = (size_t)fc * cap + i;
        const float mx = __fmul_rn((float)l1, a.sf[min(max(a.kps1_un[o1].octave, 0), a.nlevels - 1)]);
        ((float2*)nb.dist)[g] = make_float2(mx, __fdiv_rn(mx, a.sf[a.nlevels - 1]));
        const uint4* d = (const uint4*)(a.desc1 + o1 * 32);
        ((uint4*)(nb.desc + g * 32))[0] = d[0];
        ((uint4*)(nb.desc + g * 32))[1] = d[1];
        ((int4*)nb.pt)[g] = make_int4(i, b, a.match[row], id0 + r);
      }
      in_slot += sum;
    }
    __syncthreads();   // every lane has read next_id[b]
    if (tid == 0) {
      nb.count[(size_t)b * 2] = acc_slot;
      nb.count[(size_t)b * 2 + 1] = in_slot;
      if (!bcast) a.next_id[b] = id0 + in_slot;
    }
    total += in_slot;
    id_next = id0 + in_slot;
  }
  if (tid == 0) {
    if (bcast) a.next_id[0] = id_next;
    nb.info[0] = total;
    nb.info[1] = a.cur_bcast;
    nb.info[2] = n;
    nb.info[3] = bcast ? id_next : -1;
  }
}

// The camera and gate constants of a TriangIn, in Frame's float arithmetic (invfx = 1.0f / fx, mb = mbf / fx of make_cam)
static void set_camera(TriangIn& a, const TrackCam& cam, float ratio_factor) {
  a.fx = cam.ffx; a.fy = cam.ffy; a.cx = cam.fcx; a.cy = cam.fcy;
  a.invfx = 1.0f / cam.ffx; a.invfy = 1.0f / cam.ffy;
  a.bf = cam.bf; a.mb = cam.mb;
  a.ratio_factor = ratio_factor;
}

static int launch_k_triangulate(const TriangIn& a, int n_frames, hipStream_t s) {
  hipLaunchKernelGGL(k_triangulate, dim3((a.cap + TRIANG_THREADS - 1) / TRIANG_THREADS, n_frames), dim3(TRIANG_THREADS), 0, s, a);
  SD_HIP_CHECK(hipGetLastError());
  return SD_OK;
}

int launch_triangulate(const sd_orb* cur, const sd_orb* ref, const TrackBuffers& tb, const TriangBuffers& nb, const TrackCam& cam,
                       const float* d_sf, const float* d_sigma2, float ratio_factor, int n_frames, int monocular, hipStream_t s) {
  SD_REQUIRE(tb.kp_cap <= RESOLVE_KEYS, SD_ERR_CAPACITY, "triangulation supports at most 2048 keypoints per keyframe");
  const sd_keypoint* k1u = keys_un(cur);
  const sd_keypoint* k2u = keys_un(ref);
  TriangIn a = {k1u, cur->d_kps, k2u, ref->d_kps, tb.tri_match, tb.uright, tb.uright_ref, tb.depth, nb.depth_ref, tb.Tcur, tb.Tref,
                nb.median, d_sf, d_sigma2, 0, 0, 0, 0, 0, 0, 0, 0, 0, cur->nlevels, tb.kp_cap, tb.cur_bcast, monocular, nb.verdict,
                nb.branch, nb.Xw};
  set_camera(a, cam, ratio_factor);
  SD_TRY(launch_k_triangulate(a, n_frames, s));
  const ResolveIn r = {k1u, cur->d_desc, tb.tri_match, tb.Tcur, tb.Tref, d_sf, cur->nlevels, tb.kp_cap, tb.cur_bcast, n_frames, tb.next_id};
  hipLaunchKernelGGL(k_new_points_resolve, dim3(1), dim3(RESOLVE_THREADS), 0, s, r, nb);
  SD_HIP_CHECK(hipGetLastError());
  return SD_OK;
}

}  // namespace sd

using namespace sd;

namespace {
const char* const kNoTriangulation =
    "sd_track_triangulate has not run on these slots (or the search's result, mvDepth, the median depths or the camera were "
    "replaced since)";
}  // namespace

extern "C" {

int sd_track_set_tri_depth(sd_track* h, int side, int frame0, int n_frames, const float* depth, int cap) {
  QUEUE_RANGE(h, frame0, n_frames);
  SD_REQUIRE((side == 0 || side == 1) && depth && cap >= 1 && cap <= h->kp_cap, SD_ERR_INVALID_ARG, "bad side or depth array");
  END_RESULTS(h, "sd_track_set_tri_depth");
  SD_TRY(upload_rows(side == 0 ? h->tb.depth : h->nb.depth_ref, h->kp_cap, depth, cap, frame0, n_frames, h->pnp_stream));
  return wait_for(h->pnp_stream);   // the rows are the caller's pageable memory: back once they are read
}

int sd_track_set_tri_median_depth(sd_track* h, int frame0, int n_frames, const float* median_depth) {
  QUEUE_RANGE(h, frame0, n_frames);
  SD_REQUIRE(median_depth, SD_ERR_INVALID_ARG, "NULL argument");
  END_RESULTS(h, "sd_track_set_tri_median_depth");
  return h->small_ring.upload(h->nb.median + frame0, median_depth, (size_t)n_frames, h->pnp_stream);
}

int sd_track_triangulate(sd_track* h, int n_frames, int monocular) {
  SD_TRY(check_ready(h, n_frames));
  SD_TRY(require_ref_frames(h, n_frames, false));
  SD_REQUIRE(monocular == 0 || monocular == 1, SD_ERR_INVALID_ARG, "monocular must be 0 or 1");
  SD_REQUIRE(h->res.tri.live(n_frames, inputs_now(h)), SD_ERR_INVALID_ARG,
             "no live result of sd_track_search_for_triangulation covers these slots (see sd_track_get_triangulation_matches)");
  // with the rotation check a row's match depends on the other rows: "the first accepting slot" is then not the reference's loop
  SD_REQUIRE(h->tb.cur_bcast < 0 || h->res.tri.payload == 0, SD_ERR_INVALID_ARG,
             "broadcast mode needs a search with check_ori = 0 (CreateNewMapPoints' matcher has mbCheckOrientation off)");
  const float ratio_factor = 1.5f * h->cur->scaleFactor;
  END_RESULTS(h, "sd_track_triangulate");   // the point list an append left readable is overwritten
  SD_TRY(run_stage(h, true, false, STAGE_NONE, [&](hipStream_t s) {
    return launch_triangulate(h->cur, h->ref, h->tb, h->nb, h->cam, h->d_sf, h->d_sigma2, ratio_factor, n_frames, monocular, s);
  }));
  h->res.triang.set(n_frames, BIND_TRIANG, inputs_now(h));
  return SD_OK;
}

int sd_track_get_triangulated(sd_track* h, int frame0, int n_frames, uint8_t* verdict, uint8_t* branch, double* Xw, int cap,
                              int32_t* n_accepted) {
  TRACK_RANGE(h, frame0, n_frames);
  SD_REQUIRE(h->res.triang_live(frame0 + n_frames, inputs_now(h)), SD_ERR_INVALID_ARG, kNoTriangulation);
  SD_REQUIRE(!(verdict || branch || Xw) || cap >= h->kp_cap, SD_ERR_CAPACITY, "cap smaller than the keypoint capacity");
  hipStream_t s = h->cur->stream;
  const size_t K = h->kp_cap;
  SD_TRY(download_rows(verdict, cap, h->nb.verdict, frame0, n_frames, K, s));
  SD_TRY(download_rows(branch, cap, h->nb.branch, frame0, n_frames, K, s));
  if (Xw)
    SD_HIP_CHECK(hipMemcpy2DAsync(Xw, (size_t)cap * 24, h->nb.Xw + (size_t)frame0 * K * 3, K * 24, K * 24, n_frames, hipMemcpyDeviceToHost, s));
  if (n_accepted)
    SD_HIP_CHECK(hipMemcpy2DAsync(n_accepted, 4, h->nb.count + (size_t)frame0 * 2, 8, 4, n_frames, hipMemcpyDeviceToHost, s));
  return wait_for(s);
}

int sd_track_get_new_points(sd_track* h, int32_t* info4, int32_t* kp1, int32_t* slot, int32_t* idx2, int32_t* ids, double* Xw,
                            double* normal, float* max_dist, float* min_dist, uint8_t* desc, int cap) {
  TRACK_RANGE(h, 0, 1);
  // after sd_track_append_new_points the list is the record of what went into the rows: readable until the append's result ends,
  // also where the append itself (mark_flags) or a later call ended the triangulation
  SD_REQUIRE(h->res.triang_live(h->res.triang.n, inputs_now(h)) || h->res.append.live(1, inputs_now(h)), SD_ERR_INVALID_ARG,
             kNoTriangulation);
  SD_REQUIRE(info4 && cap >= 0, SD_ERR_INVALID_ARG, "info4 is NULL or cap negative");
  hipStream_t s = h->cur->stream;
  SD_TRY(download(info4, h->nb.info, 0, 1, 4, s));
  SD_TRY(wait_for(s));
  const size_t n = (size_t)info4[0];
  if (n == 0) return SD_OK;
  SD_REQUIRE(!(kp1 || slot || idx2 || ids || Xw || normal || max_dist || min_dist || desc) || (size_t)cap >= n, SD_ERR_CAPACITY,
             "cap smaller than the number of new points (info4[0])");
  const TriangBuffers& nb = h->nb;
  // column c of a device row of `row` bytes -> a dense host array of `width`-byte entries
  auto column = [&](void* dst, const void* src, size_t c_off, size_t width, size_t row) -> int {
    if (dst) SD_HIP_CHECK(hipMemcpy2DAsync(dst, width, (const uint8_t*)src + c_off, row, width, n, hipMemcpyDeviceToHost, s));
    return SD_OK;
  };
  SD_TRY(column(kp1, nb.pt, 0, 4, 16));
  SD_TRY(column(slot, nb.pt, 4, 4, 16));
  SD_TRY(column(idx2, nb.pt, 8, 4, 16));
  SD_TRY(column(ids, nb.pt, 12, 4, 16));
  SD_TRY(column(Xw, nb.geo, 0, 24, 48));
  SD_TRY(column(normal, nb.geo, 24, 24, 48));
  SD_TRY(column(max_dist, nb.dist, 0, 4, 8));
  SD_TRY(column(min_dist, nb.dist, 4, 4, 8));
  SD_TRY(download(desc, nb.desc, 0, n, 32, s));
  return wait_for(s);
}

int sd_debug_triangulate(int n1, int n2, const sd_keypoint* kps1_un, const sd_keypoint* kps1, const float* uright1, const float* depth1,
                         const sd_keypoint* kps2_un, const sd_keypoint* kps2, const float* uright2, const float* depth2,
                         const int32_t* matches12, const double* Tcw1_cm16, const double* Tcw2_cm16, const float* cam5,
                         const float* scale_factors, const float* level_sigma2, int nlevels, float scale_factor, int monocular,
                         float median_depth, uint8_t* verdict, uint8_t* branch, double* Xw) {
  SD_REQUIRE(n1 >= 0 && n2 >= 0 && n1 <= 2048 && n2 <= 2048, SD_ERR_CAPACITY, "at most 2048 keypoints per keyframe");
  SD_REQUIRE((n1 == 0 || (kps1_un && kps1 && uright1 && depth1 && matches12 && verdict && branch && Xw)) &&
                 (n2 == 0 || (kps2_un && kps2 && uright2 && depth2)),
             SD_ERR_INVALID_ARG, "NULL keyframe array");
  SD_REQUIRE(Tcw1_cm16 && Tcw2_cm16 && cam5 && scale_factors && level_sigma2 && nlevels >= 1 && nlevels <= SD_MAX_LEVELS &&
                 (monocular == 0 || monocular == 1) && cam5[0] > 0 && cam5[1] > 0,
             SD_ERR_INVALID_ARG, "bad arguments");
  for (int i = 0; i < n1; i++)
    SD_REQUIRE(matches12[i] >= -1 && matches12[i] < n2, SD_ERR_INVALID_ARG, "matches12 entry outside [-1, n2)");
  if (n1 == 0) return SD_OK;
  const size_t cap = (size_t)std::max(std::max(n1, n2), 1);
  std::vector<int32_t> m(cap, -1);
  std::memcpy(m.data(), matches12, (size_t)n1 * 4);
  Blob b;
  const size_t o_k1u = b.reserve(cap, kps1_un, n1), o_k1 = b.reserve(cap, kps1, n1);
  const size_t o_k2u = b.reserve(cap, kps2_un, n2), o_k2 = b.reserve(cap, kps2, n2);
  const size_t o_u1 = b.reserve(cap, uright1, n1), o_u2 = b.reserve(cap, uright2, n2);
  const size_t o_z1 = b.reserve(cap, depth1, n1), o_z2 = b.reserve(cap, depth2, n2), o_m = b.reserve(cap, m.data(), cap);
  const size_t o_T1 = b.reserve(16, Tcw1_cm16, 16), o_T2 = b.reserve(16, Tcw2_cm16, 16), o_med = b.reserve(1, &median_depth, 1);
  const size_t o_sf = b.reserve(nlevels, scale_factors, nlevels), o_s2 = b.reserve(nlevels, level_sigma2, nlevels);
  const size_t o_v = b.reserve<uint8_t>(cap), o_b = b.reserve<uint8_t>(cap), o_X = b.reserve<double>(cap * 3);
  SD_TRY(b.run("sd_debug_triangulate", [&] {
    TriangIn a = {b.dev<sd_keypoint>(o_k1u), b.dev<sd_keypoint>(o_k1), b.dev<sd_keypoint>(o_k2u), b.dev<sd_keypoint>(o_k2),
                  b.dev<int32_t>(o_m), b.dev<float>(o_u1), b.dev<float>(o_u2), b.dev<float>(o_z1), b.dev<float>(o_z2),
                  b.dev<double>(o_T1), b.dev<double>(o_T2), b.dev<float>(o_med), b.dev<float>(o_sf), b.dev<float>(o_s2),
                  0, 0, 0, 0, 0, 0, 0, 0, 0, nlevels, (int)cap, -1, monocular, b.dev<uint8_t>(o_v), b.dev<uint8_t>(o_b),
                  b.dev<double>(o_X)};
    set_camera(a, make_cam(cam5[0], cam5[1], cam5[2], cam5[3], cam5[4], 0, 0, 0, 0), 1.5f * scale_factor);   // (no image bounds here)
    return launch_k_triangulate(a, 1, 0);
  }));
  b.take(verdict, o_v, (size_t)n1);
  b.take(branch, o_b, (size_t)n1);
  b.take(Xw, o_X, (size_t)n1 * 24);
  return SD_OK;
}

}  // extern "C"
