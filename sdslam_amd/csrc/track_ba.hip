// Optimizer::LocalBundleAdjustment on MI355X (reference src/Optimizer.cc:417-714) with the parts of g2o it runs, restated from
//   OptimizationAlgorithmLevenberg::solve / computeLambdaInit / computeScale   src/extra/g2o/core/optimization_algorithm_levenberg.cpp:61-189
//   BlockSolver::buildSystem / setLambda (Hpp AND Hll) / solve (Schur) / restoreDiagonal   core/block_solver.hpp
//   SparseOptimizer::initializeOptimization(level) (a vertex without an edge of the level is not active), push / pop
//   BaseBinaryEdge::constructQuadraticForm, robustInformation = rho[1] * information, RobustKernelHuber
//   EdgeSE3ProjectXYZ / EdgeStereoSE3ProjectXYZ, SE3Quat (track_se3.h), LinearSolverEigen (fails on a zero pivot only)
// tests/ba_ref.py is the same restatement in numpy.
// Optimizer::BundleAdjustment (:46-219, sd_track_global_ba, tests/gba_ref.py) runs on the same kernels: BaProblem::mode and the
// fields beside it say what differs, and above SD_BA_MAX_FREE_KF free cameras the k_gba_* kernels factorise the reduced system.
//
// The problem: points = the list of sd_track_set_observations (CSR), one edge per observation that is neither of a bad point
// nor of a bad keyframe, in CSR order.  Cameras 0 .. n_kf - 1 carry a role: 1 local (a free vertex, at most SD_BA_MAX_FREE_KF),
// 2 local and fixed, 0 fixed if observed.  Free camera number s ("slot") is the s-th camera with role 1.
//
// Control flow stays on the device.  The host queues the worst case -- per round (5, then 10 iterations) and per iteration one
// linearisation and ten trials -- and every kernel reads the state record (BaState) first and returns when its step is not the
// one the record asks for: a kernel is told (iteration, trial) by the host and runs if the record says the same.  Only the
// one-workgroup kernels (setup, round_begin, iter_begin, decide) write the record's control fields; k_ba_classify adds to its two
// counters (info16[12], [13]) with integer atomics.  No workgroup waits for another one.
//   k_ba_gather       thread per point: its observations -> per-edge camera, measurement, information, flags
//   k_ba_setup        one workgroup: refusals, point status, slots, SE3Quat of every pose, both estimate buffers, the record
//   k_ba_index        one workgroup: the camera-major edge lists of the free cameras, each in edge order
//   k_ba_round_begin  one workgroup: the active vertices of the round's level-0 edges
//   per iteration:  k_ba_linearise (lane per edge: error, chi2, Huber rho, both Jacobians), k_ba_sum_points (wave per point:
//     Hll, bl over its edges in CSR order), k_ba_sum_cameras (wave per free camera: Hpp, bp over its list in order),
//     k_ba_iter_begin (chi2 of the iteration, lambda at iteration 0)
//   per trial:  k_ba_schur (wave per block (i <= j) of S = Hpp + lambda I - sum Hpl (Hll + lambda I)^-1 Hlp, and b), k_ba_solve
//     (one workgroup: LDL^T of S, packed lower triangle in LDS, and both substitutions), k_ba_update (back-substitution per point,
//     oplus of every vertex into the OTHER estimate buffer: push / pop is two buffers), k_ba_errors (computeActiveErrors at the
//     trial), k_ba_decide (rho, accept / reject, lambda, _nBad, the exits)
//   k_ba_classify     lane per edge, after each round: level 1 / obs_erase
//   k_ba_finish       outputs, and the write-back into Tref / Tcur / Xw of the row
// Determinism: no floating-point atomics.  A sum over edges is taken by one lane in list order (chunks of 64 edges: the lanes
// compute the terms, LDS holds them, the owner adds them in order); a sum over all edges or vertices (chi2, computeScale) is a
// strided partial per thread and a fixed tree.  e->chi2() of the classification reads `err`, which every computeActiveErrors
// overwrites for the active edges only: after a rejected last trial it holds the rejected step's errors, for a level-1 edge in
// round 2 round 1's last.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstddef>
#include <cstring>
#include <type_traits>
#include <vector>

#include "sd_wave.h"
#include "track_handle.h"
#include "track_se3.h"

namespace sd {

enum { BA_LIVE = 1, BA_STEREO = 2, BA_LEVEL1 = 4, BA_NOT_RESIDENT = 8, BA_BAD_INDEX = 16, BA_NO_VERTEX = 32 /* k_ba_setup's own */ };
enum { BA_EXIT_NOT_RUN = 0, BA_EXIT_NBAD = 1, BA_EXIT_QMAX = 2, BA_EXIT_RHO_ZERO = 3, BA_EXIT_ITERATIONS = 4 };   // poseopt_oracle.cc
constexpr int BA_K = SD_BA_MAX_FREE_KF, BA_N = 6 * BA_K, BA_PACKED = BA_N * (BA_N + 1) / 2;
constexpr int BA_EDGE_DOUBLES = 3 + 1 + 3 + 1 + 9 + 18 + 3 + 1;
constexpr int GBA_NB = 48;   // the panel of the blocked factorisation: 8 cameras; a block with its padding is 18 KB of LDS

struct BaState {
  int32_t status, round, round_live, iter, max_iter, trial_live, qmax, nbad, robust, cur, solve_ok, n_slots;
  double lambda, ni, cur_chi, ini_chi, rho;
  int32_t info[16];
};

static __device__ __forceinline__ bool ba_iter_wanted(const BaState* st, int it) { return st->status == 0 && st->round_live && st->iter == it; }
static __device__ __forceinline__ bool ba_trial_wanted(const BaState* st, int it, int q) {
  return ba_iter_wanted(st, it) && st->trial_live && st->qmax == q;
}

void ba_carve(BaBuffers& b, uint8_t* base, size_t P, size_t E, size_t n_kf, size_t kcap) {
  kcap = std::max<size_t>(kcap, BA_K);   // k_ba_solve writes BA_N entries of xp whatever the problem's size
  const size_t n = 6 * kcap, cw = (kcap + 31) / 32;
  size_t o = 0;
  auto take = [&](auto** p, size_t count) {
    using T = std::remove_pointer_t<std::remove_pointer_t<decltype(p)>>;
    *p = (T*)(base + o);
    o = align_up(o + std::max<size_t>(count, 1) * sizeof(T), 16);
  };
  take(&b.st, 1);
  take(&b.e_meas, E * 3); take(&b.e_info, E); take(&b.err, E * 3); take(&b.chi2r, E); take(&b.Jl, E * 9); take(&b.Jp, E * 18);
  take(&b.wr, E * 3); take(&b.w, E);
  take(&b.Hll, P * 9); take(&b.bl, P * 3); take(&b.X, 2 * P * 3); take(&b.v_scale, n_kf + P);
  take(&b.Hpp, kcap * 36); take(&b.bp, kcap * 6); take(&b.pose, 2 * n_kf * 8);
  // S: the packed lower triangle and one more row, the right-hand side as the blocked factorisation carries it (k_gba_diag)
  take(&b.S, (n + 1) * (n + 2) / 2); take(&b.bs, n); take(&b.xp, n);
  take(&b.W, kcap > BA_K ? (n + 1) * GBA_NB : 0); take(&b.covis, kcap * cw);
  take(&b.T_out, n_kf * 16); take(&b.X_out, P * 3);
  take(&b.e_cam, E); take(&b.e_pt, E); take(&b.clist, E); take(&b.coff, kcap + 1); take(&b.slot, n_kf); take(&b.slot_cam, kcap);
  take(&b.e_flag, E); take(&b.p_active, P); take(&b.p_status, P); take(&b.c_has, n_kf); take(&b.c_act, n_kf); take(&b.erase, E);
  take(&b.role, n_kf);
  b.bytes = o;
  b.cap_points = P; b.cap_obs = E; b.n_kf = (int)n_kf; b.kcap = (int)kcap;
}
size_t ba_bytes(size_t P, size_t E, size_t n_kf, size_t kcap) {
  BaBuffers b{};
  ba_carve(b, nullptr, P, E, n_kf, kcap);
  return b.bytes;
}

// Where the problem comes from and where the write-back goes
struct BaProblem {
  const int32_t* off;        // [n_points + 1]
  const uint8_t* point_bad;  // or NULL
  const uint8_t* kf_bad;     // or NULL
  int n_points, n_obs, n_kf;
  // the resident path: observations as (frame, kp) of the extractors; camera f < n_kf - 1 is ref frame f, camera n_kf - 1 the current keyframe
  const int32_t* frame;
  const int32_t* kp;
  const sd_keypoint* ref_kps;
  const int32_t* ref_nkp;
  const float* ref_ur;
  int ref_cap, n_ref;
  const sd_keypoint* cur_kps;
  const int32_t* cur_nkp;
  const float* cur_ur;
  int cur_cap, cur_frame;
  const float* inv_sigma2;
  int nlevels;
  const double* Tref;        // [n_kf - 1][16]
  const double* Tcur;        // [16]
  // the debug path: per edge its camera and measurement; poses [n_kf][16]
  const int32_t* d_kf;       // NULL: resident
  const float* d_uv;
  const float* d_ur;
  const float* d_inv;
  const double* d_T;
  double* Xw;                // [n_points][3]: read, and written by the write-back
  double* wb_Tref;           // NULL: no write-back
  double* wb_Tcur;
  double fx, fy, cx, cy, bf;
  // what tells the two callers apart.  mode 0: LocalBundleAdjustment (two rounds of 5 and 10 iterations, the level-1 / erase
  // classification, role 0 = a fixed camera if observed); mode 1: BundleAdjustment (one optimize(n_iterations), robust or not,
  // role 0 = no vertex: an edge to it refuses the call)
  int mode, n_iterations, robust;
  int kcap;                  // the free cameras the scratch holds: SD_BA_MAX_FREE_KF for mode 0
  double delta_mono, delta_stereo;   // the Huber deltas where the kernel is on
};
static void ba_set_mode(BaProblem& pr, int mode, int n_iterations, int robust, int kcap) {
  pr.mode = mode; pr.n_iterations = n_iterations; pr.robust = robust; pr.kcap = kcap;
  pr.delta_mono = (double)(float)std::sqrt(mode ? 5.99 : 5.991);   // thHuber2D = sqrt(5.99) (sic, Optimizer.cc:87); sqrt(5.991) at :520
  pr.delta_stereo = (double)(float)std::sqrt(7.815);
}

static __device__ __forceinline__ const double* ba_pose_in(const BaProblem& pr, int c) {
  if (pr.d_kf) return pr.d_T + (size_t)c * 16;
  return c < pr.n_kf - 1 ? pr.Tref + (size_t)c * 16 : pr.Tcur;
}

__global__ void k_ba_gather(BaProblem pr, BaBuffers b) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  // After sd_track_erase_observations the lists end at off[n_points], before the n_obs entries the block was packed for (only
  // the device knows where): the entries behind the end are nobody's edges.  Every kernel that walks e < n_obs asks e_flag first.
  for (int e = pr.off[pr.n_points] + p; e < pr.n_obs; e += gridDim.x * blockDim.x) b.e_flag[e] = b.erase[e] = 0;
  if (p >= pr.n_points) return;
  const bool pbad = pr.point_bad && pr.point_bad[p];
  for (int e = pr.off[p]; e < pr.off[p + 1]; e++) {
    b.e_pt[e] = p;
    int flag = 0, cam = 0;
    float u = 0.f, v = 0.f, ur = -1.f, inv = 0.f;
    if (!pbad && !(pr.kf_bad && pr.kf_bad[e])) {
      if (pr.d_kf) {
        cam = pr.d_kf[e];
        if (cam == -2) flag = BA_NOT_RESIDENT;
        else if (cam < 0 || cam >= pr.n_kf) flag = BA_BAD_INDEX;
        else {
          flag = BA_LIVE;
          u = pr.d_uv[2 * (size_t)e]; v = pr.d_uv[2 * (size_t)e + 1]; ur = pr.d_ur[e]; inv = pr.d_inv[e];
        }
      } else {
        const int fr = pr.frame[e], k = pr.kp[e];
        const bool cur = fr == -1;
        if (fr == -2) flag = BA_NOT_RESIDENT;
        else if (fr < -2 || fr >= pr.n_ref || (cur && pr.cur_frame < 0)) flag = BA_BAD_INDEX;
        else {
          const int f = cur ? pr.cur_frame : fr, cap = cur ? pr.cur_cap : pr.ref_cap;
          const int nk = min((cur ? pr.cur_nkp : pr.ref_nkp)[f], cap);
          if (k < 0 || k >= nk) flag = BA_BAD_INDEX;
          else {
            const sd_keypoint kq = (cur ? pr.cur_kps : pr.ref_kps)[(size_t)f * cap + k];
            flag = BA_LIVE;
            cam = cur ? pr.n_kf - 1 : fr;
            u = kq.x; v = kq.y;
            ur = cur ? pr.cur_ur[(size_t)(pr.cur_frame) * cap + k] : pr.ref_ur[(size_t)f * cap + k];
            inv = pr.inv_sigma2[min(max(kq.octave, 0), pr.nlevels - 1)];
          }
        }
      }
    }
    const bool stereo = !(ur < 0.f);   // mvuRight < 0: monocular
    if ((flag & BA_LIVE) && stereo) flag |= BA_STEREO;
    b.e_cam[e] = (flag & BA_LIVE) ? cam : 0;
    b.e_flag[e] = (uint8_t)flag;
    b.e_meas[(size_t)e * 3] = u; b.e_meas[(size_t)e * 3 + 1] = v; b.e_meas[(size_t)e * 3 + 2] = stereo ? (double)ur : 0.0;
    b.e_info[e] = inv;
    b.err[(size_t)e * 3] = b.err[(size_t)e * 3 + 1] = b.err[(size_t)e * 3 + 2] = 0.0;
    b.chi2r[e] = 0.0;
    b.erase[e] = 0;
  }
}

static __device__ __forceinline__ void ba_q_to_R(const double* q, double R[3][3]) {   // Eigen toRotationMatrix
  const double tx = 2 * q[0], ty = 2 * q[1], tz = 2 * q[2];
  const double twx = tx * q[3], twy = ty * q[3], twz = tz * q[3];
  const double txx = tx * q[0], txy = ty * q[0], txz = tz * q[0];
  const double tyy = ty * q[1], tyz = tz * q[1], tzz = tz * q[2];
  R[0][0] = 1 - (tyy + tzz); R[0][1] = txy - twz; R[0][2] = txz + twy;
  R[1][0] = txy + twz; R[1][1] = 1 - (txx + tzz); R[1][2] = tyz - twx;
  R[2][0] = txz - twy; R[2][1] = tyz + twx; R[2][2] = 1 - (txx + tyy);
}

static __device__ __forceinline__ Se3q ba_load_pose(const double* p) {
  Se3q s;
  for (int i = 0; i < 4; i++) s.q[i] = p[i];
  for (int i = 0; i < 3; i++) s.t[i] = p[4 + i];
  return s;
}
static __device__ __forceinline__ void ba_store_pose(double* p, const Se3q& s) {
  for (int i = 0; i < 4; i++) p[i] = s.q[i];
  for (int i = 0; i < 3; i++) p[4 + i] = s.t[i];
  p[7] = 0.0;
}

__global__ __launch_bounds__(256) void k_ba_setup(BaProblem pr, BaBuffers b) {
  __shared__ int s_flags, s_cnt[3], s_status;
  const int t = threadIdx.x, nt = blockDim.x;
  if (t == 0) s_flags = s_cnt[0] = s_cnt[1] = s_cnt[2] = 0;
  for (int c = t; c < pr.n_kf; c += nt) b.c_has[c] = b.c_act[c] = 0;
  if (pr.mode)
    for (int k = t; k < pr.kcap * ((pr.kcap + 31) / 32); k += nt) b.covis[k] = 0;
  __syncthreads();
  int fl = 0, mono = 0, st = 0;
  for (int e = t; e < pr.n_obs; e += nt) {
    const int f = b.e_flag[e];
    fl |= f & (BA_NOT_RESIDENT | BA_BAD_INDEX);
    if (f & BA_LIVE) {
      b.c_has[b.e_cam[e]] = 1;
      if (pr.mode && b.role[b.e_cam[e]] == 0) fl |= BA_NO_VERTEX;
      if (f & BA_STEREO) st++; else mono++;
    }
  }
  if (fl) atomicOr(&s_flags, fl);
  atomicAdd(&s_cnt[0], mono);
  atomicAdd(&s_cnt[1], st);
  __syncthreads();
  if (t == 0) {
    int n_free = 0, n_fixed = 0;
    for (int c = 0; c < pr.n_kf; c++) {
      const int role = b.role[c];
      b.slot[c] = -1;
      if (role == 1) {
        if (n_free < pr.kcap) { b.slot[c] = n_free; b.slot_cam[n_free] = c; }
        n_free++;
      } else if (role == 2 || b.c_has[c]) n_fixed++;
    }
    const int status = (s_flags & BA_NOT_RESIDENT) ? SD_BA_NOT_RESIDENT : (s_flags & BA_BAD_INDEX) ? SD_BA_BAD_INDEX
                       : n_free > pr.kcap ? SD_BA_TOO_MANY_KF : (s_flags & BA_NO_VERTEX) ? SD_BA_NO_VERTEX : SD_BA_OK;
    s_status = status;
    BaState* S = b.st;
    S->status = status; S->round = 0; S->round_live = 0; S->iter = 0; S->max_iter = 0; S->trial_live = 0; S->qmax = 0; S->nbad = 0;
    S->robust = 1; S->cur = 0; S->solve_ok = 0; S->n_slots = min(n_free, pr.kcap);
    S->lambda = -1.0; S->ni = 2.0; S->cur_chi = S->ini_chi = S->rho = 0.0;
    for (int i = 0; i < 16; i++) S->info[i] = 0;
    S->info[0] = status;
    if (status == SD_BA_OK) { S->info[1] = n_free; S->info[2] = n_fixed; S->info[4] = s_cnt[0]; S->info[5] = s_cnt[1]; }
  }
  __syncthreads();
  const int status = s_status;
  int n_opt = 0;
  for (int p = t; p < pr.n_points; p += nt) {
    int any = 0;
    for (int e = pr.off[p]; e < pr.off[p + 1]; e++) any |= b.e_flag[e];
    const int ps = (any & BA_BAD_INDEX) ? SD_BA_POINT_BAD_INDEX : (status == SD_BA_OK && (any & BA_LIVE)) ? SD_BA_POINT_OPTIMISED : SD_BA_POINT_SKIPPED;
    b.p_status[p] = (uint8_t)ps;
    b.p_active[p] = 0;
    n_opt += ps == SD_BA_POINT_OPTIMISED;
    for (int k = 0; k < 3; k++) {
      const double x = pr.Xw[(size_t)p * 3 + k];
      b.X[(size_t)p * 3 + k] = b.X[((size_t)pr.n_points + p) * 3 + k] = b.X_out[(size_t)p * 3 + k] = x;
    }
  }
  atomicAdd(&s_cnt[2], n_opt);
  for (int c = t; c < pr.n_kf; c += nt) {
    const double* T = ba_pose_in(pr, c);
    for (int i = 0; i < 16; i++) b.T_out[(size_t)c * 16 + i] = T[i];
    double R[3][3], tt[3];
    for (int r = 0; r < 3; r++) {
      for (int k = 0; k < 3; k++) R[r][k] = T[k * 4 + r];
      tt[r] = T[12 + r];
    }
    const Se3q s = se3_from_Rt(R, tt);   // Converter::toSE3Quat
    ba_store_pose(b.pose + (size_t)c * 8, s);
    ba_store_pose(b.pose + ((size_t)pr.n_kf + c) * 8, s);
  }
  __syncthreads();
  if (t == 0) b.st->info[3] = s_cnt[2];
}

// The edges of free camera `slot`, in edge order: coff[slot] .. coff[slot + 1] - 1 of clist
__global__ __launch_bounds__(1024) void k_ba_index(BaProblem pr, BaBuffers b) {
  __shared__ int s_n[SD_GBA_MAX_FREE_KF], s_off[SD_GBA_MAX_FREE_KF + 1];
  if (b.st->status != 0) return;
  const int K = b.st->n_slots;   // a slot past it has no camera and no edge
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, n_waves = blockDim.x >> 6;
  const unsigned long long lt = lanemask_lt(lane);
  for (int pass = 0; pass < 2; pass++) {
    for (int s = wave; s < K; s += n_waves) {
      int n = pass ? s_off[s] : 0;
      for (int e0 = 0; e0 < pr.n_obs; e0 += 64) {
        const int e = e0 + lane;
        const bool mine = e < pr.n_obs && (b.e_flag[e] & BA_LIVE) && b.slot[b.e_cam[e]] == s;
        const int pos = wave_append(mine, lt, n);
        if (pass && mine) b.clist[pos] = e;
      }
      if (!pass && lane == 0) s_n[s] = n;
    }
    __syncthreads();
    if (!pass && threadIdx.x == 0) {
      int o = 0;
      for (int s = 0; s < K; s++) { s_off[s] = o; b.coff[s] = o; o += s_n[s]; }
      for (int s = K; s <= pr.kcap; s++) b.coff[s] = o;
    }
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void k_ba_round_begin(BaProblem pr, BaBuffers b, int round) {
  __shared__ int s_any;
  BaState* S = b.st;
  if (S->status != 0) return;
  const int t = threadIdx.x, nt = blockDim.x;
  if (t == 0) s_any = 0;
  for (int c = t; c < pr.n_kf; c += nt) b.c_act[c] = 0;
  __syncthreads();
  int any = 0;
  for (int p = t; p < pr.n_points; p += nt) {
    int act = 0;
    for (int e = pr.off[p]; e < pr.off[p + 1]; e++) {
      const int f = b.e_flag[e];
      if ((f & BA_LIVE) && !(f & BA_LEVEL1)) {
        act = 1;
        if (b.slot[b.e_cam[e]] >= 0) b.c_act[b.e_cam[e]] = 1;
      }
    }
    b.p_active[p] = (uint8_t)act;
    any |= act;
  }
  if (any) atomicOr(&s_any, 1);
  __syncthreads();
  if (t == 0) {
    S->round = round; S->round_live = s_any; S->iter = 0; S->max_iter = pr.mode ? pr.n_iterations : round ? 10 : 5; S->trial_live = 0; S->qmax = 0; S->nbad = 0;
    S->robust = pr.mode ? pr.robust : round ? 0 : 1;   // e->setRobustKernel(0) on every edge after round 1
    S->lambda = -1.0; S->ni = 2.0;
  }
}

// estimate().map(Xw) of an edge in estimate buffer `buf`
static __device__ __forceinline__ void ba_map(const BaProblem& pr, const BaBuffers& b, int buf, int e, Se3q* T, double* pc) {
  *T = ba_load_pose(b.pose + ((size_t)buf * pr.n_kf + b.e_cam[e]) * 8);
  const double* X = b.X + ((size_t)buf * pr.n_points + b.e_pt[e]) * 3;
  const double Xv[3] = {X[0], X[1], X[2]};
  double r[3];
  q_rotate(T->q, Xv, r);
  for (int i = 0; i < 3; i++) pc[i] = r[i] + T->t[i];
}

// computeError of either edge type; returns _error.dot(information() * _error)
static __device__ __forceinline__ double ba_error(const BaProblem& pr, const double* pc, const double* meas, bool stereo, double info, double* err) {
  if (!stereo) {
    const double px = pc[0] / pc[2], py = pc[1] / pc[2];   // project2d
    err[0] = meas[0] - (px * pr.fx + pr.cx);
    err[1] = meas[1] - (py * pr.fy + pr.cy);
    err[2] = 0.0;
    return err[0] * (info * err[0]) + err[1] * (info * err[1]);
  }
  const float invz = (float)(1.0 / pc[2]);   // const float invz = 1.0f / trans_xyz[2]
  const double r0 = pc[0] * invz * pr.fx + pr.cx, r1 = pc[1] * invz * pr.fy + pr.cy, r2 = r0 - pr.bf * invz;
  err[0] = meas[0] - r0; err[1] = meas[1] - r1; err[2] = meas[2] - r2;
  return err[0] * (info * err[0]) + err[1] * (info * err[1]) + err[2] * (info * err[2]);
}

static __device__ __forceinline__ void ba_huber(double e2, double delta, double* rho0, double* rho1) {
  const double dsqr = delta * delta;
  if (e2 <= dsqr) { *rho0 = e2; *rho1 = 1.0; }
  else { const double sq = sqrt(e2); *rho0 = 2 * sq * delta - dsqr; *rho1 = delta / sq; }
}

// computeActiveErrors of one edge in buffer `buf`: err, and its term of activeRobustChi2
static __device__ __forceinline__ void ba_edge_error(const BaProblem& pr, const BaBuffers& b, int buf, int e, int robust, double* rho1_out) {
  const int f = b.e_flag[e];
  const bool stereo = f & BA_STEREO;
  Se3q T;
  double pc[3], err[3];
  ba_map(pr, b, buf, e, &T, pc);
  const double chi2 = ba_error(pr, pc, b.e_meas + (size_t)e * 3, stereo, b.e_info[e], err);
  for (int i = 0; i < 3; i++) b.err[(size_t)e * 3 + i] = err[i];
  double rho0 = chi2, rho1 = 1.0;
  if (robust) ba_huber(chi2, stereo ? pr.delta_stereo : pr.delta_mono, &rho0, &rho1);
  b.chi2r[e] = rho0;
  if (rho1_out) *rho1_out = rho1;
}

__global__ __launch_bounds__(256) void k_ba_linearise(BaProblem pr, BaBuffers b, int it) {
  const BaState* S = b.st;
  if (!ba_iter_wanted(S, it)) return;
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= pr.n_obs) return;
  const int f = b.e_flag[e];
  if (!(f & BA_LIVE) || (f & BA_LEVEL1)) return;
  const bool stereo = f & BA_STEREO;
  double rho1;
  ba_edge_error(pr, b, S->cur, e, S->robust, &rho1);
  Se3q T;
  double pc[3], R[3][3];
  ba_map(pr, b, S->cur, e, &T, pc);
  ba_q_to_R(T.q, R);
  const double x = pc[0], y = pc[1], z = pc[2], z_2 = z * z, fx = pr.fx, fy = pr.fy, bf = pr.bf;
  double* Jl = b.Jl + (size_t)e * 9;
  double* Jp = b.Jp + (size_t)e * 18;
  if (stereo) {
    for (int c = 0; c < 3; c++) {
      Jl[c] = -fx * R[0][c] / z + fx * x * R[2][c] / z_2;
      Jl[3 + c] = -fy * R[1][c] / z + fy * y * R[2][c] / z_2;
      Jl[6 + c] = Jl[c] - bf * R[2][c] / z_2;
    }
  } else {   // EdgeSE3ProjectXYZ: -1. / z * tmp * R, tmp = [fx 0 -x / z * fx; 0 fy -y / z * fy]
    const double a = -1. / z, t02 = -x / z * fx, t12 = -y / z * fy;
    for (int c = 0; c < 3; c++) {
      Jl[c] = (a * fx) * R[0][c] + (a * t02) * R[2][c];
      Jl[3 + c] = (a * fy) * R[1][c] + (a * t12) * R[2][c];
      Jl[6 + c] = 0.0;
    }
  }
  Jp[0] = x * y / z_2 * fx; Jp[1] = -(1 + (x * x / z_2)) * fx; Jp[2] = y / z * fx; Jp[3] = -1. / z * fx; Jp[4] = 0; Jp[5] = x / z_2 * fx;
  Jp[6] = (1 + y * y / z_2) * fy; Jp[7] = -x * y / z_2 * fy; Jp[8] = -x / z * fy; Jp[9] = 0; Jp[10] = -1. / z * fy; Jp[11] = y / z_2 * fy;
  if (stereo) {
    Jp[12] = Jp[0] - bf * y / z_2; Jp[13] = Jp[1] + bf * x / z_2; Jp[14] = Jp[2]; Jp[15] = Jp[3]; Jp[16] = 0; Jp[17] = Jp[5] - bf / z_2;
  } else {
    for (int k = 12; k < 18; k++) Jp[k] = 0.0;
  }
  const double info = b.e_info[e];
  b.w[e] = rho1 * info;                                                                  // robustInformation
  for (int d = 0; d < 3; d++) b.wr[(size_t)e * 3 + d] = -(info * b.err[(size_t)e * 3 + d]) * rho1;   // omega_r = -omega * error, *= rho[1]
}

// Hll and bl of point p: lanes 0..8 own an entry of Hll, 9..11 one of bl, each summing the point's edges in CSR order
__global__ __launch_bounds__(256) void k_ba_sum_points(BaProblem pr, BaBuffers b, int it) {
  if (!ba_iter_wanted(b.st, it)) return;
  const int lane = threadIdx.x & 63, p = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
  if (p >= pr.n_points || lane >= 12) return;
  double acc = 0.0;
  if (b.p_active[p])
    for (int e = pr.off[p]; e < pr.off[p + 1]; e++) {
      const int f = b.e_flag[e];
      if (!(f & BA_LIVE) || (f & BA_LEVEL1)) continue;
      const double* Jl = b.Jl + (size_t)e * 9;
      if (lane < 9) {
        const int r = lane / 3, c = lane % 3;
        const double w = b.w[e];
        acc += (Jl[r] * w * Jl[c] + Jl[3 + r] * w * Jl[3 + c]) + Jl[6 + r] * w * Jl[6 + c];
      } else {
        const int r = lane - 9;
        const double* wr = b.wr + (size_t)e * 3;
        acc += (Jl[r] * wr[0] + Jl[3 + r] * wr[1]) + Jl[6 + r] * wr[2];
      }
    }
  if (lane < 9) b.Hll[(size_t)p * 9 + lane] = acc;
  else b.bl[(size_t)p * 3 + lane - 9] = acc;
}

// In-order sum of per-lane terms: the lanes of a 64-thread workgroup hold NV terms each for `cnt` consecutive list entries; lane k < NV
// adds term k of entries 0 .. cnt - 1 to acc, in that order
template <int NV>
static __device__ __forceinline__ void ba_ordered_add(double* s_term, const double (&v)[NV], int lane, int cnt, double& acc) {
#pragma unroll
  for (int k = 0; k < NV; k++) s_term[lane * NV + k] = v[k];
  __syncthreads();
  if (lane < NV)
    for (int l = 0; l < cnt; l++) acc += s_term[l * NV + lane];
  __syncthreads();
}

// Hpl of an edge = Jp^T (w) Jl, [6][3]
static __device__ __forceinline__ void ba_hpl(const BaBuffers& b, int e, double (&H)[18]) {
  const double* Jp = b.Jp + (size_t)e * 18;
  const double* Jl = b.Jl + (size_t)e * 9;
  const double w = b.w[e];
#pragma unroll
  for (int r = 0; r < 6; r++)
#pragma unroll
    for (int a = 0; a < 3; a++) H[r * 3 + a] = (Jp[r] * w * Jl[a] + Jp[6 + r] * w * Jl[3 + a]) + Jp[12 + r] * w * Jl[6 + a];
}

// Hpp (lanes 0..35) and bp (36..41) of free camera blockIdx.x over its edge list in order
__global__ __launch_bounds__(64) void k_ba_sum_cameras(BaProblem pr, BaBuffers b, int it) {
  __shared__ double s_term[64 * 42];
  if (!ba_iter_wanted(b.st, it)) return;
  const int lane = threadIdx.x, s = blockIdx.x;
  const int o0 = b.coff[s], n = b.coff[s + 1] - o0;
  double acc = 0.0;
  for (int base = 0; base < n; base += 64) {
    const int cnt = min(64, n - base);
    double v[42];
#pragma unroll
    for (int k = 0; k < 42; k++) v[k] = 0.0;
    if (lane < cnt) {
      const int e = b.clist[o0 + base + lane];
      if (!(b.e_flag[e] & BA_LEVEL1)) {
        const double* Jp = b.Jp + (size_t)e * 18;
        const double* wr = b.wr + (size_t)e * 3;
        const double w = b.w[e];
#pragma unroll
        for (int r = 0; r < 6; r++) {
#pragma unroll
          for (int c = 0; c < 6; c++) v[r * 6 + c] = (Jp[r] * w * Jp[c] + Jp[6 + r] * w * Jp[6 + c]) + Jp[12 + r] * w * Jp[12 + c];
          v[36 + r] = (Jp[r] * wr[0] + Jp[6 + r] * wr[1]) + Jp[12 + r] * wr[2];
        }
      }
    }
    ba_ordered_add<42>(s_term, v, lane, cnt, acc);
  }
  if (lane < 36) b.Hpp[(size_t)s * 36 + lane] = acc;
  else if (lane < 42) b.bp[(size_t)s * 6 + lane - 36] = acc;
}

// Sum (or maximum) over the workgroup in a fixed tree; every thread gets it.  s_red: blockDim.x doubles
static __device__ __forceinline__ double ba_block_reduce(double v, double* s_red, bool take_max) {
  const int t = threadIdx.x;
  __syncthreads();
  s_red[t] = v;
  __syncthreads();
  for (int step = blockDim.x >> 1; step > 0; step >>= 1) {
    if (t < step) s_red[t] = take_max ? fmax(s_red[t], s_red[t + step]) : s_red[t] + s_red[t + step];
    __syncthreads();
  }
  return s_red[0];
}

// activeRobustChi2: the terms of the active edges, a strided partial per thread, then the tree
static __device__ __forceinline__ double ba_active_chi2(const BaProblem& pr, const BaBuffers& b, double* s_red) {
  double part = 0.0;
  for (int e = threadIdx.x; e < pr.n_obs; e += blockDim.x) {
    const int f = b.e_flag[e];
    if ((f & BA_LIVE) && !(f & BA_LEVEL1)) part += b.chi2r[e];
  }
  return ba_block_reduce(part, s_red, false);
}

__global__ __launch_bounds__(1024) void k_ba_iter_begin(BaProblem pr, BaBuffers b, int it) {
  __shared__ double s_red[1024];
  BaState* S = b.st;
  if (!ba_iter_wanted(S, it)) return;
  const double chi = ba_active_chi2(pr, b, s_red);
  double lam = 0.0;
  if (it == 0) {   // computeLambdaInit: tau * the largest |diagonal entry| of the active vertices
    double m = 0.0;
    for (int p = threadIdx.x; p < pr.n_points; p += blockDim.x)
      if (b.p_active[p])
        for (int k = 0; k < 3; k++) m = fmax(m, fabs(b.Hll[(size_t)p * 9 + k * 4]));
    for (int i = threadIdx.x; i < S->n_slots * 6; i += blockDim.x)
      if (b.c_act[b.slot_cam[i / 6]]) m = fmax(m, fabs(b.Hpp[(size_t)(i / 6) * 36 + (i % 6) * 7]));
    lam = 1e-5 * ba_block_reduce(m, s_red, true);
  }
  if (threadIdx.x == 0) {
    if (it == 0) { S->lambda = lam; S->ni = 2.0; S->nbad = 0; }
    S->cur_chi = S->ini_chi = chi;
    S->rho = 0.0; S->qmax = 0; S->trial_live = 1;
  }
}

// (Hll + lambda I)^-1 of point p
static __device__ __forceinline__ void ba_dinv(const BaBuffers& b, int p, double lambda, double (&D)[9]) {
  const double* H = b.Hll + (size_t)p * 9;
  const double a = H[0] + lambda, bb = H[1], c = H[2], d = H[3], e = H[4] + lambda, f = H[5], g = H[6], h = H[7], i = H[8] + lambda;
  const double c00 = e * i - f * h, c01 = f * g - d * i, c02 = d * h - e * g;
  const double inv_det = 1.0 / ((a * c00 + bb * c01) + c * c02);
  D[0] = c00 * inv_det; D[1] = (c * h - bb * i) * inv_det; D[2] = (bb * f - c * e) * inv_det;
  D[3] = c01 * inv_det; D[4] = (a * i - c * g) * inv_det; D[5] = (c * d - a * f) * inv_det;
  D[6] = c02 * inv_det; D[7] = (bb * g - a * h) * inv_det; D[8] = (a * e - bb * d) * inv_det;
}

// Block (i, j), i <= j, of the reduced system, one 64-lane workgroup each: lanes 0..35 own an entry of the block, 36..41 (on the
// diagonal) one of b.  The terms come from camera i's edge list in order; an edge of point p contributes once per active edge of p
// on camera j.  S is stored as the packed lower triangle the solve reads.
__global__ __launch_bounds__(64) void k_ba_schur(BaProblem pr, BaBuffers b, int it, int q) {
  __shared__ double s_term[64 * 42];
  const BaState* S = b.st;
  if (!ba_trial_wanted(S, it, q)) return;
  const int lane = threadIdx.x, K = S->n_slots;
  int i = 0, rest = blockIdx.x;
  while (i < K && rest >= K - i) { rest -= K - i; i++; }
  if (i >= K) return;
  const int j = i + rest;
  const double lambda = S->lambda;
  const int o0 = b.coff[i], n = b.coff[i + 1] - o0;
  double acc = 0.0;
  if (pr.mode && i != j && !((b.covis[(size_t)i * ((pr.kcap + 31) / 32) + (j >> 5)] >> (j & 31)) & 1)) {   // no common point: the block is 0
    if (lane < 36) b.S[(size_t)(6 * j + lane % 6) * (6 * j + lane % 6 + 1) / 2 + 6 * i + lane / 6] = 0.0;
    return;
  }
  if (i == j) {
    if (lane < 36) acc = b.Hpp[(size_t)i * 36 + lane] + (lane % 7 == 0 ? lambda : 0.0);
    else if (lane < 42) acc = b.bp[(size_t)i * 6 + lane - 36];
  }
  const int cam_j = b.slot_cam[j];
  for (int base = 0; base < n; base += 64) {
    const int cnt = min(64, n - base);
    double v[42];
#pragma unroll
    for (int k = 0; k < 42; k++) v[k] = 0.0;
    if (lane < cnt) {
      const int e = b.clist[o0 + base + lane];
      if (!(b.e_flag[e] & BA_LEVEL1)) {
        const int p = b.e_pt[e];
        double D[9], H[18], M[18];
        ba_dinv(b, p, lambda, D);
        ba_hpl(b, e, H);
#pragma unroll
        for (int r = 0; r < 6; r++)
#pragma unroll
          for (int a = 0; a < 3; a++) M[r * 3 + a] = (H[r * 3] * D[a] + H[r * 3 + 1] * D[3 + a]) + H[r * 3 + 2] * D[6 + a];
        for (int e2 = pr.off[p]; e2 < pr.off[p + 1]; e2++) {
          const int f2 = b.e_flag[e2];
          if (!(f2 & BA_LIVE) || (f2 & BA_LEVEL1) || b.e_cam[e2] != cam_j) continue;
          double H2[18];
          ba_hpl(b, e2, H2);
#pragma unroll
          for (int r = 0; r < 6; r++)
#pragma unroll
            for (int c = 0; c < 6; c++) v[r * 6 + c] -= (M[r * 3] * H2[c * 3] + M[r * 3 + 1] * H2[c * 3 + 1]) + M[r * 3 + 2] * H2[c * 3 + 2];
        }
        if (i == j) {   // b_i -= Hpl (Dinv bl)
          const double* bl = b.bl + (size_t)p * 3;
#pragma unroll
          for (int r = 0; r < 6; r++) v[36 + r] = -((M[r * 3] * bl[0] + M[r * 3 + 1] * bl[1]) + M[r * 3 + 2] * bl[2]);
        }
      }
    }
    ba_ordered_add<42>(s_term, v, lane, cnt, acc);
  }
  if (lane < 36) {
    const int r = lane / 6, c = lane % 6;
    const int row = 6 * j + c, col = 6 * i + r;   // entry (6i + r, 6j + c) of the symmetric S, stored at (row >= col)
    if (i != j || c >= r) b.S[(size_t)row * (row + 1) / 2 + col] = acc;
  } else if (lane < 42 && i == j) {
    b.bs[6 * i + lane - 36] = acc;
  }
}

// LDL^T of S without pivoting, in index order, on the packed lower triangle in LDS; the forward substitution rides along, then
// the division by D and the backward substitution.  A zero pivot fails the solve (SimplicialLDLT's only failure): x = 0.
__global__ __launch_bounds__(256) void k_ba_solve(BaProblem pr, BaBuffers b, int it, int q) {
  __shared__ double s_A[BA_PACKED], s_col[BA_N], s_l[BA_N], s_y[BA_N];
  __shared__ int s_fail;
  BaState* S = b.st;
  if (!ba_trial_wanted(S, it, q)) return;
  const int t = threadIdx.x, tx = t & 15, ty = t >> 4, n = 6 * S->n_slots;
  for (int k = t; k < n * (n + 1) / 2; k += 256) s_A[k] = b.S[k];
  for (int k = t; k < n; k += 256) s_y[k] = b.bs[k];
  if (t == 0) s_fail = 0;
  __syncthreads();
  for (int k = 0; k < n; k++) {
    const double d = s_A[k * (k + 1) / 2 + k];
    if (d == 0.0) {   // uniform
      if (t == 0) s_fail = 1;
      break;
    }
    const double yk = s_y[k];
    for (int i = k + 1 + t; i < n; i += 256) {
      const double a = s_A[i * (i + 1) / 2 + k], l = a / d;
      s_col[i] = a;
      s_l[i] = l;
      s_A[i * (i + 1) / 2 + k] = l;
      s_y[i] -= l * yk;
    }
    __syncthreads();
    for (int i = k + 1 + ty; i < n; i += 16)
      for (int j = k + 1 + tx; j <= i; j += 16) s_A[i * (i + 1) / 2 + j] -= s_l[i] * s_col[j];
    __syncthreads();
  }
  __syncthreads();
  const bool ok = !s_fail;
  if (ok) {
    for (int k = t; k < n; k += 256) s_y[k] /= s_A[k * (k + 1) / 2 + k];
    __syncthreads();
    for (int k = n - 1; k > 0; k--) {
      const double yk = s_y[k];
      for (int i = t; i < k; i += 256) s_y[i] -= s_A[k * (k + 1) / 2 + i] * yk;
      __syncthreads();
    }
  }
  for (int k = t; k < BA_N; k += 256) b.xp[k] = (ok && k < n) ? s_y[k] : 0.0;
  if (t == 0) S->solve_ok = ok;
}

// update(x): thread p < n_points back-substitutes its point (cl = bl - Hlp xp, xl = Dinv cl) and adds; thread n_points + c does
// exp(x) * estimate of camera c.  The new estimates go into the other buffer; a vertex that is not active is copied.  v_scale:
// the vertex's terms of computeScale.
__global__ __launch_bounds__(256) void k_ba_update(BaProblem pr, BaBuffers b, int it, int q) {
  const BaState* S = b.st;
  if (!ba_trial_wanted(S, it, q)) return;
  const int t = blockIdx.x * blockDim.x + threadIdx.x, cur = S->cur, nb = 1 - cur;
  const double lambda = S->lambda;
  if (t < pr.n_points) {
    const int p = t;
    const double* X = b.X + ((size_t)cur * pr.n_points + p) * 3;
    double* Xn = b.X + ((size_t)nb * pr.n_points + p) * 3;
    double xl[3] = {0.0, 0.0, 0.0}, scale = 0.0;
    if (b.p_active[p] && S->solve_ok) {
      const double* bl = b.bl + (size_t)p * 3;
      double cl[3] = {bl[0], bl[1], bl[2]};
      for (int e = pr.off[p]; e < pr.off[p + 1]; e++) {
        const int f = b.e_flag[e];
        const int s = (f & BA_LIVE) && !(f & BA_LEVEL1) ? b.slot[b.e_cam[e]] : -1;
        if (s < 0) continue;
        double H[18];
        ba_hpl(b, e, H);
        const double* x = b.xp + 6 * s;
        for (int a = 0; a < 3; a++) {
          double dot = 0.0;
          for (int r = 0; r < 6; r++) dot += H[r * 3 + a] * x[r];
          cl[a] -= dot;
        }
      }
      double D[9];
      ba_dinv(b, p, lambda, D);
      for (int a = 0; a < 3; a++) {
        xl[a] = (D[a * 3] * cl[0] + D[a * 3 + 1] * cl[1]) + D[a * 3 + 2] * cl[2];
        scale += xl[a] * (lambda * xl[a] + bl[a]);
      }
    }
    for (int a = 0; a < 3; a++) Xn[a] = (b.p_active[p] && S->solve_ok) ? X[a] + xl[a] : X[a];
    b.v_scale[pr.n_kf + p] = scale;
  } else if (t < pr.n_points + pr.n_kf) {
    const int c = t - pr.n_points, s = b.slot[c];
    const double* P0 = b.pose + ((size_t)cur * pr.n_kf + c) * 8;
    double* P1 = b.pose + ((size_t)nb * pr.n_kf + c) * 8;
    double scale = 0.0;
    if (s >= 0 && b.c_act[c] && S->solve_ok) {
      double x[6];
      for (int r = 0; r < 6; r++) {
        x[r] = b.xp[6 * s + r];
        scale += x[r] * (lambda * x[r] + b.bp[(size_t)s * 6 + r]);
      }
      ba_store_pose(P1, se3q_mul(se3q_exp(x), ba_load_pose(P0)));   // VertexSE3Expmap::oplusImpl
    } else {
      for (int k = 0; k < 8; k++) P1[k] = P0[k];
    }
    b.v_scale[c] = scale;
  }
}

__global__ __launch_bounds__(256) void k_ba_errors(BaProblem pr, BaBuffers b, int it, int q) {
  const BaState* S = b.st;
  if (!ba_trial_wanted(S, it, q)) return;
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= pr.n_obs) return;
  const int f = b.e_flag[e];
  if ((f & BA_LIVE) && !(f & BA_LEVEL1)) ba_edge_error(pr, b, 1 - S->cur, e, S->robust, nullptr);
}

// The rest of OptimizationAlgorithmLevenberg::solve after computeActiveErrors of the trial, and SparseOptimizer::optimize's loop
__global__ __launch_bounds__(1024) void k_ba_decide(BaProblem pr, BaBuffers b, int it, int q) {
  __shared__ double s_red[1024];
  BaState* S = b.st;
  if (!ba_trial_wanted(S, it, q)) return;
  double temp_chi = ba_active_chi2(pr, b, s_red);
  double part = 0.0;
  for (int v = threadIdx.x; v < pr.n_kf + pr.n_points; v += blockDim.x) part += b.v_scale[v];
  double scale = ba_block_reduce(part, s_red, false);
  if (threadIdx.x != 0) return;
  if (!S->solve_ok) temp_chi = DBL_MAX;
  double rho = S->cur_chi - temp_chi;
  scale += 1e-3;
  rho /= scale;
  if (rho > 0 && isfinite(temp_chi)) {
    double alpha = 1. - pow((2 * rho - 1), 3.0);
    alpha = fmin(alpha, 2. / 3.);
    S->lambda *= fmax(1. / 3., alpha);
    S->ni = 2.0;
    S->cur_chi = temp_chi;
    S->cur = 1 - S->cur;   // discardTop: the trial is the estimate
  } else {
    S->lambda *= S->ni;
    S->ni *= 2;           // pop: the estimate buffer stays
  }
  S->rho = rho;
  const int qmax = S->qmax + 1, r = S->round;
  S->qmax = qmax;
  S->info[7 + 3 * r]++;   // trials
  if (rho < 0 && qmax < 10) return;   // the next trial
  S->trial_live = 0;
  S->info[6 + 3 * r]++;   // iterations
  int exit_taken = BA_EXIT_ITERATIONS;
  bool stop = S->iter + 1 >= S->max_iter;
  if (qmax == 10 || rho == 0) {
    exit_taken = qmax == 10 ? BA_EXIT_QMAX : BA_EXIT_RHO_ZERO;
    stop = true;
  } else {
    if ((S->ini_chi - S->cur_chi) * 1e3 < S->ini_chi) S->nbad++;
    else S->nbad = 0;
    if (S->nbad >= 3) { exit_taken = BA_EXIT_NBAD; stop = true; }
  }
  if (stop) { S->round_live = 0; S->info[8 + 3 * r] = exit_taken; }
  else S->iter++;
}

// e->chi2() > threshold || !e->isDepthPositive(): round 0 puts the edge on level 1, round 1 into obs_erase
__global__ __launch_bounds__(256) void k_ba_classify(BaProblem pr, BaBuffers b, int round) {
  BaState* S = b.st;
  if (S->status != 0) return;
  const int e = blockIdx.x * blockDim.x + threadIdx.x;
  if (e >= pr.n_obs) return;
  const int f = b.e_flag[e];
  if (!(f & BA_LIVE)) return;
  const double* err = b.err + (size_t)e * 3;
  const double info = b.e_info[e];
  const bool stereo = f & BA_STEREO;
  const double chi2 = stereo ? err[0] * (info * err[0]) + err[1] * (info * err[1]) + err[2] * (info * err[2])
                             : err[0] * (info * err[0]) + err[1] * (info * err[1]);
  Se3q T;
  double pc[3];
  ba_map(pr, b, S->cur, e, &T, pc);
  const bool bad = chi2 > (stereo ? 7.815 : 5.991) || !(pc[2] > 0.0);
  if (!bad) return;
  if (round == 0) { b.e_flag[e] = (uint8_t)(f | BA_LEVEL1); atomicAdd(&S->info[12], 1); }
  else { b.erase[e] = 1; atomicAdd(&S->info[13], 1); }
}

__global__ __launch_bounds__(256) void k_ba_finish(BaProblem pr, BaBuffers b) {
  const BaState* S = b.st;
  if (S->status != 0) return;
  const int t = blockIdx.x * blockDim.x + threadIdx.x, cur = S->cur;
  if (t < pr.n_points) {
    if (b.p_status[t] != SD_BA_POINT_OPTIMISED) return;
    for (int k = 0; k < 3; k++) {
      const double x = b.X[((size_t)cur * pr.n_points + t) * 3 + k];
      b.X_out[(size_t)t * 3 + k] = x;
      if (pr.wb_Tref) pr.Xw[(size_t)t * 3 + k] = x;
    }
  } else if (t < pr.n_points + pr.n_kf) {
    const int c = t - pr.n_points;
    if (b.slot[c] < 0 || !b.c_has[c]) return;   // a local keyframe that no point observes keeps its pose
    const Se3q s = ba_load_pose(b.pose + ((size_t)cur * pr.n_kf + c) * 8);
    double R[3][3], T[16];
    ba_q_to_R(s.q, R);
    for (int i = 0; i < 16; i++) T[i] = i == 15 ? 1.0 : 0.0;
    for (int r = 0; r < 3; r++) {
      for (int k = 0; k < 3; k++) T[k * 4 + r] = R[r][k];
      T[12 + r] = s.t[r];
    }
    double* wb = !pr.wb_Tref ? nullptr : c < pr.n_kf - 1 ? pr.wb_Tref + (size_t)c * 16 : pr.wb_Tcur;
    for (int i = 0; i < 16; i++) {
      b.T_out[(size_t)c * 16 + i] = T[i];
      if (wb) wb[i] = T[i];
    }
  }
}

// mode 1, once per call: bit j of row i (i < j) says that free cameras i and j see a common point, so block (i, j) of S can be
// other than 0.  Integer atomics on a bitmap k_ba_setup cleared; the bitmap does not depend on their order.
__global__ __launch_bounds__(256) void k_gba_covis(BaProblem pr, BaBuffers b) {
  if (b.st->status != 0) return;
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= pr.n_points) return;
  const int cw = (pr.kcap + 31) / 32;
  for (int e = pr.off[p]; e < pr.off[p + 1]; e++) {
    const int si = (b.e_flag[e] & BA_LIVE) ? b.slot[b.e_cam[e]] : -1;
    if (si < 0) continue;
    for (int e2 = pr.off[p]; e2 < pr.off[p + 1]; e2++) {
      const int sj = (b.e_flag[e2] & BA_LIVE) ? b.slot[b.e_cam[e2]] : -1;
      if (sj > si) atomicOr(&b.covis[(size_t)si * cw + (sj >> 5)], 1u << (sj & 31));
    }
  }
}

// ---- The blocked LDL^T of the reduced system in global memory, for more free cameras than k_ba_solve's LDS holds ----
// The same factorisation as k_ba_solve, without pivoting and in index order, on the packed lower triangle k_ba_schur writes
// (entry (r, c) at r (r + 1) / 2 + c), in panels of GBA_NB columns.  The right-hand side is row n of the triangle (k_gba_diag of
// panel 0 puts it there), so the forward substitution and the division by D are the panel and trailing steps of one more row:
// its "L" entries are y = D^-1 L^-1 b.  Per panel:
//   k_gba_diag    one workgroup: the diagonal block in LDS; L and D back in place, the unscaled columns (L D) of its rows into W
//   k_gba_panel   a lane per row below the block: the triangular solve against the block; L in place, L D into W
//   k_gba_trail   a workgroup per 32 x 32 tile of the trailing triangle: A(i, j) -= sum_k L(i, k) W(j, k), k ascending
// then, panels in descending order, k_gba_back: every workgroup solves the panel's x from the block's L^T (the same values in
// each), workgroup 0 stores it, and each lane owns one earlier entry of y and subtracts the panel's terms, k descending.
// Every entry has one owning lane and takes its terms one by one in the order the unblocked loop takes them, so L and D are
// k_ba_solve's to the bit (y is not: it forms (z_k / d_k) * (L D)(j, k) where k_ba_solve forms L(j, k) * z_k).  A zero pivot clears solve_ok in the record; every later solver kernel of the trial returns on it.
struct LdltArgs {
  BaState* st;
  double* A;    // packed lower triangle, n + 1 rows
  double* bs;   // [n] the right-hand side; the backward substitution's working vector
  double* W;    // [n + 1][GBA_NB] the current panel's L D
  double* x;    // [n]
  int n;        // >= 0: the size (sd_debug_ldlt); -1: 6 * n_slots of the record
};
static __device__ __forceinline__ size_t tri(int r, int c) { return (size_t)r * (r + 1) / 2 + c; }
static __device__ __forceinline__ int ldlt_n(const LdltArgs& a) { return a.n >= 0 ? a.n : 6 * a.st->n_slots; }

__global__ __launch_bounds__(256) void k_gba_diag(LdltArgs a, int it, int q, int panel) {
  __shared__ double s_A[GBA_NB][GBA_NB + 1], s_col[GBA_NB], s_l[GBA_NB];
  __shared__ int s_fail;
  BaState* S = a.st;
  if (!ba_trial_wanted(S, it, q)) return;
  if (panel > 0 && !S->solve_ok) return;
  const int n = ldlt_n(a), c0 = panel * GBA_NB;
  if (c0 >= n) return;
  const int w = min(GBA_NB, n - c0), t = threadIdx.x, tx = t & 15, ty = t >> 4;
  if (panel == 0)
    for (int k = t; k < n; k += 256) a.A[tri(n, k)] = a.bs[k];
  for (int e = t; e < w * w; e += 256) {
    const int r = e / w, c = e % w;
    if (c <= r) s_A[r][c] = a.A[tri(c0 + r, c0 + c)];
  }
  if (t == 0) s_fail = 0;
  __syncthreads();
  for (int k = 0; k < w; k++) {
    const double d = s_A[k][k];
    if (d == 0.0) {   // uniform
      if (t == 0) s_fail = 1;
      break;
    }
    for (int i = k + 1 + t; i < w; i += 256) {
      const double v = s_A[i][k];
      s_col[i] = v;
      s_l[i] = v / d;
    }
    __syncthreads();
    for (int i = k + 1 + t; i < w; i += 256) {
      s_A[i][k] = s_l[i];
      a.W[(size_t)(c0 + i) * GBA_NB + k] = s_col[i];
    }
    for (int i = k + 1 + ty; i < w; i += 16)
      for (int j = k + 1 + tx; j <= i; j += 16) s_A[i][j] -= s_l[i] * s_col[j];
    __syncthreads();
  }
  __syncthreads();
  const bool ok = !s_fail;
  if (ok)
    for (int e = t; e < w * w; e += 256) {
      const int r = e / w, c = e % w;
      if (c <= r) a.A[tri(c0 + r, c0 + c)] = s_A[r][c];
    }
  if (t == 0 && (panel == 0 || !ok)) S->solve_ok = ok;
}

__global__ __launch_bounds__(64) void k_gba_panel(LdltArgs a, int it, int q, int panel) {
  __shared__ double s_W11[GBA_NB][GBA_NB + 1], s_d[GBA_NB], s_row[64][GBA_NB + 1];
  const BaState* S = a.st;
  if (!ba_trial_wanted(S, it, q) || !S->solve_ok) return;
  const int n = ldlt_n(a), c0 = panel * GBA_NB;
  if (c0 >= n) return;
  const int w = min(GBA_NB, n - c0), c1 = c0 + w, t = threadIdx.x, r0 = c1 + blockIdx.x * 64;
  if (r0 > n) return;
  const int rows = min(64, n + 1 - r0);
  for (int e = t; e < w * w; e += 64) {
    const int r = e / w, c = e % w;
    if (c < r) s_W11[r][c] = a.W[(size_t)(c0 + r) * GBA_NB + c];
    else if (c == r) s_d[r] = a.A[tri(c0 + r, c0 + r)];
  }
  for (int e = t; e < rows * w; e += 64) s_row[e / w][e % w] = a.A[tri(r0 + e / w, c0 + e % w)];
  __syncthreads();
  if (t < rows) {
    const int i = r0 + t;
    for (int j = 0; j < w; j++) {
      double v = s_row[t][j];
      for (int k = 0; k < j; k++) v -= s_row[t][k] * s_W11[j][k];   // s_row[t][k], k < j, already holds L(i, k)
      const double l = v / s_d[j];
      s_row[t][j] = l;
      a.W[(size_t)i * GBA_NB + j] = v;
      if (i == n) a.bs[c0 + j] = l;   // y, where k_gba_back takes it
    }
  }
  __syncthreads();
  for (int e = t; e < rows * w; e += 64) a.A[tri(r0 + e / w, c0 + e % w)] = s_row[e / w][e % w];
}

__global__ __launch_bounds__(256) void k_gba_trail(LdltArgs a, int it, int q, int panel) {
  __shared__ double s_L[32][GBA_NB + 1], s_W[32][GBA_NB + 1];
  const BaState* S = a.st;
  if (!ba_trial_wanted(S, it, q) || !S->solve_ok) return;
  const int n = ldlt_n(a), c0 = panel * GBA_NB, c1 = c0 + GBA_NB;
  if (c1 >= n) return;   // the last panel has only row n below it, and row n has no entry right of column n - 1
  // tile (I, J), J <= I, of rows c1 .. n, columns c1 .. n - 1
  int I = (int)((sqrtf(8.f * (float)blockIdx.x + 1.f) - 1.f) * 0.5f);
  while ((I + 1) * (I + 2) / 2 <= (int)blockIdx.x) I++;
  while (I * (I + 1) / 2 > (int)blockIdx.x) I--;
  const int J = blockIdx.x - I * (I + 1) / 2, i0 = c1 + 32 * I, j0 = c1 + 32 * J;
  if (i0 > n) return;
  const int t = threadIdx.x, tx = t & 15, ty = t >> 4;
  for (int e = t; e < 32 * GBA_NB; e += 256) {
    const int r = e / GBA_NB, k = e % GBA_NB;
    s_L[r][k] = i0 + r <= n ? a.A[tri(i0 + r, c0 + k)] : 0.0;
    s_W[r][k] = j0 + r < n ? a.W[(size_t)(j0 + r) * GBA_NB + k] : 0.0;
  }
  __syncthreads();
  for (int di = 0; di < 2; di++)
    for (int dj = 0; dj < 2; dj++) {
      const int li = ty + 16 * di, lj = tx + 16 * dj, i = i0 + li, j = j0 + lj;
      if (i > n || j > i || j >= n) continue;
      double v = a.A[tri(i, j)];
      for (int k = 0; k < GBA_NB; k++) v -= s_L[li][k] * s_W[lj][k];
      a.A[tri(i, j)] = v;
    }
}

__global__ __launch_bounds__(256) void k_gba_back(LdltArgs a, int it, int q, int panel) {
  __shared__ double s_L[GBA_NB][GBA_NB + 1], s_x[GBA_NB];
  const BaState* S = a.st;
  if (!ba_trial_wanted(S, it, q) || !S->solve_ok) return;
  const int n = ldlt_n(a), c0 = panel * GBA_NB;
  if (c0 >= n) return;
  const int w = min(GBA_NB, n - c0), t = threadIdx.x;
  for (int e = t; e < w * w; e += 256) {
    const int r = e / w, c = e % w;
    if (c < r) s_L[r][c] = a.A[tri(c0 + r, c0 + c)];
  }
  if (t < w) s_x[t] = a.bs[c0 + t];
  __syncthreads();
  for (int k = w - 1; k > 0; k--) {
    if (t < k) s_x[t] -= s_L[k][t] * s_x[k];
    __syncthreads();
  }
  if (blockIdx.x == 0 && t < w) a.x[c0 + t] = s_x[t];
  const int j = blockIdx.x * 256 + t;
  if (j >= c0) return;
  double v = a.bs[j];
  for (int k = w - 1; k >= 0; k--) v -= a.A[tri(c0 + k, j)] * s_x[k];
  a.bs[j] = v;
}

// The factorisation and both substitutions of an n x n system, n known to the host: 4 launches a panel
static int launch_ldlt(const LdltArgs& a, int n, int it, int q, hipStream_t s) {
  const int np = (n + GBA_NB - 1) / GBA_NB;
  for (int p = 0; p < np; p++) {
    const int c1 = std::min(n, (p + 1) * GBA_NB), below = n + 1 - c1;
    hipLaunchKernelGGL(k_gba_diag, dim3(1), dim3(256), 0, s, a, it, q, p);
    hipLaunchKernelGGL(k_gba_panel, dim3((below + 63) / 64), dim3(64), 0, s, a, it, q, p);
    if (c1 < n) {
      const int T = (below + 31) / 32;
      hipLaunchKernelGGL(k_gba_trail, dim3(T * (T + 1) / 2), dim3(256), 0, s, a, it, q, p);
    }
    SD_HIP_CHECK(hipGetLastError());
  }
  for (int p = np - 1; p >= 0; p--) hipLaunchKernelGGL(k_gba_back, dim3(std::max(1, (p * GBA_NB + 255) / 256)), dim3(256), 0, s, a, it, q, p);
  SD_HIP_CHECK(hipGetLastError());
  return SD_OK;
}

#define BA_LAUNCH(kernel, grid, block, ...)                                    \
  do {                                                                           \
    hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), 0, s, pr, b, ##__VA_ARGS__); \
    SD_HIP_CHECK(hipGetLastError());                                             \
  } while (0)

// The whole schedule.  n_free: the cameras with role 1 as the host counts them (more than SD_BA_MAX_FREE_KF: the device refuses)
int launch_ba(const BaProblem& pr, const BaBuffers& b, int n_free, hipStream_t s) {
  const int P = pr.n_points, E = pr.n_obs, K = std::min(n_free, pr.kcap);
  const int gp = std::max(1, (P + 255) / 256), ge = std::max(1, (E + 255) / 256), gv = std::max(1, (P + pr.n_kf + 255) / 256);
  const LdltArgs la{b.st, b.S, b.bs, b.W, b.xp, -1};
  BA_LAUNCH(k_ba_gather, gp, 256);
  BA_LAUNCH(k_ba_setup, 1, 256);
  if (n_free <= pr.kcap && E > 0) {
    BA_LAUNCH(k_ba_index, 1, 1024);
    if (pr.mode) BA_LAUNCH(k_gba_covis, gp, 256);
    for (int round = 0; round < (pr.mode ? 1 : 2); round++) {
      BA_LAUNCH(k_ba_round_begin, 1, 256, round);
      for (int it = 0; it < (pr.mode ? pr.n_iterations : round ? 10 : 5); it++) {
        BA_LAUNCH(k_ba_linearise, ge, 256, it);
        BA_LAUNCH(k_ba_sum_points, std::max(1, (P + 3) / 4), 256, it);
        if (K > 0) BA_LAUNCH(k_ba_sum_cameras, K, 64, it);
        BA_LAUNCH(k_ba_iter_begin, 1, 1024, it);
        for (int q = 0; q < 10; q++) {
          if (K > 0) BA_LAUNCH(k_ba_schur, K * (K + 1) / 2, 64, it, q);
          if (K <= BA_K) BA_LAUNCH(k_ba_solve, 1, 256, it, q);   // the reduced system fits one workgroup's LDS
          else SD_TRY(launch_ldlt(la, 6 * K, it, q, s));
          BA_LAUNCH(k_ba_update, gv, 256, it, q);
          BA_LAUNCH(k_ba_errors, ge, 256, it, q);
          BA_LAUNCH(k_ba_decide, 1, 1024, it, q);
        }
      }
      if (!pr.mode) BA_LAUNCH(k_ba_classify, ge, 256, round);
    }
  }
  BA_LAUNCH(k_ba_finish, gv, 256);
  return SD_OK;
}

}  // namespace sd

using namespace sd;

// The handle's scratch holds min(SD_GBA_MAX_FREE_KF, n_kf) free cameras (and never fewer than SD_BA_MAX_FREE_KF)
static size_t ba_handle_kcap(size_t n_kf) { return std::max<size_t>(BA_K, std::min<size_t>(SD_GBA_MAX_FREE_KF, n_kf)); }

static int ba_alloc(BaBuffers& b, size_t P, size_t E, size_t n_kf) {
  uint8_t* base = nullptr;
  SD_HIP_CHECK(hipMalloc((void**)&base, ba_bytes(P, E, n_kf, ba_handle_kcap(n_kf))));
  ba_carve(b, base, P, E, n_kf, ba_handle_kcap(n_kf));
  b.base = base;
  return SD_OK;
}

// sd_track_create / sd_track_destroy (track.hip); sd_track_set_observations grows the scratch with its own block (track_refresh.hip)
int ba_create(sd_track* h) {
  h->ba.ran_points = -1;
  SD_TRY(ba_alloc(h->ba, (size_t)h->max_points, (size_t)h->max_points * 16, (size_t)h->max_batch + 1));
  SD_HIP_CHECK(hipMemset(h->ba.role, 0, (size_t)h->max_batch + 1));
  h->ba_roles.assign((size_t)h->max_batch + 1, 0);
  return SD_OK;
}
void ba_destroy(sd_track* h) {
  if (h->ba.base) (void)hipFree(h->ba.base);
  h->ba.base = nullptr;
}
int ba_grow(sd_track* h, size_t n_obs) {
  if (n_obs <= h->ba.cap_obs) return SD_OK;
  SD_HIP_CHECK(hipStreamSynchronize(h->pnp_stream));   // queued kernels may still use the old scratch
  BaBuffers nb{};
  SD_TRY(ba_alloc(nb, h->ba.cap_points, std::max(n_obs, h->ba.cap_obs * 2), (size_t)h->max_batch + 1));
  SD_HIP_CHECK(hipMemcpy(nb.role, h->ba_roles.data(), h->ba_roles.size(), hipMemcpyHostToDevice));
  (void)hipFree(h->ba.base);
  nb.ran_points = -1;   // the result of the last run went with the old scratch
  h->ba = nb;
  return SD_OK;
}

namespace {

int count_free(const uint8_t* roles, size_t n) {
  int k = 0;
  for (size_t i = 0; i < n; i++) k += roles[i] == 1;
  return k;
}

const char* const kNoBa = "sd_track_local_ba has not run (or sd_track_set_observations has replaced its scratch since)";
const char* const kNoGba = "sd_track_global_ba has not run (or sd_track_set_observations has replaced its scratch since)";

}  // namespace

extern "C" {

int sd_track_set_ba_keyframes(sd_track* h, int n_ref_frames, const uint8_t* kf_role, int cur_role) {
  SD_REQUIRE(h, SD_ERR_INVALID_ARG, "handle is NULL");
  SD_REQUIRE(n_ref_frames >= 0 && n_ref_frames <= h->max_batch, SD_ERR_CAPACITY, "n_ref_frames exceeds max_batch");
  SD_REQUIRE(n_ref_frames == 0 || kf_role, SD_ERR_INVALID_ARG, "kf_role is NULL");
  SD_REQUIRE(cur_role == 1 || cur_role == 2, SD_ERR_INVALID_ARG, "cur_role must be 1 or 2");
  for (int f = 0; f < n_ref_frames; f++) SD_REQUIRE(kf_role[f] <= 2, SD_ERR_INVALID_ARG, "kf_role must be 0, 1 or 2");
  SD_HIP_CHECK(hipSetDevice(h->device));
  std::vector<uint8_t> roles((size_t)h->max_batch + 1, 0);
  if (n_ref_frames) std::memcpy(roles.data(), kf_role, (size_t)n_ref_frames);
  roles[(size_t)h->max_batch] = (uint8_t)cur_role;
  SD_TRY(h->small_ring.upload(h->ba.role, roles.data(), roles.size(), h->pnp_stream));
  h->ba_roles = roles;
  h->ba_n_ref = n_ref_frames;
  h->ba_roles_set = true;
  return SD_OK;
}

}  // extern "C"

// sd_track_local_ba (mode 0) and sd_track_global_ba (mode 1): the checks, the problem on the resident buffers, the queued schedule
static int queue_ba(sd_track* h, int point_row, int write_back, int mode, int n_iterations, int robust) {
  SD_REQUIRE(h, SD_ERR_INVALID_ARG, "handle is NULL");
  SD_REQUIRE(!mode || (n_iterations >= 1 && n_iterations <= SD_GBA_MAX_ITERATIONS), SD_ERR_INVALID_ARG,
             "n_iterations outside [1, SD_GBA_MAX_ITERATIONS]");
  SD_REQUIRE(robust == 0 || robust == 1, SD_ERR_INVALID_ARG, "robust must be 0 or 1");
  SD_REQUIRE(h->have_cam, SD_ERR_INVALID_ARG, "sd_track_set_camera has not been called");
  SD_REQUIRE(h->rf.n_points >= 0, SD_ERR_INVALID_ARG, "sd_track_set_observations has not been called");
  SD_REQUIRE(h->ba_roles_set, SD_ERR_INVALID_ARG, "sd_track_set_ba_keyframes has not been called");
  SD_REQUIRE(point_row >= 0 && point_row < h->max_batch, SD_ERR_INVALID_ARG, "point_row outside [0, max_batch)");
  SD_REQUIRE(write_back == 0 || write_back == 1, SD_ERR_INVALID_ARG, "write_back must be 0 or 1");
  SD_REQUIRE(h->rf.max_ref_frame < 0 || (h->ref->have_geom && h->ref->last_frames > h->rf.max_ref_frame), SD_ERR_INVALID_ARG,
             "an observation names a frame of the ref extractor that has not been extracted");
  SD_REQUIRE(h->rf.max_ref_frame < 0 || keypoint_capacity(h->ref) == h->kp_cap, SD_ERR_INVALID_ARG,
             "cur / ref extractors must share the keypoint capacity");   // the mvuRight rows of both sides are kp_cap long
  const int cf = h->tb.cur_bcast >= 0 ? h->tb.cur_bcast : 0;
  SD_REQUIRE(!h->rf.has_cur || (h->cur->have_geom && h->cur->last_frames > cf), SD_ERR_INVALID_ARG,
             "an observation names the current keyframe, which has not been extracted");
  SD_REQUIRE((size_t)h->rf.n_obs <= h->ba.cap_obs && (size_t)h->rf.n_points <= h->ba.cap_points, SD_ERR_CAPACITY,
             "the observation lists exceed the bundle adjustment's scratch");
  SD_HIP_CHECK(hipSetDevice(h->device));
  if (write_back && mode) END_RESULTS(h, "sd_track_global_ba(write_back)");
  else if (write_back) END_RESULTS(h, "sd_track_local_ba(write_back)");
  h->ba.ran_points = -1;
  const RefreshBuffers& rf = h->rf;
  const TrackBuffers& tb = h->tb;
  BaProblem pr{};
  pr.off = (const int32_t*)(rf.obs + rf.o_off);
  pr.point_bad = rf.o_pbad ? rf.obs + rf.o_pbad : nullptr;
  pr.kf_bad = rf.o_kbad ? rf.obs + rf.o_kbad : nullptr;
  pr.n_points = rf.n_points;
  pr.n_obs = rf.n_obs;
  pr.n_kf = h->max_batch + 1;
  pr.frame = (const int32_t*)(rf.obs + rf.o_frame);
  pr.kp = (const int32_t*)(rf.obs + rf.o_kp);
  pr.ref_kps = keys_un(h->ref);
  pr.ref_nkp = h->ref->d_nout;
  pr.ref_ur = tb.uright_ref;
  pr.ref_cap = keypoint_capacity(h->ref);
  pr.n_ref = h->ref->have_geom ? std::min(h->max_batch, h->ref->last_frames) : 0;
  pr.cur_kps = keys_un(h->cur);
  pr.cur_nkp = h->cur->d_nout;
  pr.cur_ur = tb.uright;
  pr.cur_cap = tb.kp_cap;
  pr.cur_frame = h->cur->have_geom && h->cur->last_frames > cf ? cf : -1;
  pr.inv_sigma2 = h->d_inv_sigma2;
  pr.nlevels = h->cur->nlevels;
  pr.Tref = tb.Tref;
  pr.Tcur = tb.Tcur;
  pr.Xw = tb.lm_Xw + (size_t)point_row * tb.max_points * 3;
  if (write_back) { pr.wb_Tref = tb.Tref; pr.wb_Tcur = tb.Tcur; }
  pr.fx = h->cam.fx; pr.fy = h->cam.fy; pr.cx = h->cam.cx; pr.cy = h->cam.cy; pr.bf = h->cam.bf;
  ba_set_mode(pr, mode, n_iterations, robust, mode ? h->ba.kcap : BA_K);
  const int n_free = count_free(h->ba_roles.data(), h->ba_roles.size());
  SD_TRY(run_stage(h, true, false, STAGE_NONE, [&](hipStream_t s) { return launch_ba(pr, h->ba, n_free, s); }));
  h->ba.ran_points = rf.n_points;
  h->ba.ran_obs = rf.n_obs;
  h->ba.ran_global = mode;
  h->ba_serial = rf.serial;
  return SD_OK;
}

// What both getters download; obs_erase NULL: not wanted
static int get_ba(sd_track* h, int mode, double* T_ref_cm16, double* T_cur_cm16, double* Xw, uint8_t* point_status, uint8_t* obs_erase,
                  int32_t* info16, int cap_points, int cap_obs) {
  TRACK_RANGE(h, 0, 1);
  SD_REQUIRE(h->ba.ran_points >= 0 && h->ba.ran_global == mode, SD_ERR_INVALID_ARG, mode ? kNoGba : kNoBa);
  const size_t P = (size_t)h->ba.ran_points, E = (size_t)h->ba.ran_obs;
  SD_REQUIRE(!(Xw || point_status) || (cap_points >= 0 && (size_t)cap_points >= P), SD_ERR_CAPACITY, "cap_points smaller than the number of points");
  SD_REQUIRE(!obs_erase || (cap_obs >= 0 && (size_t)cap_obs >= E), SD_ERR_CAPACITY, "cap_obs smaller than the number of observations");
  hipStream_t s = h->cur->stream;
  const BaBuffers& b = h->ba;
  if (h->ba_n_ref) SD_TRY(download(T_ref_cm16, b.T_out, 0, (size_t)h->ba_n_ref, 16, s));
  SD_TRY(download(T_cur_cm16, b.T_out, (size_t)h->max_batch, 1, 16, s));
  if (P) SD_TRY(download(Xw, b.X_out, 0, P, 3, s));
  if (P) SD_TRY(download(point_status, b.p_status, 0, P, 1, s));
  if (E) SD_TRY(download(obs_erase, b.erase, 0, E, 1, s));
  SD_TRY(download(info16, b.st->info, 0, 16, 1, s));
  return wait_for(s);
}

extern "C" {

int sd_track_local_ba(sd_track* h, int point_row, int write_back) { return queue_ba(h, point_row, write_back, 0, 0, 1); }

int sd_track_global_ba(sd_track* h, int point_row, int n_iterations, int robust, int write_back) {
  return queue_ba(h, point_row, write_back, 1, n_iterations, robust);
}

int sd_track_get_global_ba(sd_track* h, double* T_ref_cm16, double* T_cur_cm16, double* Xw, uint8_t* point_status, int32_t* info16,
                           int cap_points) {
  return get_ba(h, 1, T_ref_cm16, T_cur_cm16, Xw, point_status, nullptr, info16, cap_points, 0);
}

int sd_track_get_local_ba(sd_track* h, double* T_ref_cm16, double* T_cur_cm16, double* Xw, uint8_t* point_status, uint8_t* obs_erase,
                          int32_t* info16, int cap_points, int cap_obs) {
  return get_ba(h, 0, T_ref_cm16, T_cur_cm16, Xw, point_status, obs_erase, info16, cap_points, cap_obs);
}

}  // extern "C"

// sd_debug_local_ba (mode 0) and sd_debug_global_ba (mode 1, obs_erase NULL)
static int debug_ba(const char* name, int mode, int n_iterations, int robust, int n_points, const int32_t* obs_off, const int32_t* obs_kf,
                    const float* obs_uv, const float* obs_ur, const float* obs_inv_sigma2, const uint8_t* obs_kf_bad,
                    const uint8_t* point_bad, int n_kf, const double* T_cm16, const uint8_t* kf_role, const double* Xw, const float* cam9,
                    double* T_out_cm16, double* Xw_out, uint8_t* point_status, uint8_t* obs_erase, int32_t* info16) {
  SD_REQUIRE(!mode || (n_iterations >= 1 && n_iterations <= SD_GBA_MAX_ITERATIONS), SD_ERR_INVALID_ARG,
             "n_iterations outside [1, SD_GBA_MAX_ITERATIONS]");
  SD_REQUIRE(robust == 0 || robust == 1, SD_ERR_INVALID_ARG, "robust must be 0 or 1");
  SD_REQUIRE(n_points >= 0 && obs_off && obs_off[0] == 0, SD_ERR_INVALID_ARG, "NULL list, negative n_points or obs_off[0] != 0");
  for (int i = 0; i < n_points; i++) SD_REQUIRE(obs_off[i + 1] >= obs_off[i], SD_ERR_INVALID_ARG, "obs_off is not monotone");
  const int total = obs_off[n_points];
  SD_REQUIRE(n_points <= (1 << 20) && total <= (1 << 22) && n_kf >= 1 && n_kf <= (1 << 16), SD_ERR_CAPACITY,
             "at most 2^20 points, 2^22 observations and 2^16 keyframes");
  SD_REQUIRE((total == 0 || (obs_kf && obs_uv && obs_ur && obs_inv_sigma2)) && T_cm16 && kf_role && (n_points == 0 || Xw) && cam9 &&
                 T_out_cm16 && (n_points == 0 || (Xw_out && point_status)) && (total == 0 || mode || obs_erase) && info16,
             SD_ERR_INVALID_ARG, "NULL array");
  for (int c = 0; c < n_kf; c++) SD_REQUIRE(kf_role[c] <= 2, SD_ERR_INVALID_ARG, "kf_role must be 0, 1 or 2");
  const size_t P = (size_t)n_points, E = (size_t)total, Kn = (size_t)n_kf;
  const int n_free = count_free(kf_role, Kn);
  const size_t kcap = mode ? (size_t)std::min(std::max(n_free, BA_K), SD_GBA_MAX_FREE_KF) : (size_t)BA_K;
  Blob blob;
  const size_t o_off = blob.reserve(P + 1, obs_off, P + 1), o_kf = blob.reserve(E + 1, obs_kf, E), o_uv = blob.reserve(2 * E + 2, obs_uv, 2 * E);
  const size_t o_ur = blob.reserve(E + 1, obs_ur, E), o_inv = blob.reserve(E + 1, obs_inv_sigma2, E);
  const size_t o_kb = blob.reserve(E + 1, obs_kf_bad, obs_kf_bad ? E : 0), o_pb = blob.reserve(P + 1, point_bad, point_bad ? P : 0);
  const size_t o_T = blob.reserve(Kn * 16, T_cm16, Kn * 16), o_X = blob.reserve(P * 3 + 3, Xw, P * 3);
  const size_t o_scratch = blob.reserve(ba_bytes(P, E, Kn, kcap), (const uint8_t*)nullptr, 0);
  BaBuffers b{};
  SD_TRY(blob.run(name, [&] {
    ba_carve(b, blob.dev<uint8_t>(o_scratch), P, E, Kn, kcap);
    if (hipError_t e = hipMemcpy(b.role, kf_role, Kn, hipMemcpyHostToDevice); e != hipSuccess) return hip_error(name, e);
    BaProblem pr{};
    pr.off = blob.dev<int32_t>(o_off);
    pr.point_bad = point_bad ? blob.dev<uint8_t>(o_pb) : nullptr;
    pr.kf_bad = obs_kf_bad ? blob.dev<uint8_t>(o_kb) : nullptr;
    pr.n_points = n_points; pr.n_obs = total; pr.n_kf = n_kf;
    pr.d_kf = blob.dev<int32_t>(o_kf); pr.d_uv = blob.dev<float>(o_uv); pr.d_ur = blob.dev<float>(o_ur); pr.d_inv = blob.dev<float>(o_inv);
    pr.d_T = blob.dev<double>(o_T);
    pr.Xw = blob.dev<double>(o_X);
    const TrackCam cam = make_cam(cam9[0], cam9[1], cam9[2], cam9[3], cam9[4], cam9[5], cam9[6], cam9[7], cam9[8]);
    pr.fx = cam.fx; pr.fy = cam.fy; pr.cx = cam.cx; pr.cy = cam.cy; pr.bf = cam.bf;
    ba_set_mode(pr, mode, n_iterations, robust, (int)kcap);
    SD_TRY(launch_ba(pr, b, n_free, 0));
    SD_HIP_CHECK(hipDeviceSynchronize());
    return SD_OK;
  }));
  // the scratch came back with the rest of the blob: its addresses are offsets into the mirror
  auto host = [&](const void* dev_ptr) { return o_scratch + (size_t)((const uint8_t*)dev_ptr - (const uint8_t*)b.st); };
  blob.take(T_out_cm16, host(b.T_out), Kn * 16 * 8);
  blob.take(Xw_out, host(b.X_out), P * 24);
  blob.take(point_status, host(b.p_status), P);
  if (obs_erase) blob.take(obs_erase, host(b.erase), E);
  blob.take(info16, host(b.st) + offsetof(BaState, info), 64);
  return SD_OK;
}

extern "C" {

int sd_debug_local_ba(int n_points, const int32_t* obs_off, const int32_t* obs_kf, const float* obs_uv, const float* obs_ur,
                      const float* obs_inv_sigma2, const uint8_t* obs_kf_bad, const uint8_t* point_bad, int n_kf, const double* T_cm16,
                      const uint8_t* kf_role, const double* Xw, const float* cam9, double* T_out_cm16, double* Xw_out,
                      uint8_t* point_status, uint8_t* obs_erase, int32_t* info16) {
  return debug_ba("sd_debug_local_ba", 0, 0, 1, n_points, obs_off, obs_kf, obs_uv, obs_ur, obs_inv_sigma2, obs_kf_bad, point_bad, n_kf, T_cm16,
                  kf_role, Xw, cam9, T_out_cm16, Xw_out, point_status, obs_erase, info16);
}

int sd_debug_global_ba(int n_points, const int32_t* obs_off, const int32_t* obs_kf, const float* obs_uv, const float* obs_ur,
                       const float* obs_inv_sigma2, const uint8_t* obs_kf_bad, const uint8_t* point_bad, int n_kf, const double* T_cm16,
                       const uint8_t* kf_role, const double* Xw, const float* cam9, int n_iterations, int robust, double* T_out_cm16,
                       double* Xw_out, uint8_t* point_status, int32_t* info16) {
  return debug_ba("sd_debug_global_ba", 1, n_iterations, robust, n_points, obs_off, obs_kf, obs_uv, obs_ur, obs_inv_sigma2, obs_kf_bad,
                  point_bad, n_kf, T_cm16, kf_role, Xw, cam9, T_out_cm16, Xw_out, point_status, nullptr, info16);
}

int sd_debug_ldlt(int n, const double* A_packed_lower, const double* b, double* x, int32_t* ok) {
  SD_REQUIRE(n >= 1 && n <= 6 * SD_GBA_MAX_FREE_KF, SD_ERR_INVALID_ARG, "n outside [1, 6 * SD_GBA_MAX_FREE_KF]");
  SD_REQUIRE(A_packed_lower && b && x && ok, SD_ERR_INVALID_ARG, "NULL array");
  const size_t N = (size_t)n;
  BaState st{};   // a record that wants (iteration 0, trial 0)
  st.round_live = 1;
  st.trial_live = 1;
  Blob blob;
  const size_t o_st = blob.reserve(1, &st, 1), o_A = blob.reserve((N + 1) * (N + 2) / 2, A_packed_lower, N * (N + 1) / 2);
  const size_t o_b = blob.reserve(N, b, N), o_W = blob.reserve((N + 1) * GBA_NB, (const double*)nullptr, 0);
  const size_t o_x = blob.reserve(N, (const double*)nullptr, 0);
  SD_TRY(blob.run("sd_debug_ldlt", [&] {
    const LdltArgs la{blob.dev<BaState>(o_st), blob.dev<double>(o_A), blob.dev<double>(o_b), blob.dev<double>(o_W), blob.dev<double>(o_x), n};
    SD_TRY(launch_ldlt(la, n, 0, 0, 0));
    SD_HIP_CHECK(hipDeviceSynchronize());
    return SD_OK;
  }));
  blob.take(&st, o_st, sizeof st);
  *ok = st.solve_ok;
  blob.take(x, o_x, N * 8);   // never written after a zero pivot: the zeros it was uploaded with
  return SD_OK;
}

}  // extern "C"
