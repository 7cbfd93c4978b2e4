// ORBmatcher::SearchForTriangulation(KeyFrame* pKF1, KeyFrame* pKF2, F12, vMatchedPairs) and LocalMapping::ComputeF12 on
// MI355X (reference src/ORBmatcher.cc:359-475, :128-144; src/LocalMapping.cc:494-511; caller LocalMapping::CreateNewMapPoints):
// the epipolar brute-force matcher that finds the pairs a new keyframe triangulates against each of its neighbours.
//
// Slot f pairs frame f (or the broadcast frame) of the `cur` extractor -- KF1, pose Tcur -- with frame f of the `ref`
// extractor -- KF2, pose Tref -- as k_search_points does.  Two kernels:
//
//   k_tri_geometry, one lane per slot, double throughout, every product and sum rounded on its own (the library is built
//   with -ffp-contract=off).  With R1w, t1w from Tcur and R2w, t2w from Tref, every 3 x 3 product entry is
//   (x0 * y0 + x1 * y1) + x2 * y2, k = 0..2 in order, and matrix chains go left to right:
//     R12 = R1w * R2w^T;   t12[r] = (((-R12[r][0]) * t2w[0] + (-R12[r][1]) * t2w[1]) + (-R12[r][2]) * t2w[2]) + t1w[r]
//     inverse of a 3 x 3 M by cofactors: C[i][j] = M[i+1][j+1] * M[i+2][j+2] - M[i+1][j+2] * M[i+2][j+1] (indices mod 3),
//       det = (M[0][0] * C[0][0] + M[0][1] * C[0][1]) + M[0][2] * C[0][2], inv[i][j] = C[j][i] * (1.0 / det)
//     F12 = ((inv(K^T) * [t12]x) * R12) * inv(K),  K = the tracker's camera (both keyframes share it)
//   and the epipole (:362-368): Cw = -(R1w^T * t1w), C2 = R2w * Cw + t2w, invz = (float)(1.0 / C2z),
//     ex = (float)((fx * C2x) * invz + cx), ey likewise.
//
//   k_search_triangulation, one workgroup per slot.  This variant of the matcher never sets vbMatched2, so every idx1 row is
//   independent and the scaffold of track_bf_dev.h does the scan: a lane's BF_PT rows carry the descriptor, the epipolar line
//   a, b, c, den and the stereo bit in registers, a KF2 tile carries x, y and the gate threshold beside the descriptor, and
//   the eligibility mask is idx2 < N2, no map point.  Every gate of the reference is
//   a pure filter and `dist > bestDist -> continue` keeps the smallest distance, the LARGEST idx2 among equals, so a row's
//   result is min over the passing candidates of dist << 11 | (2047 - idx2).
//   What depends on the KF2 keypoint alone is evaluated once per keypoint instead of once per pair, in the reference's
//   arithmetic: the epipole gate (ex - x2)^2 + (ey - y2)^2 < 100 * mvScaleFactors[octave2] becomes a second bit mask (set:
//   keypoint is mono and inside the radius; it rejects the pair when the row is mono too), and the threshold of
//   (double)dsqr < 3.84 * (double)mvLevelSigma2[octave2] becomes the float thr = 3.84 * sigma2 rounded UP: for a float dsqr,
//   dsqr < thr holds exactly when (double)dsqr < the double product does.  den == 0 makes dsqr inf or NaN, which fails the
//   comparison as the reference's explicit test does; the row is also dropped explicitly at the end.
//   Gate order: the epipolar test first, for the wave's 128 rows; the tile's descriptor is read and the popcounts run only
//   when one of them passes.  The gate passes so few candidates that this beats computing both and selecting, although a wave
//   skips only when all of its rows reject (measured: DESIGN.md section 6, SearchForTriangulation).
//   Rotation check (:434-463): the bin arithmetic is that of SearchByPoints (:1269-1278, rot_bin) and the cut is the same
//   ComputeThreeMaxima: bf_rotation_cut (track_bf_dev.h) serves both matchers.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <string>
#include <vector>

#include "track_bf_dev.h"
#include "track_handle.h"

namespace sd {

// What the matcher reads and writes besides the two keyframes' keypoints: rows of `cap` entries per slot
struct TriBuffers {
  const uint8_t* has1;   // [B][cap] KF1 keypoint holds a map point (slot row)
  const uint8_t* has2;   // [B][cap] the same for KF2
  const float* ur1;      // [.][cap] KF1 mvuRight (row of the cur FRAME)
  const float* ur2;      // [B][cap] KF2 mvuRight
  const double* F12;     // [B][9] row-major
  const float* epi;      // [B][2]
  const float* sf;       // [nlevels] mvScaleFactors
  const float* sigma2;   // [nlevels] mvLevelSigma2
  int32_t* match;        // [B][cap] KF2 index or -1
  int32_t* n;            // [B]
};

// out = A * B, row-major 3 x 3
__device__ __forceinline__ void mul33(const double* A, const double* B, double* out) {
  for (int r = 0; r < 3; r++)
    for (int c = 0; c < 3; c++) out[r * 3 + c] = dot3(A[r * 3], A[r * 3 + 1], A[r * 3 + 2], B[c], B[3 + c], B[6 + c]);
}
__device__ __forceinline__ void inv33(const double* M, double* out) {
  double C[9];
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) {
      const int i1 = (i + 1) % 3, i2 = (i + 2) % 3, j1 = (j + 1) % 3, j2 = (j + 2) % 3;
      C[i * 3 + j] = __dsub_rn(__dmul_rn(M[i1 * 3 + j1], M[i2 * 3 + j2]), __dmul_rn(M[i1 * 3 + j2], M[i2 * 3 + j1]));
    }
  const double invdet = __ddiv_rn(1.0, dot3(M[0], M[1], M[2], C[0], C[1], C[2]));
  for (int i = 0; i < 3; i++)
    for (int j = 0; j < 3; j++) out[i * 3 + j] = __dmul_rn(C[j * 3 + i], invdet);
}

__global__ __launch_bounds__(64) void k_tri_geometry(const double* __restrict__ Tcur, const double* __restrict__ Tref, TrackCam cam,
                                                     const double* __restrict__ F12_set /* NULL: ComputeF12 */, double* __restrict__ F12_out,
                                                     float* __restrict__ epi_out, int n_frames) {
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= n_frames) return;
  const double *T1 = Tcur + (size_t)f * 16, *T2 = Tref + (size_t)f * 16;   // column-major: R[r][c] = T[c * 4 + r]
  double R1[9], R2[9], t1[3], t2[3];
  for (int r = 0; r < 3; r++) {
    for (int c = 0; c < 3; c++) {
      R1[r * 3 + c] = T1[c * 4 + r];
      R2[r * 3 + c] = T2[c * 4 + r];
    }
    t1[r] = T1[12 + r];
    t2[r] = T2[12 + r];
  }
  double* F = F12_out + (size_t)f * 9;
  if (F12_set) {
    for (int i = 0; i < 9; i++) F[i] = F12_set[(size_t)f * 9 + i];
  } else {
    double R12[9], t12[3];
    for (int r = 0; r < 3; r++)
      for (int c = 0; c < 3; c++) R12[r * 3 + c] = dot3(R1[r * 3], R1[r * 3 + 1], R1[r * 3 + 2], R2[c * 3], R2[c * 3 + 1], R2[c * 3 + 2]);
    for (int r = 0; r < 3; r++) t12[r] = __dadd_rn(dot3(-R12[r * 3], -R12[r * 3 + 1], -R12[r * 3 + 2], t2[0], t2[1], t2[2]), t1[r]);
    const double tx[9] = {0.0, -t12[2], t12[1], t12[2], 0.0, -t12[0], -t12[1], t12[0], 0.0};
    const double K[9] = {cam.fx, 0.0, cam.cx, 0.0, cam.fy, cam.cy, 0.0, 0.0, 1.0};
    const double Kt[9] = {cam.fx, 0.0, 0.0, 0.0, cam.fy, 0.0, cam.cx, cam.cy, 1.0};
    double Kti[9], Ki[9], A[9], Bm[9];
    inv33(Kt, Kti);
    inv33(K, Ki);
    mul33(Kti, tx, A);
    mul33(A, R12, Bm);
    mul33(Bm, Ki, F);
  }
  double Cw[3], C2[3];
  for (int r = 0; r < 3; r++) Cw[r] = -dot3(R1[r], R1[3 + r], R1[6 + r], t1[0], t1[1], t1[2]);
  for (int r = 0; r < 3; r++) C2[r] = __dadd_rn(dot3(R2[r * 3], R2[r * 3 + 1], R2[r * 3 + 2], Cw[0], Cw[1], Cw[2]), t2[r]);
  const float invz = (float)__ddiv_rn(1.0, C2[2]);
  epi_out[(size_t)f * 2] = (float)__dadd_rn(__dmul_rn(__dmul_rn(cam.fx, C2[0]), (double)invz), cam.cx);
  epi_out[(size_t)f * 2 + 1] = (float)__dadd_rn(__dmul_rn(__dmul_rn(cam.fy, C2[1]), (double)invz), cam.cy);
}

// Dynamic LDS: LdsSearchTri (track_match_lds.h)
__global__ __launch_bounds__(BF_THREADS) void k_search_triangulation(const sd_keypoint* __restrict__ kps1_all, const uint8_t* __restrict__ desc1_all,
                                                                     const int32_t* __restrict__ n1_all, const sd_keypoint* __restrict__ kps2_all,
                                                                     const uint8_t* __restrict__ desc2_all, const int32_t* __restrict__ n2_all,
                                                                     TriBuffers tb, int cur_bcast, int cap, int capw /* cap rounded up to 64 */,
                                                                     int nlevels, int check_ori) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const LdsSearchTri L(capw);
  uint32_t* s_tile = lds_at<uint32_t>(smem, L.tile);
  float4* s_aux = lds_at<float4>(smem, L.aux);
  uint16_t* s_i1 = lds_at<uint16_t>(smem, L.i1);
  int16_t* s_match = lds_at<int16_t>(smem, L.match);
  uint32_t* s_elig = lds_at<uint32_t>(smem, L.elig);
  uint32_t* s_erej = lds_at<uint32_t>(smem, L.erej);
  int* s_hist = lds_at<int>(smem, L.hist);
  int* s_n1v = lds_at<int>(smem, L.n1v);
  const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const BfSlot S(kps1_all, desc1_all, n1_all, kps2_all, desc2_all, n2_all, f, cur_bcast, cap);
  const int N2 = S.N2;
  const uint8_t* has1 = tb.has1 + (size_t)f * cap;
  const uint8_t* has2 = tb.has2 + (size_t)f * cap;
  const float* ur1 = tb.ur1 + (size_t)S.fc * cap;
  const float* ur2 = tb.ur2 + (size_t)f * cap;
  const double* F = tb.F12 + (size_t)f * 9;
  const float ex = tb.epi[(size_t)f * 2], ey = tb.epi[(size_t)f * 2 + 1];

  // ---- KF2 as bits: eligible (idx2 < N2, no map point); mono and inside the epipole's radius (:418-423)
  const auto eligible = [&](int i) { return i < N2 && has2[i] == 0; };
  pack_flags(eligible, capw, s_elig, tid, BF_THREADS);
  pack_flags([&](int i) {
    if (i >= N2) return false;
    const bool el = has2[i] == 0, mono = !(ur2[i] >= 0);   // three independent loads, not a chain: few slots leave the latency bare
    const sd_keypoint kp = S.kps2[i];
    const float distex = ex - kp.x, distey = ey - kp.y;
    return el && mono && distex * distex + distey * distey < 100.0f * tb.sf[min(max(kp.octave, 0), nlevels - 1)];
  }, capw, s_erej, tid, BF_THREADS);
  for (int i = tid; i < capw; i += BF_THREADS) s_match[i] = -1;
  if (tid < 32) s_hist[tid] = 0;
  // ---- the KF1 rows without a map point, ascending
  if (wave == 0) bf_compact_rows([&](int i) { return i < S.N1 && has1[i] == 0; }, capw, s_i1, s_n1v, lane);
  __syncthreads();
  const int n1v = *s_n1v;
  const int ntiles = (N2 + BF_TILE - 1) / BF_TILE;

  for (int e0 = 0; e0 < n1v; e0 += BF_THREADS * BF_PT) {
    uint32_t d1[BF_PT][8], best[BF_PT];
    float la[BF_PT], lb[BF_PT], lc[BF_PT], den[BF_PT];
    bool mono1[BF_PT];
    int ent[BF_PT];
#pragma unroll
    for (int p = 0; p < BF_PT; p++) {
      ent[p] = e0 + p * BF_THREADS + tid;
      const int i1 = ent[p] < n1v ? s_i1[ent[p]] : s_i1[0];   // n1v >= 1 here: entry 0 exists
      load_desc8(S.desc1, i1, d1[p]);
      // l = x1' F12 = [a b c] (:130-132): double, left to right, rounded to float once
      const double x1 = (double)S.kps1[i1].x, y1 = (double)S.kps1[i1].y;
      la[p] = (float)__dadd_rn(__dadd_rn(__dmul_rn(x1, F[0]), __dmul_rn(y1, F[3])), F[6]);
      lb[p] = (float)__dadd_rn(__dadd_rn(__dmul_rn(x1, F[1]), __dmul_rn(y1, F[4])), F[7]);
      lc[p] = (float)__dadd_rn(__dadd_rn(__dmul_rn(x1, F[2]), __dmul_rn(y1, F[5])), F[8]);
      den[p] = __fadd_rn(__fmul_rn(la[p], la[p]), __fmul_rn(lb[p], lb[p]));
      mono1[p] = !(ur1[i1] >= 0);
      best[p] = BF_NONE;
    }
    for (int t = 0; t < ntiles; t++) {
      const int j0 = t * BF_TILE, jn = min(BF_TILE, N2 - j0);
      bf_stage_tile(S.desc2, j0, jn, s_tile, tid, [&] {
        for (int j = tid; j < jn; j += BF_THREADS) {
          const sd_keypoint kp = S.kps2[j0 + j];
          const double thr = __dmul_rn(3.84, (double)tb.sigma2[min(max(kp.octave, 0), nlevels - 1)]);
          s_aux[j] = make_float4(kp.x, kp.y, __double2float_ru(thr), 0.f);
        }
      });
      for (int wd = 0; wd < (jn + 31) >> 5; wd++) {
        const uint32_t rej = (uint32_t)__builtin_amdgcn_readfirstlane((int)s_erej[(j0 >> 5) + wd]);
        for_each_set_bit(s_elig[(j0 >> 5) + wd], [&](int bit) {
          const int jl = wd * 32 + bit;
          const float4 q = s_aux[jl];                                                                       // LDS broadcasts
          const bool mono_rej = (rej >> bit) & 1u;
          bool pass[BF_PT];
#pragma unroll
          for (int p = 0; p < BF_PT; p++) {
            // CheckDistEpipolarLine (:134-143), all float
            const float num = __fadd_rn(__fadd_rn(__fmul_rn(la[p], q.x), __fmul_rn(lb[p], q.y)), lc[p]);
            const float dsqr = __fdiv_rn(__fmul_rn(num, num), den[p]);
            pass[p] = dsqr < q.z && !(mono_rej && mono1[p]);
          }
          bool any = false;
#pragma unroll
          for (int p = 0; p < BF_PT; p++) any |= pass[p];
          if (!__ballot(any)) return;   // wave-uniform: no row of this wave takes the candidate
          uint32_t d2[8];
          load_desc8(s_tile, jl, d2);
          const uint32_t low = (uint32_t)(2047 - (j0 + jl));
#pragma unroll
          for (int p = 0; p < BF_PT; p++) {
            const int dist = hamming256(d1[p], d2);
            const uint32_t key = ((uint32_t)dist << 11) | low;
            best[p] = pass[p] && dist <= BF_TH_LOW ? min(best[p], key) : best[p];   // a select, not a branch
          }
        });
      }
    }
#pragma unroll
    for (int p = 0; p < BF_PT; p++)
      if (ent[p] < n1v && best[p] != BF_NONE && den[p] != 0.f) s_match[s_i1[ent[p]]] = (int16_t)(2047 - (int)(best[p] & 2047u));
  }
  __syncthreads();
  if (tid >= 64) return;   // one wavefront counts and runs the rotation check

  int nmatches = 0;
  for (int e0 = 0; e0 < n1v; e0 += 64) nmatches += __popcll(__ballot(e0 + lane < n1v && s_match[s_i1[e0 + lane]] >= 0));
  if (check_ori) nmatches -= bf_rotation_cut(S, s_i1, n1v, s_match, s_hist, lane);
  bf_write_out(s_match, cap, nmatches, tb.match + (size_t)f * cap, tb.n + f, lane);
}

static int launch_search_triangulation(const sd_keypoint* kps1, const uint8_t* desc1, const int32_t* n1, const sd_keypoint* kps2,
                                       const uint8_t* desc2, const int32_t* n2, const TriBuffers& tb, int cur_bcast, int cap, int nlevels,
                                       int n_frames, int check_ori, hipStream_t s) {
  const int capw = (cap + 63) & ~63;
  SD_REQUIRE(capw <= 2048, SD_ERR_CAPACITY, "SearchForTriangulation supports at most 2048 keypoints per keyframe");
  hipLaunchKernelGGL(k_search_triangulation, dim3(n_frames), dim3(BF_THREADS), LdsSearchTri(capw).bytes, s, kps1, desc1, n1, kps2, desc2, n2,
                     tb, cur_bcast, cap, capw, nlevels, check_ori != 0);
  SD_HIP_CHECK(hipGetLastError());
  return SD_OK;
}

int launch_tri(const sd_orb* cur, const sd_orb* ref, const TrackBuffers& b, const TrackCam& cam, const float* d_sf, const float* d_sigma2,
               int n_frames, int use_set_f12, int check_ori, hipStream_t s) {
  hipLaunchKernelGGL(k_tri_geometry, dim3((n_frames + 63) / 64), dim3(64), 0, s, b.Tcur, b.Tref, cam,
                     use_set_f12 ? (const double*)b.tri_F12_set : (const double*)nullptr, b.tri_F12, b.tri_epi, n_frames);
  SD_HIP_CHECK(hipGetLastError());
  const TriBuffers tb = {b.sp_valid1, b.sp_valid2, b.uright, b.uright_ref, b.tri_F12, b.tri_epi, d_sf, d_sigma2, b.tri_match, b.tri_n};
  return launch_search_triangulation(keys_un(cur), cur->d_desc, cur->d_nout, keys_un(ref), ref->d_desc, ref->d_nout, tb, b.cur_bcast,
                                     b.kp_cap, cur->nlevels, n_frames, check_ori, s);
}

}  // namespace sd

using namespace sd;

extern "C" {

int sd_track_set_uright_ref(sd_track* h, int frame0, int n_frames, const float* uright, int cap) {
  QUEUE_RANGE(h, frame0, n_frames);
  SD_REQUIRE(uright && cap >= 1 && cap <= h->kp_cap, SD_ERR_INVALID_ARG, "bad uright array");
  END_RESULTS(h, "sd_track_set_uright_ref");
  SD_TRY(upload_rows(h->tb.uright_ref, h->kp_cap, uright, cap, frame0, n_frames, h->pnp_stream));
  return wait_for(h->pnp_stream);   // the rows are the caller's pageable memory: back once they are read
}

int sd_track_set_f12(sd_track* h, int frame0, int n_frames, const double* F12_rm9) {
  QUEUE_RANGE(h, frame0, n_frames);
  SD_REQUIRE(F12_rm9, SD_ERR_INVALID_ARG, "NULL argument");
  END_RESULTS(h, "sd_track_set_f12");
  SD_TRY(h->pose_ring.upload(h->tb.tri_F12_set + (size_t)frame0 * 9, F12_rm9, (size_t)n_frames * 9, h->pnp_stream));
  std::fill(h->f12_set.begin() + frame0, h->f12_set.begin() + frame0 + n_frames, (uint8_t)1);
  return SD_OK;
}

int sd_track_search_for_triangulation(sd_track* h, int n_frames, int use_set_f12, int check_ori) {
  SD_TRY(check_ready(h, n_frames));
  SD_TRY(require_ref_frames(h, n_frames, false, true));
  if (use_set_f12)
    for (int f = 0; f < n_frames; f++)
      SD_REQUIRE(h->f12_set[f], SD_ERR_INVALID_ARG, "use_set_f12 = 1, but sd_track_set_f12 has not covered these slots");
  END_RESULTS(h, "sd_track_search_for_triangulation");
  SD_TRY(run_stage(h, true, false, STAGE_MATCH, [&](hipStream_t s) {   // timed in the matcher's slot
    return launch_tri(h->cur, h->ref, h->tb, h->cam, h->d_sf, h->d_sigma2, n_frames, use_set_f12, check_ori, s);
  }));
  h->res.tri.set(n_frames, BIND_TRI, inputs_now(h), check_ori != 0);   // payload: the rotation check ran (sd_track_triangulate asks)
  return SD_OK;
}

int sd_track_get_triangulation_matches(sd_track* h, int frame0, int n_frames, int32_t* matches12, int cap, int32_t* n_matches,
                                       double* F12_rm9, float* epipole2) {
  TRACK_RANGE(h, frame0, n_frames);
  SD_REQUIRE(h->res.tri.live(frame0 + n_frames, inputs_now(h)), SD_ERR_INVALID_ARG,
             "sd_track_search_for_triangulation has not run on these slots (or their keyframes, flags, mvuRight, poses, F12 or the "
             "broadcast setting were replaced since)");
  SD_REQUIRE(!matches12 || cap >= h->kp_cap, SD_ERR_CAPACITY, "cap smaller than the keypoint capacity");
  hipStream_t s = h->cur->stream;
  SD_TRY(download_rows(matches12, cap, h->tb.tri_match, frame0, n_frames, h->kp_cap, s));
  SD_TRY(download(n_matches, h->tb.tri_n, frame0, n_frames, 1, s));
  SD_TRY(download(F12_rm9, h->tb.tri_F12, frame0, n_frames, 9, s));
  SD_TRY(download(epipole2, h->tb.tri_epi, frame0, n_frames, 2, s));
  return wait_for(s);
}

int sd_debug_search_for_triangulation(int n1, int n2, const sd_keypoint* kps1, const uint8_t* desc1, const uint8_t* has_mp1,
                                      const float* uright1, const sd_keypoint* kps2, const uint8_t* desc2, const uint8_t* has_mp2,
                                      const float* uright2, const double* F12_rm9, const float* epipole2, const float* scale_factors,
                                      const float* level_sigma2, int nlevels, int check_ori, int32_t* matches12, int32_t* n_matches) {
  SD_REQUIRE(n1 >= 0 && n2 >= 0 && n1 <= 2048 && n2 <= 2048, SD_ERR_CAPACITY, "at most 2048 keypoints per keyframe");
  SD_REQUIRE((n1 == 0 || (kps1 && desc1 && has_mp1 && uright1 && matches12)) && (n2 == 0 || (kps2 && desc2 && has_mp2 && uright2)),
             SD_ERR_INVALID_ARG, "NULL keyframe array");
  SD_REQUIRE(F12_rm9 && epipole2 && scale_factors && level_sigma2 && nlevels >= 1 && nlevels <= SD_MAX_LEVELS && n_matches,
             SD_ERR_INVALID_ARG, "bad arguments");
  const size_t cap = (size_t)std::max(std::max(n1, n2), 1);
  Blob b;
  const int32_t counts[3] = {n1, n2, 0};
  const size_t o_k1 = b.reserve(cap, kps1, n1), o_k2 = b.reserve(cap, kps2, n2);
  const size_t o_d1 = b.reserve(cap * 32, desc1, (size_t)n1 * 32), o_d2 = b.reserve(cap * 32, desc2, (size_t)n2 * 32);
  const size_t o_h1 = b.reserve(cap, has_mp1, n1), o_h2 = b.reserve(cap, has_mp2, n2);
  const size_t o_u1 = b.reserve(cap, uright1, n1), o_u2 = b.reserve(cap, uright2, n2);
  const size_t o_F = b.reserve(9, F12_rm9, 9), o_e = b.reserve(2, epipole2, 2);
  const size_t o_sf = b.reserve(nlevels, scale_factors, nlevels), o_s2 = b.reserve(nlevels, level_sigma2, nlevels);
  const size_t o_n = b.reserve(3, counts, 3), o_m = b.reserve<int32_t>(cap);
  SD_TRY(b.run("sd_debug_search_for_triangulation", [&] {
    const TriBuffers tb = {b.dev<uint8_t>(o_h1), b.dev<uint8_t>(o_h2), b.dev<float>(o_u1), b.dev<float>(o_u2), b.dev<double>(o_F),
                           b.dev<float>(o_e), b.dev<float>(o_sf), b.dev<float>(o_s2), b.dev<int32_t>(o_m), b.dev<int32_t>(o_n) + 2};
    return launch_search_triangulation(b.dev<sd_keypoint>(o_k1), b.dev<uint8_t>(o_d1), b.dev<int32_t>(o_n), b.dev<sd_keypoint>(o_k2),
                                       b.dev<uint8_t>(o_d2), b.dev<int32_t>(o_n) + 1, tb, -1, (int)cap, nlevels, 1, check_ori, 0);
  }));
  b.take(matches12, o_m, (size_t)n1 * 4);
  b.take(n_matches, o_n + 8, 4);
  return SD_OK;
}

}  // extern "C"
