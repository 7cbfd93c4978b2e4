// ORBmatcher::SearchByPoints(KeyFrame* currentKF, KeyFrame* pKF, matches) on MI355X: brute-force Hamming matching of the
// map points of two keyframes (reference src/ORBmatcher.cc:1209-1301; called per loop candidate by
// LoopClosing::ComputeSim3, src/LoopClosing.cc:255).  BASELINE configs[1] ("ORB extract + Hamming match") / SURVEY §8(d)
// C2(ii): 1000 x 1000 descriptors per frame pair.
//
// One workgroup per keyframe pair; slot f pairs frame f (or the broadcast frame) of the `cur` extractor -- currentKF --
// with frame f of the `ref` extractor -- pKF.  The reference loop is sequential in idx1 only through vbMatched2 (a pKF point
// is given away once), so the work splits in two:
//   phase 1 (all lanes, N1 x N2 popcounts): every currentKF point with a map point gets the BF_K smallest keys
//            dist << 11 | idx2 over the pKF points with a map point.  The scan is the scaffold of track_bf_dev.h, which
//            k_search_triangulation shares: rows in registers, pKF tiles in LDS, a scalar walk over the validity bits.
//   phase 2 (one wave, idx1 ascending): the two smallest keys not yet given away = (bestDist1, bestIdx2) and bestDist2
//            -- both updated with strict `<` in idx2 order in the reference, which is exactly key order -- then the
//            TH_LOW / mfNNratio tests and vbMatched2.  When fewer than two of a point's BF_K keys survive and a further
//            candidate could still matter, the row is recomputed by the whole wave against the live vbMatched2.
//   rotation histogram (bf_rotation_cut) afterwards: the bins never feed back into the loop.
// Integer work only; results are bit-identical to the sequential loop by construction.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdlib>

#include "orb_internal.h"
#include "track_bf_dev.h"
#include "track_internal.h"

namespace sd {

__device__ __forceinline__ void bf_insert(uint32_t (&k)[BF_K], uint32_t key) {
  if (key < k[BF_K - 1]) {
#pragma unroll
    for (int q = 0; q < BF_K; q++) {
      const uint32_t lo = min(k[q], key);
      key = max(k[q], key);
      k[q] = lo;
    }
  }
}

// Dynamic LDS: LdsSearchPoints (track_match_lds.h)
__global__ __launch_bounds__(BF_THREADS) void k_search_points(const sd_keypoint* __restrict__ kps1_all, const uint8_t* __restrict__ desc1_all,
                                                              const int32_t* __restrict__ n1_all, const sd_keypoint* __restrict__ kps2_all,
                                                              const uint8_t* __restrict__ desc2_all, const int32_t* __restrict__ n2_all,
                                                              TrackBuffers tb, float nnratio, int check_ori, int capw /* cap rounded up to 64 */,
                                                              int klist /* keys of a point's list phase 2 may use: BF_K (tests: fewer) */) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const LdsSearchPoints L(capw);
  uint32_t* s_tile = lds_at<uint32_t>(smem, L.tile);
  uint32_t* s_list = lds_at<uint32_t>(smem, L.list);
  uint16_t* s_i1 = lds_at<uint16_t>(smem, L.i1);
  int16_t* s_match = lds_at<int16_t>(smem, L.match);
  uint32_t* s_v2 = lds_at<uint32_t>(smem, L.v2);
  uint32_t* s_m2 = lds_at<uint32_t>(smem, L.m2);
  int* s_hist = lds_at<int>(smem, L.hist);
  int* s_n1v = lds_at<int>(smem, L.n1v);
  const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int cap = tb.kp_cap;
  const BfSlot S(kps1_all, desc1_all, n1_all, kps2_all, desc2_all, n2_all, f, tb.cur_bcast, cap);
  const int N2 = S.N2;
  const uint8_t* v1 = tb.sp_valid1 + (size_t)f * cap;
  const uint8_t* v2 = tb.sp_valid2 + (size_t)f * cap;

  // ---- validity of the pKF points as bits; matched bits cleared; compacted list of the currentKF points (ascending)
  pack_flags([&](int i) { return i < N2 && v2[i] != 0; }, capw, s_v2, tid, BF_THREADS);
  for (int w = tid; w < capw >> 5; w += BF_THREADS) s_m2[w] = 0;
  for (int i = tid; i < capw; i += BF_THREADS) s_match[i] = -1;
  if (tid < 32) s_hist[tid] = 0;
  if (wave == 0) bf_compact_rows([&](int i) { return i < S.N1 && v1[i] != 0; }, capw, s_i1, s_n1v, lane);
  __syncthreads();
  const int n1v = *s_n1v;
  const int ntiles = (N2 + BF_TILE - 1) / BF_TILE;

  // ---- phase 1
  for (int e0 = 0; e0 < n1v; e0 += BF_THREADS * BF_PT) {
    uint32_t d1[BF_PT][8], top[BF_PT][BF_K];
    int ent[BF_PT];
#pragma unroll
    for (int p = 0; p < BF_PT; p++) {
      ent[p] = e0 + p * BF_THREADS + tid;
      load_desc8(S.desc1, ent[p] < n1v ? s_i1[ent[p]] : 0, d1[p]);
#pragma unroll
      for (int q = 0; q < BF_K; q++) top[p][q] = BF_NONE;
    }
    for (int t = 0; t < ntiles; t++) {
      const int j0 = t * BF_TILE, jn = min(BF_TILE, N2 - j0);
      bf_stage_tile(S.desc2, j0, jn, s_tile, tid, [] {});
      for (int wd = 0; wd < (jn + 31) >> 5; wd++)
        for_each_set_bit(s_v2[(j0 >> 5) + wd], [&](int bit) {
          const int jl = wd * 32 + bit;
          uint32_t d2[8];
          load_desc8(s_tile, jl, d2);   // LDS broadcast
#pragma unroll
          for (int p = 0; p < BF_PT; p++) bf_insert(top[p], ((uint32_t)hamming256(d1[p], d2) << 11) | (uint32_t)(j0 + jl));
        });
    }
#pragma unroll
    for (int p = 0; p < BF_PT; p++)
      if (ent[p] < n1v) {
#pragma unroll
        for (int q = 0; q < BF_K; q++) s_list[(size_t)ent[p] * BF_K + q] = top[p][q];
      }
  }
  __syncthreads();
  if (tid >= 64) return;   // one wavefront runs the order-dependent loop

  // ---- phase 2: for (idx1 ascending) best / second best among the pKF points not yet given away
  int nmatches = 0;
  for (int e = 0; e < n1v; e++) {
    uint32_t key = BF_NONE;
    if (lane < klist) key = s_list[(size_t)e * BF_K + lane];
    const bool have = key != BF_NONE;                        // the list ends where the pKF candidates end
    const bool taken = have && ((s_m2[(key & 2047) >> 5] >> (key & 31)) & 1u);
    const unsigned long long bhave = __ballot(have), bavail = __ballot(have && !taken);
    const int navail = __popcll(bavail);
    uint32_t k1 = BF_NONE, k2 = BF_NONE;
    if (navail >= 1) k1 = (uint32_t)__builtin_amdgcn_readlane((int)key, __ffsll((long long)bavail) - 1);
    if (navail >= 2) k2 = (uint32_t)__builtin_amdgcn_readlane((int)key, __ffsll((long long)(bavail & (bavail - 1))) - 1);
    const bool complete = __popcll(bhave) < klist;           // fewer than klist candidates exist at all: the list is everything
    if (navail < 2 && !complete) {
      // a candidate beyond the list could be the best or the second best; every such key is >= the list's last one
      const uint32_t klast = (uint32_t)__shfl((int)key, klist - 1);
      const uint32_t lower = navail >= 1 ? k1 : klast;       // smallest key the best can still have
      if ((int)(lower >> 11) < BF_TH_LOW) {
        // whole-wave recomputation of the row against the live vbMatched2
        uint32_t a1[8];
        load_desc8(S.desc1, s_i1[e], a1);
        uint32_t m0 = BF_NONE, m1 = BF_NONE;
        for (int j = lane; j < N2; j += 64) {
          if (!((s_v2[j >> 5] >> (j & 31)) & 1u) || ((s_m2[j >> 5] >> (j & 31)) & 1u)) continue;
          uint32_t b2[8];
          load_desc8(S.desc2, j, b2);
          const uint32_t kk = ((uint32_t)hamming256(a1, b2) << 11) | (uint32_t)j;
          if (kk < m0) { m1 = m0; m0 = kk; }
          else if (kk < m1) m1 = kk;
        }
        k1 = wave_min_u32(m0);
        if (m0 == k1) m0 = m1;                               // keys are unique: exactly one lane gives up its first
        k2 = wave_min_u32(m0);
      } else {
        k1 = BF_NONE;                                        // bestDist1 >= TH_LOW whatever lies beyond the list: no match
      }
    }
    const int bestDist1 = k1 == BF_NONE ? 256 : (int)(k1 >> 11);
    const int bestDist2 = k2 == BF_NONE ? 256 : (int)(k2 >> 11);
    if (bestDist1 < BF_TH_LOW && (float)bestDist1 < nnratio * (float)bestDist2) {
      const int j = k1 & 2047;
      if (lane == 0) {
        s_match[s_i1[e]] = (int16_t)j;
        s_m2[j >> 5] |= 1u << (j & 31);
      }
      nmatches++;
    }
  }
  if (check_ori) nmatches -= bf_rotation_cut(S, s_i1, n1v, s_match, s_hist, lane);
  bf_write_out(s_match, cap, nmatches, tb.sp_match + (size_t)f * cap, tb.sp_n + f, lane);
}

int launch_search_points(const sd_orb* cur, const sd_orb* ref, const TrackBuffers& tb, int n_frames, float nnratio, int check_ori,
                         hipStream_t s) {
  const int capw = (tb.kp_cap + 63) & ~63;
  SD_REQUIRE(capw <= 2048, SD_ERR_CAPACITY, "SearchByPoints supports at most 2048 keypoints per keyframe");
  // option "track.bf_list_k" = 1..3 (tests): phase 2 sees only the first keys of every list, so the whole-wave recomputation -- rare on real
  // data -- runs for most points
  const int klist = std::min(BF_K, std::max(1, opt(OPT_BF_LIST_K)));
  hipLaunchKernelGGL(k_search_points, dim3(n_frames), dim3(BF_THREADS), LdsSearchPoints(capw).bytes, s, keys_un(cur), cur->d_desc,
                     cur->d_nout, keys_un(ref), ref->d_desc, ref->d_nout, tb, nnratio, check_ori, capw, klist);
  SD_HIP_CHECK(hipGetLastError());
  return SD_OK;
}

}  // namespace sd
