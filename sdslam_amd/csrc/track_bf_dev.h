// The scaffold the two brute-force Hamming matchers share: k_search_points (track_bf.hip) and k_search_triangulation (track_tri.hip).
// One workgroup of BF_THREADS per keyframe pair.  The KF1 rows that take part are compacted, ascending, into s_i1; a lane owns BF_PT
// of them (descriptors in registers); the KF2 descriptors pass through LDS in tiles of BF_TILE and are read as broadcasts, and the
// scan runs over the SET BITS of the tile's eligibility words on the scalar unit, so ineligible keypoints cost nothing.  What a
// row keeps of a candidate, and every gate, is the kernel's own.
#pragma once
#include "track_match_dev.h"

namespace sd {

#define BF_THREADS 256
#define BF_PT 2         // KF1 rows per lane
#define BF_TH_LOW 50
#define BF_NONE 0xFFFFFFFFu

// Slot f pairs frame f (or the broadcast frame) of the `cur` extractor -- KF1 -- with frame f of the `ref` extractor -- KF2
struct BfSlot {
  int fc, N1, N2;
  const sd_keypoint *kps1, *kps2;
  const uint32_t *desc1, *desc2;
  __device__ __forceinline__ BfSlot(const sd_keypoint* kps1_all, const uint8_t* desc1_all, const int32_t* n1_all, const sd_keypoint* kps2_all,
                                    const uint8_t* desc2_all, const int32_t* n2_all, int f, int cur_bcast, int cap)
      : fc(cur_bcast >= 0 ? cur_bcast : f), N1(min(max(n1_all[fc], 0), cap)), N2(min(max(n2_all[f], 0), cap)),
        kps1(kps1_all + (size_t)fc * cap), kps2(kps2_all + (size_t)f * cap),
        desc1((const uint32_t*)(desc1_all + (size_t)fc * cap * 32)), desc2((const uint32_t*)(desc2_all + (size_t)f * cap * 32)) {}
};

// The KF1 rows i < capw with pred(i), ascending, to s_i1 and their number to *s_n1v.  One wave calls.
template <typename Pred>
__device__ __forceinline__ void bf_compact_rows(Pred pred, int capw, uint16_t* s_i1, int* s_n1v, int lane) {
  const unsigned long long lt = lanemask_lt(lane);
  int n = 0;
  for (int i0 = 0; i0 < capw; i0 += 64) {
    const bool ok = pred(i0 + lane);
    const int pos = wave_append(ok, lt, n);
    if (ok) s_i1[pos] = (uint16_t)(i0 + lane);
  }
  if (lane == 0) *s_n1v = n;
}

// KF2 descriptors [j0, j0 + jn) to s_tile, between the barrier that ends the reads of the previous tile and the one that
// publishes this tile; also() stages whatever else the kernel keeps per tile.  All BF_THREADS call.
template <typename Also>
__device__ __forceinline__ void bf_stage_tile(const uint32_t* desc2, int j0, int jn, uint32_t* s_tile, int tid, Also also) {
  __syncthreads();
  for (int w = tid; w < jn * 2; w += BF_THREADS) ((uint4*)s_tile)[w] = ((const uint4*)(desc2 + (size_t)j0 * 8))[w];
  also();
  __syncthreads();
}

// body(bit) for every set bit of `word`, ascending.  The word is made wave-uniform, so the walk is a scalar loop and `bit` a scalar.
template <typename Body>
__device__ __forceinline__ void for_each_set_bit(uint32_t word, Body body) {
  uint32_t mask = (uint32_t)__builtin_amdgcn_readfirstlane((int)word);
  while (mask) {
    const int bit = __ffs((int)mask) - 1;
    mask &= mask - 1;
    body(bit);
  }
}

// Rotation consistency (src/ORBmatcher.cc:1269-1296, :434-463) once the scan is over -- the bins never influence a match decision:
// histogram of rot_bin over the matched rows, ComputeThreeMaxima, and the matches outside the three bins go.  rot_bin is pure and
// is evaluated again for the cut.  One wave calls, s_hist zeroed; returns the number of matches dropped.
__device__ __forceinline__ int bf_rotation_cut(const BfSlot& S, const uint16_t* s_i1, int n1v, int16_t* s_match, int* s_hist, int lane) {
  for (int e = lane; e < n1v; e += 64) {
    const int i1 = s_i1[e], j = s_match[i1];
    if (j >= 0) atomicAdd(&s_hist[rot_bin(S.kps1[i1].angle, S.kps2[j].angle)], 1);
  }
  __threadfence_block();
  int ind1, ind2, ind3;
  three_maxima(s_hist, ind1, ind2, ind3);
  int dropped = 0;
  for (int e0 = 0; e0 < n1v; e0 += 64) {
    const int e = e0 + lane;
    bool drop = false;
    if (e < n1v) {
      const int i1 = s_i1[e], j = s_match[i1];
      if (j >= 0) {
        const int bin = rot_bin(S.kps1[i1].angle, S.kps2[j].angle);
        drop = bin != ind1 && bin != ind2 && bin != ind3;
        if (drop) s_match[i1] = -1;
      }
    }
    dropped += __popcll(__ballot(drop));
  }
  return dropped;
}

// The matches of the slot's KF1 row and their number.  One wave calls.
__device__ __forceinline__ void bf_write_out(const int16_t* s_match, int cap, int nmatches, int32_t* out, int32_t* n_out, int lane) {
  for (int i = lane; i < cap; i += 64) out[i] = (int32_t)s_match[i];
  if (lane == 0) *n_out = nmatches;
}

}  // namespace sd
