// Device helpers the matchers of track_match.hip, track_bf.hip, track_tri.hip and track_fuse.hip share.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "orb_internal.h"
#include "sd_wave.h"
#include "track_internal.h"
#include "track_match_lds.h"

namespace sd {

template <typename T>
__device__ __forceinline__ T* lds_at(uint8_t* smem, uint32_t off) { return (T*)(smem + off); }

// Flags pred(i), i in [0, n_bits), packed into the 32-bit words dst[0 .. (n_bits + 31) / 32): one flag per thread and round,
// a wave's 64 flags are one ballot = two words.  All NT threads call (NT a multiple of 64; tid = lane for a single wave).
template <typename Pred>
__device__ __forceinline__ void pack_flags(Pred pred, int n_bits, uint32_t* dst, int tid, int NT) {
  const int lane = tid & 63, wave = tid >> 6, n_words = (n_bits + 31) >> 5;
  for (int i0 = 0; i0 < ((n_bits + 63) & ~63); i0 += NT) {
    const unsigned long long b = __ballot(pred(i0 + tid));
    const int w = (i0 >> 5) + 2 * wave;
    if (lane == 0 && w < n_words) {
      dst[w] = (uint32_t)b;
      if (w + 1 < n_words) dst[w + 1] = (uint32_t)(b >> 32);
    }
  }
}

// Bin of the rotation histogram for the angle difference a - b (src/ORBmatcher.cc:1043-1049)
__device__ __forceinline__ int rot_bin(float a, float b) {
  const float factor = 1.0f / HISTO_LENGTH;
  float rot = a - b;
  if (rot < 0.0) rot += 360.0f;
  const int bin = (int)roundf(rot * factor);
  return bin == HISTO_LENGTH ? 0 : bin;
}

// ORBmatcher::ComputeThreeMaxima (src/ORBmatcher.cc:1423-1454) on the bin counts: the three dominant bins, -1 for one that
// holds fewer than 10 % of the largest
__device__ __forceinline__ void three_maxima(const int* hist, int& ind1, int& ind2, int& ind3) {
  int i1 = -1, i2 = -1, i3 = -1;   // (locals, handed out at the end: the compiler keeps them in registers)
  int max1 = 0, max2 = 0, max3 = 0;
  for (int b = 0; b < HISTO_LENGTH; b++) {
    const int sh = hist[b];
    if (sh > max1) {
      max3 = max2; max2 = max1; max1 = sh;
      i3 = i2; i2 = i1; i1 = b;
    } else if (sh > max2) {
      max3 = max2; max2 = sh;
      i3 = i2; i2 = b;
    } else if (sh > max3) {
      max3 = sh;
      i3 = b;
    }
  }
  if (max2 < 0.1f * (float)max1) i2 = i3 = -1;
  else if (max3 < 0.1f * (float)max1) i3 = -1;
  ind1 = i1; ind2 = i2; ind3 = i3;
}

// GL lanes of a wave work on one point.  64: the whole wave (`lane`, `lt` as usual, gm = ~0).  Fewer: one point per group, `glane` =
// lane within the group, `glt` = the lower lanes OF THE GROUP and `gm` = the group's lanes, both as bit masks of the 64-bit wave
// ballot.  The groups diverge freely; a ballot only ever carries the active lanes.
template <int GL>
struct SubWave {
  int group, glane;
  unsigned long long gm, glt;
  __device__ __forceinline__ explicit SubWave(int lane)
      : group(lane / GL), glane(lane % GL), gm(((1ull << GL) - 1ull) << (GL * group)), glt(((1ull << glane) - 1ull) << (GL * group)) {}
};

// ---- Frame bucket grid (shared by k_match, k_match_local, k_fuse and the debug read-out k_features_in_area) ----
// Frame::PosInGrid (src/Frame.cc:323-332, round()) as a sort key: cell << 11 | keypoint index, cell = posX * 48 + posY;
// 0xFFFFFFFF for a keypoint outside the grid (AssignFeaturesToGrid skips it).
__device__ __forceinline__ uint32_t grid_key(const sd_keypoint& kp, const TrackCam& cam, float invW, float invH, int i) {
  const int posX = (int)roundf((kp.x - cam.min_x) * invW);
  const int posY = (int)roundf((kp.y - cam.min_y) * invH);
  if (posX < 0 || posX >= GRID_COLS || posY < 0 || posY >= GRID_ROWS) return 0xFFFFFFFFu;
  return ((uint32_t)(posX * GRID_ROWS + posY) << 11) | (uint32_t)i;
}
// Ascending bitonic sort of v[0 .. n) in LDS, n a power of two.  All NT threads call, after a barrier that makes v complete;
// ends with a barrier.
__device__ __forceinline__ void bitonic_sort_lds(uint32_t* v, int n, int tid, int NT) {
  for (int k = 2; k <= n; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      for (int i = tid; i < n; i += NT) {
        const int ixj = i ^ j;
        if (ixj > i) {
          const uint32_t a = v[i], b = v[ixj];
          if ((a > b) == ((i & k) == 0)) {
            v[i] = b;
            v[ixj] = a;
          }
        }
      }
      __syncthreads();
    }
}
// Frame::AssignFeaturesToGrid (src/Frame.cc:179-192): sort of the KP2 keys in LDS (mGrid[x][y] in ascending keypoint index =
// one contiguous, ordered run per cell) and the first sorted position of every cell.  All NT threads call, after a barrier
// that makes s_key complete; ends with s_cstart written but NOT yet synchronised.
__device__ __forceinline__ void grid_sort_and_starts(uint32_t* s_key, uint16_t* s_cstart, int KP2, int tid, int NT) {
  bitonic_sort_lds(s_key, KP2, tid, NT);
  for (int c = tid; c <= GRID_COLS * GRID_ROWS; c += NT) {
    const uint32_t target = (uint32_t)c << 11;
    int lo = 0, hi = KP2;
    while (lo < hi) {
      int mid = (lo + hi) >> 1;
      if (s_key[mid] < target) lo = mid + 1;
      else hi = mid;
    }
    s_cstart[c] = (uint16_t)lo;
  }
}

}  // namespace sd
