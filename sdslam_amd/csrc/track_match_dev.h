// Device helpers the matchers of track_match.hip, track_bf.hip and track_tri.hip share.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "track_match_lds.h"

namespace sd {

template <typename T>
__device__ __forceinline__ T* lds_at(uint8_t* smem, uint32_t off) { return (T*)(smem + off); }

// Minimum over the wave, every lane gets it: the device library's DPP reduction instead of six LDS-crossbar shuffles
// (the serial phase-2 chain of the matchers does one per point: single-frame search 1.25 -> 0.97 ms; A/B on one box at
// 1024 frames: 129.6 k vs 129.2 k frames/s).
extern "C" __device__ __attribute__((const)) unsigned int __ockl_wfred_min_u32(unsigned int);
__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) { return __ockl_wfred_min_u32(v); }

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

}  // namespace sd
