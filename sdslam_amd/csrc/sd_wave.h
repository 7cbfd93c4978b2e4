// Wave-level idioms every kernel file uses: lane masks, the ordered ballot-append, the device library's wave reductions, the
// wave fence and the 256-bit Hamming distance.  Device-only, stateless, nothing of the tracker or the extractor.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace sd {

// Bits of the lanes below `lane` in a 64-bit ballot
__device__ __forceinline__ unsigned long long lanemask_lt(int lane) { return lane == 0 ? 0ull : (~0ull >> (64 - lane)); }

// Ordered append of the lanes with `pred` to a list that holds n entries (n wave-uniform): returns this lane's position -- lanes
// ascending, meaningful where pred holds -- and advances n by the number of such lanes.  lt = lanemask_lt(lane).
__device__ __forceinline__ int wave_append(bool pred, unsigned long long lt, int& n) {
  const unsigned long long b = __ballot(pred);
  const int pos = n + __popcll(b & lt);
  n += __popcll(b);
  return pos;
}

// Reductions over the wave, every lane gets the result: the device library's DPP reductions.
extern "C" __device__ __attribute__((const)) double __ockl_wfred_add_f64(double);
extern "C" __device__ __attribute__((const)) int __ockl_wfred_add_i32(int);
extern "C" __device__ __attribute__((const)) unsigned int __ockl_wfred_min_u32(unsigned int);
__device__ __forceinline__ double wave_sum(double v) { return __ockl_wfred_add_f64(v); }
__device__ __forceinline__ int wave_sum_i32(int v) { return __ockl_wfred_add_i32(v); }
// Instead of six LDS-crossbar shuffles (the serial phase-2 chain of the matchers does one per point: single-frame search
// 1.25 -> 0.97 ms; A/B on one box at 1024 frames: 129.6 k vs 129.2 k frames/s).
__device__ __forceinline__ uint32_t wave_min_u32(uint32_t v) { return __ockl_wfred_min_u32(v); }

// Orders this wave's LDS / memory accesses before the fence against those after it, for the other lanes of the wave
__device__ __forceinline__ void wave_fence() { __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront"); }

// Hamming distance of two 256-bit descriptors (ORBmatcher::DescriptorDistance), as 8 x u32 (v_bcnt_u32_b32 accumulates) ...
__device__ __forceinline__ int hamming256(const uint32_t (&a)[8], const uint32_t (&b)[8]) {
  int d = 0;
#pragma unroll
  for (int k = 0; k < 8; k++) d += __popc(a[k] ^ b[k]);
  return d;
}
// ... and as 4 x u64
__device__ __forceinline__ int hamming256(unsigned long long a0, unsigned long long a1, unsigned long long a2, unsigned long long a3,
                                          unsigned long long b0, unsigned long long b1, unsigned long long b2, unsigned long long b3) {
  return __popcll(a0 ^ b0) + __popcll(a1 ^ b1) + __popcll(a2 ^ b2) + __popcll(a3 ^ b3);
}
// Descriptor i of a 16-byte aligned array of 32-byte descriptors (global or LDS), as two 16-byte loads
__device__ __forceinline__ void load_desc8(const uint32_t* desc, int i, uint32_t (&d)[8]) {
  const uint4 a = ((const uint4*)(desc + (size_t)i * 8))[0], b = ((const uint4*)(desc + (size_t)i * 8))[1];
  d[0] = a.x; d[1] = a.y; d[2] = a.z; d[3] = a.w;
  d[4] = b.x; d[5] = b.y; d[6] = b.z; d[7] = b.w;
}

}  // namespace sd
