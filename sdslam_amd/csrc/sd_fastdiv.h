// Division of a 32-bit index by a launch-constant divisor as ONE 32-bit multiply-high: the only place the extraction path builds
// such a "magic number", and the range over which each is exact as a predicate the plan evaluates (orb_plan.cpp) instead of a
// comment.  Plain C++ (no HIP): the kernels apply a magic with a bare __umulhi, the host checks call fastdiv_apply;
// tests/native/orb_fast_lds_check.cpp sweeps both recipes against plain division.
//
// Recipe 1, e / d == umulhi(e, fastdiv_magic(d)):  m = floor((2^32 - 1) / d) + 1 = ceil(2^32 / d) for d >= 2 (for d == 1 it is
//   2^32, which 32 bits do not hold: a divisor of 1 has no magic number).  Write m d = 2^32 + r, 0 <= r < d, and e = q d + s,
//   0 <= s < d.  Then e m / 2^32 = e / d + e r / (d 2^32) = q + s / d + e r / (d 2^32), and s / d <= 1 - 1 / d, so the floor
//   is q while e r / (d 2^32) < 1 / d, i.e. e r < 2^32.  r < d, hence SUFFICIENT: d >= 2 and max_e * d < 2^32.
//   Not loose by much where r = d - 1 (d | 2^32 - 1): d = 3 is exact up to e = 1431655765 by the predicate and wrong at e = 2^31.
//
// Recipe 2, e / d == umulhi(2 e + 1, fastdiv_magic_odd(d)):  M = floor(2^31 / d), 2^31 = M d + t, 0 <= t < d.  Then
//   (2 e + 1) M / 2^32 = q + (s + 1/2) / d - (2 e + 1) t / (d 2^32).  (s + 1/2) / d < 1, so the floor never exceeds q, and it is
//   q while (2 e + 1) t <= (2 s + 1) 2^31, at worst (s = 0) while (2 e + 1) t <= 2^31.  t <= d - 1, hence SUFFICIENT: d >= 1,
//   max_e < 2^31 (2 e + 1 is a 32-bit operand) and (2 max_e + 1) (d - 1) <= 2^31.  That holds for every e when d == 1, which is
//   what the recipe is for, and it follows from the shorter e d <= 2^30 that k_fast_cells' comment used to give.  d = 3 (t = 2) is
//   exact up to e = 2^29 - 1 by the predicate and wrong at e = 2^29 + 1.
#pragma once
#include <stdint.h>

namespace sd {

constexpr uint32_t fastdiv_magic(uint32_t d) { return 0xFFFFFFFFu / d + 1u; }
constexpr bool fastdiv_exact(uint32_t d, uint64_t max_e) { return d >= 2 && max_e < (1ull << 32) && max_e * d < (1ull << 32); }

constexpr uint32_t fastdiv_magic_odd(uint32_t d) { return 0x80000000u / d; }
constexpr bool fastdiv_odd_exact(uint32_t d, uint64_t max_e) {
  return d >= 1 && max_e < (1ull << 31) && (2 * max_e + 1) * (uint64_t)(d - 1) <= (1ull << 31);
}

// what __umulhi computes, for host-side checks
constexpr uint32_t fastdiv_apply(uint32_t e, uint32_t magic) { return (uint32_t)(((uint64_t)e * magic) >> 32); }
constexpr uint32_t fastdiv_apply_odd(uint32_t e, uint32_t magic_odd) { return fastdiv_apply(2u * e + 1u, magic_odd); }

}  // namespace sd
