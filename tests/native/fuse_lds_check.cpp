// Host check of k_fuse's dynamic-LDS layout (LdsFuse, sdslam_amd/csrc/track_match_lds.h), built with AddressSanitizer and
// UBSan, in the manner of match_lds_check.cpp: for every capacity the launcher can pass, every array is aligned to its element
// size, the arrays do not overlap, the last one ends inside `bytes`, `bytes` equals the sum written out below, and a walk that
// writes every element of every array through the kernel's own offsets stays inside an allocation of `bytes` (the sanitizer
// watches) and leaves no array's pattern damaged by another's.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "track_match_lds.h"

using namespace sd;

struct Arr { const char* name; uint32_t off, elem, count; };

int main() {
  const uint32_t CS = GRID_COLS * GRID_ROWS + 2;
  int n = 0;
  for (int KP2 = 64; KP2 <= 2048; KP2 <<= 1, n++) {
    const LdsFuse L(KP2);
    std::vector<Arr> arrs = {{"key", L.key, 4, (uint32_t)KP2}, {"cstart", L.cstart, 2, CS}, {"pose", L.pose, 8, 16}, {"nfound", L.nfound, 4, 1}};
    auto fail = [&](const char* what, const Arr& x) {
      std::printf("LdsFuse(%d): %s: %s at %u, %u x %u bytes, total %u\n", KP2, what, x.name, x.off, x.count, x.elem, L.bytes);
      std::exit(1);
    };
    for (const Arr& x : arrs)
      if (x.off % x.elem) fail("misaligned", x);
    std::sort(arrs.begin(), arrs.end(), [](const Arr& p, const Arr& q) { return p.off < q.off; });
    for (size_t i = 0; i + 1 < arrs.size(); i++)
      if (arrs[i].off + arrs[i].elem * arrs[i].count > arrs[i + 1].off) fail("overlaps its successor", arrs[i]);
    if (arrs.back().off + arrs.back().elem * arrs.back().count > L.bytes) fail("ends past the total", arrs.back());
    // key | cstart | pad to 8 | pose | nfound
    const size_t head = (size_t)KP2 * 4 + (size_t)CS * 2;
    const size_t want = ((head + 7) & ~(size_t)7) + 16 * 8 + 4;
    if (L.bytes != want) {
      std::printf("LdsFuse(%d): %u bytes, expected %zu\n", KP2, L.bytes, want);
      return 1;
    }
    if (L.bytes > 64 * 1024) {
      std::printf("LdsFuse(%d): %u bytes exceed a workgroup's 64 KB\n", KP2, L.bytes);
      return 1;
    }
    // the sweep: an exact-size heap block, every element written through its offset, then read back
    uint8_t* smem = (uint8_t*)std::malloc(L.bytes);
    std::memset(smem, 0, L.bytes);
    for (size_t a = 0; a < arrs.size(); a++)
      for (uint32_t i = 0; i < arrs[a].count; i++) std::memset(smem + arrs[a].off + (size_t)i * arrs[a].elem, (int)(a + 1), arrs[a].elem);
    for (size_t a = 0; a < arrs.size(); a++)
      for (uint32_t b = 0; b < arrs[a].count * arrs[a].elem; b++)
        if (smem[arrs[a].off + b] != (uint8_t)(a + 1)) fail("pattern damaged", arrs[a]);
    std::free(smem);
  }
  std::printf("fuse_lds_check OK (%d capacities)\n", n);
  return 0;
}
