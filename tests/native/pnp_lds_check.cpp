// Host check of k_pnp's LDS address map (csrc/track_pnp_lds.h): every LDS instruction of the cooperative 12 x 12 Jacobi sweeps,
// for all 21 steps of a sweep, is replayed on the bank rules of gfx950 and its conflict degree counted.
//   ds_read_b64:  lane groups {0-31}, {32-63}; bank of byte address a = (a / 4) mod 64 (a double covers two banks)
//   ds_write_b64 / ds_read2_b64: groups of 16 consecutive lanes; bank = (a / 4) mod 32
// Lanes of a group that hit one bank with different addresses are served one after the other: degree = the largest number of
// distinct addresses on one bank within one group.  Also: the map is a bijection onto [0, kWorkDoubles), and the unpadded map
// the kernel had before is counted the same way for comparison.
#include <algorithm>
#include <cstdio>
#include <set>
#include <vector>

#include "track_pnp_lds.h"

using namespace sd::pnp_lds;

static int old_index(int row, int k, int h) { return k == kMatW ? (144 + row) * PNP_CHUNK + h : (row * 12 + k) * PNP_CHUNK + h; }

// degree of one wave-instruction: addr[lane] = double index or -1 (lane inactive)
static int degree(const std::vector<int>& addr, int group, int dword_banks) {
  int worst = 1;
  for (int g0 = 0; g0 < 64; g0 += group) {
    std::vector<std::set<int>> on_bank(dword_banks);
    for (int l = g0; l < g0 + group; l++)
      if (addr[l] >= 0) {
        on_bank[(2 * addr[l]) % dword_banks].insert(addr[l]);
        on_bank[(2 * addr[l] + 1) % dword_banks].insert(addr[l]);
      }
    for (auto& s : on_bank) worst = std::max(worst, (int)s.size());
  }
  return worst;
}

template <typename Map>
static void sweep_degrees(Map&& index, bool refit, int nact, int* rd, int* wr) {
  for (int st = 1; st <= 21; st++)
    for (int k = 0; k <= kMatW; k++)
      for (int side = 0; side < 2; side++) {   // the instruction that touches row i, the one that touches row j
        std::vector<int> addr(64, -1);
        for (int lane = 0; lane < 64; lane++) {
          const int g = refit ? lane : lane / PNP_CHUNK, h = refit ? 0 : lane % PNP_CHUNK;
          const int i = std::max(0, st - 11) + g, j = st - i;
          if (g < 6 && i < j && h < nact) addr[lane] = index(side ? j : i, k, h);
        }
        *rd = std::max(*rd, degree(addr, 32, 64));
        *wr = std::max(*wr, degree(addr, 16, 32));
      }
}

int main() {
  std::set<int> seen;
  for (int h = 0; h < PNP_CHUNK; h++)
    for (int row = 0; row < 12; row++)
      for (int k = 0; k < kMatRow; k++) {
        const int a = mat_index(row, k, h);
        if (a < 0 || a >= kWorkDoubles || !seen.insert(a).second) {
          std::printf("map not a bijection at h=%d row=%d k=%d\n", h, row, k);
          return 1;
        }
      }
  int rd = 1, wr = 1, old_rd = 1, old_wr = 1, old_refit = 1, unused = 1;
  for (int nact = 1; nact <= PNP_CHUNK; nact++) sweep_degrees(mat_index, false, nact, &rd, &wr);
  sweep_degrees(mat_index, true, 1, &rd, &wr);
  sweep_degrees(old_index, false, PNP_CHUNK, &old_rd, &old_wr);
  sweep_degrees(old_index, true, 1, &old_refit, &unused);
  std::printf("unpadded map: reads %d-way, writes %d-way, refit %d-way\n", old_rd, old_wr, old_refit);
  std::printf("worst conflict degree: reads %d, writes %d\n", rd, wr);
  if (rd != 1 || wr != 1) return 1;
  std::printf("pnp_lds_check OK\n");
  return 0;
}
