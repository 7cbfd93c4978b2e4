// Host check of k_refresh_points' static LDS layout (LdsRefreshWave, sdslam_amd/csrc/track_refresh_lds.h), built with
// AddressSanitizer and UBSan, in the manner of fuse_lds_check.cpp: every wave's arrays lie inside the workgroup's block and
// inside a workgroup's 64 KB, the terms alias the descriptor words and nothing else, no two waves share a byte, a walk through
// the kernel's own index functions stays inside an allocation of that size, and the accesses the header calls conflict-free are:
//   ds_write_b64 of a lane's own term        16 contiguous lanes a group, bank = (byte / 4) mod 32, two dwords a lane
//   ds_write_b32 / ds_read_b32 of a lane's   32 lanes a group, bank = (byte / 4) mod 32
//     own descriptor word (rows l + 64 r)
//   every lane reading descriptor j          one address: a broadcast
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>

#include "track_refresh_lds.h"

using namespace sd;

#define CHECK(cond, ...)                 \
  do {                                   \
    if (!(cond)) {                       \
      std::printf("FAILED %s: ", #cond); \
      std::printf(__VA_ARGS__);          \
      std::printf("\n");                 \
      std::exit(1);                      \
    }                                    \
  } while (0)

int main() {
  constexpr LdsRefreshWave L;
  CHECK(kLdsRefreshBytes == L.bytes * REFRESH_WAVES && kLdsRefreshBytes <= 64 * 1024, "%u bytes", kLdsRefreshBytes);
  CHECK(L.bytes % 16 == 0 && L.desc % 16 == 0 && L.term % 8 == 0 && L.pos % 2 == 0, "alignment");
  const uint32_t desc_end = L.desc + 8 * REFRESH_CAP * 4, term_end = L.term + 3 * REFRESH_CAP * 8, pos_end = L.pos + REFRESH_CAP * 2;
  CHECK(L.term >= L.desc && term_end <= desc_end, "the terms alias the descriptor words only");
  CHECK(L.pos >= desc_end && pos_end <= L.bytes, "pos lies beside them, inside the wave's region");
  CHECK(L.bytes == 8 * REFRESH_CAP * 4 + REFRESH_CAP * 2, "%u bytes a wave, expected 8 KB + 512", L.bytes);

  // the sweep: an exact-size heap block, every element written through the kernel's index functions, then read back
  uint8_t* smem = (uint8_t*)std::malloc(kLdsRefreshBytes);
  std::memset(smem, 0, kLdsRefreshBytes);
  for (uint32_t w = 0; w < REFRESH_WAVES; w++) {
    uint8_t* mine = smem + (size_t)w * L.bytes;
    double* term = (double*)(mine + L.term);
    for (uint32_t k = 0; k < 3; k++)
      for (uint32_t o = 0; o < REFRESH_CAP; o++) term[LdsRefreshWave::term_at(k, o)] = 1.0;
    uint32_t* desc = (uint32_t*)(mine + L.desc);
    for (uint32_t k = 0; k < 8; k++)
      for (uint32_t j = 0; j < REFRESH_CAP; j++) desc[LdsRefreshWave::desc_word(k, j)] = (w << 16) | (k << 8) | j;
    uint16_t* pos = (uint16_t*)(mine + L.pos);
    for (uint32_t j = 0; j < REFRESH_CAP; j++) pos[j] = (uint16_t)(w * 1000 + j);
  }
  for (uint32_t w = 0; w < REFRESH_WAVES; w++) {
    const uint8_t* mine = smem + (size_t)w * L.bytes;
    for (uint32_t k = 0; k < 8; k++)
      for (uint32_t j = 0; j < REFRESH_CAP; j++)
        CHECK(((const uint32_t*)(mine + L.desc))[LdsRefreshWave::desc_word(k, j)] == ((w << 16) | (k << 8) | j), "wave %u word %u of %u", w, k, j);
    for (uint32_t j = 0; j < REFRESH_CAP; j++) CHECK(((const uint16_t*)(mine + L.pos))[j] == (uint16_t)(w * 1000 + j), "pos %u", j);
  }
  std::free(smem);
  // distinct (k, o) / (w, j) are distinct elements
  std::set<uint32_t> seen;
  for (uint32_t k = 0; k < 8; k++)
    for (uint32_t j = 0; j < REFRESH_CAP; j++) CHECK(seen.insert(LdsRefreshWave::desc_word(k, j)).second && LdsRefreshWave::desc_word(k, j) < 8 * REFRESH_CAP, "desc_word");
  seen.clear();
  for (uint32_t k = 0; k < 3; k++)
    for (uint32_t o = 0; o < REFRESH_CAP; o++) CHECK(seen.insert(LdsRefreshWave::term_at(k, o)).second && LdsRefreshWave::term_at(k, o) < 3 * REFRESH_CAP, "term_at");

  int groups = 0;
  for (uint32_t wave = 0; wave < REFRESH_WAVES; wave++) {
    const uint32_t base = wave * L.bytes;
    // a lane's own descriptor word, rows l + 64 r: 32-lane groups, 32 banks
    for (uint32_t r = 0; r < REFRESH_CAP / 64; r++)
      for (uint32_t w = 0; w < 8; w++)
        for (uint32_t g = 0; g < 2; g++, groups++) {
          std::set<uint32_t> banks;
          for (uint32_t l = 32 * g; l < 32 * g + 32; l++) banks.insert(((base + L.desc + 4 * LdsRefreshWave::desc_word(w, l + 64 * r)) / 4) % 32);
          CHECK(banks.size() == 32, "own word %u of rows +%u: %zu banks for 32 lanes", w, 64 * r, banks.size());
        }
    // a lane's own term, observations l + 64 r: 16-lane groups, two dwords a lane, 32 banks
    for (uint32_t r = 0; r < REFRESH_CAP / 64; r++)
      for (uint32_t k = 0; k < 3; k++)
        for (uint32_t g = 0; g < 4; g++, groups++) {
          std::set<uint32_t> banks;
          for (uint32_t l = 16 * g; l < 16 * g + 16; l++) {
            const uint32_t a = base + L.term + 8 * LdsRefreshWave::term_at(k, l + 64 * r);
            banks.insert((a / 4) % 32);
            banks.insert((a / 4 + 1) % 32);
          }
          CHECK(banks.size() == 32, "own term %u of observations +%u: %zu banks for 16 lanes", k, 64 * r, banks.size());
        }
  }
  std::printf("refresh_lds_check OK (%u bytes a workgroup, %d lane groups)\n", kLdsRefreshBytes, groups);
  return 0;
}
