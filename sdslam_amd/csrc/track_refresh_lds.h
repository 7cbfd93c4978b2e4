// Static-LDS layout of k_refresh_points (track_refresh.hip): one region per wave = per map point, REFRESH_WAVES of them per
// workgroup.  Plain C++ (no HIP): tests/native/refresh_lds_check.cpp checks the bounds, the aliasing and the bank claims on the host.
//
// A region holds, one after the other in time,
//   term  double[3][REFRESH_CAP]     component k of observation o's unit viewing direction at k * REFRESH_CAP + o.  Lane l writes
//                                    its own observations (ds_write_b64: 16 contiguous lanes a group, banks of 32 dwords: dwords
//                                    2l, 2l + 1 -- conflict-free); lanes 0..2 then walk one component each, in list order.
//   desc  uint32_t[8][REFRESH_CAP]   word w of compacted descriptor j at w * REFRESH_CAP + j ("word-major").  Lane l reading word
//                                    w of ITS descriptor l + 64 r is a ds_read_b32 (32 lanes a group, 32 banks): bank (l + 64 r)
//                                    mod 32 = l mod 32, conflict-free; every lane reading word w of descriptor j is one address, a
//                                    broadcast.  A 32-byte row per descriptor would put lanes l and l + 8 of a ds_read_b128 group
//                                    on one bank (2-way).
// and beside them
//   pos   uint16_t[REFRESH_CAP]      compacted row j -> position in the caller's list (the bad keyframes are skipped)
// term is dead (two barriers) before desc is written, so the two share their bytes.
#pragma once
#include <stdint.h>

#include "track_match_lds.h"

namespace sd {

#define REFRESH_CAP 256     // observations per point (SD_REFRESH_MAX_OBS)
#define REFRESH_WAVES 4     // points per workgroup

struct LdsRefreshWave : LdsLayout {
  uint32_t desc = 0, term = 0, pos = 0;
  constexpr LdsRefreshWave() {
    desc = take<LdsQuad>(8 * REFRESH_CAP * 4 / 16);
    term = desc;                                   // 3 * REFRESH_CAP doubles inside the 8 * REFRESH_CAP dwords
    pos = take<uint16_t>(REFRESH_CAP);
    bytes += (0u - bytes) & 15u;                   // the next wave's region starts 16-byte aligned
  }
  static constexpr uint32_t desc_word(uint32_t w, uint32_t j) { return w * REFRESH_CAP + j; }   // in dwords from desc
  static constexpr uint32_t term_at(uint32_t k, uint32_t o) { return k * REFRESH_CAP + o; }     // in doubles from term
};
static_assert(3 * REFRESH_CAP * 8 <= 8 * REFRESH_CAP * 4, "the terms must fit the descriptor area they alias");

constexpr uint32_t kLdsRefreshBytes = LdsRefreshWave().bytes * REFRESH_WAVES;

}  // namespace sd
