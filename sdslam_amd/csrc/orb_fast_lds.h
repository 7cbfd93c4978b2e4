// Dynamic-LDS layout of k_fast_cells (orb.hip) and everything the kernel derives from a cell's zone: one struct, built by the
// kernel from its CellGeom and by plan_geometry (orb_plan.cpp) when it sizes the launch and checks the cell, so the two cannot
// disagree.  Plain C++ (no HIP): tests/native/orb_fast_lds_check.cpp sweeps it on the host.
//
// A workgroup works through its cell in strips of strip_rows zone rows.  A strip scores its own rows and one above / below (a
// whole-cell strip has neither): at most NSR rows.  Its LDS, in order:
//   tile    uint8_t[NSR + 6][TP]     the pixels of the scored rows and the 3-pixel ring around them.  Column 0 is source column
//                                    xa, the zone's first ring column xs = zx0 - 3 + edge aligned DOWN to 16 bytes (sh = xs - xa),
//                                    and the pitch TP = 16 TPU is a whole number of 16-byte units: a tile row is whole units in the
//                                    source and in LDS alike, staged as fast_u4 (or, from frames that are only 4-byte aligned, as
//                                    TPW = 4 TPU dwords).  Unit / dword i of the strip lands at LDS byte 16 i / 4 i.
//   sc      uint8_t[NSR + 2][TP]     the score map, rows -1 ... NSR and columns -1 ... TP - 2 of the zone, at the TILE's pitch:
//                                    a pixel's byte offset from the first zone pixel, y TP + x, addresses its ring (tile0 +
//                                    offset) and its score (sc0 + offset) alike.  That offset is the queue entry.
//   queue   uint16_t[4][QCAP]        per wave, the raster-ordered offsets of the pixels that pass the compass test; a wave owns
//                                    RPW = ceil(NSR / 4) rows, at worst every pixel of them (QCAP = RPW zw).  Entries are 16 bits:
//                                    (NSR + 1) TP <= 65536 (entries_fit16), which also keeps sc0 + entry + TP + 1, the furthest
//                                    score the NMS reads, a 16-bit quantity.
// tile and sc start 16-byte aligned (TP is a multiple of 16), the queues 2-byte aligned.
//
// The kernel recovers (row, column) from four flat indices by multiply-high (sd_fastdiv.h); div_*() give each division's divisor
// and the largest dividend the kernel can present, masked-off lanes included:
//   div_zw    phase A walks a wave's rows as one flat pixel range i = y zw + x < NSR zw
//   div_tp    the key of a survivor takes its queue entry apart: entry <= (NSR - 1) TP + zw - 1
//   div_tpu   16-byte staging, unit i of TPU (NSR + 6): a thread evaluates i0 + 256 j, j < FAST_STAGE_DEPTH / 4, for every
//             i0 < nu BEFORE the i < nu mask, so up to the next multiple of 256 FAST_STAGE_DEPTH / 4 (odd recipe: TPU is 1 for
//             zones narrower than 11 pixels)
//   div_tpw   dword staging, likewise in steps of 256 FAST_STAGE_DEPTH over TPW (NSR + 6) dwords
//
// What a launch requests is not a cell's exact size but the layout at the worst pad, worst_pad() (sh = 15; the same cell is
// staged from the caller's frames, edge 0, or from the padded pyramid, edge SD_EDGE, at different pads) plus kFastLdsSlack.
// The strip search of plan_geometry decides on the r2 sizes its budgets were measured with (fast_r2_bytes: 4-byte aligned tile
// pitch, tight score pitch) so that a cell that was one strip then stays one strip.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "sd_fastdiv.h"

#ifndef FAST_STAGE_DEPTH
#define FAST_STAGE_DEPTH 12   // tile dwords in flight per thread while staging (256 threads x 12 x 4 B = 12 KB per round trip)
#endif

namespace sd {

constexpr int kFastThreads = 256, kFastWaves = 4;
constexpr size_t kFastLdsSlack = 64;   // bytes requested beyond the worst-pad layout (part of every request since r2)

struct FastDiv { uint32_t d; uint64_t max_e; };   // a division by d of dividends 0 ... max_e

struct LdsFastTile {
  int xa = 0, sh = 0;                      // source column of tile column 0, and the zone's pad behind it (0 ... 15)
  int TPU = 0, TP = 0, TPW = 0;            // tile pitch in 16-byte units, bytes, dwords
  int NSR = 0, RPW = 0, QCAP = 0;          // rows a strip scores at most, score rows per wave, queue entries per wave
  uint32_t tile = 0, sc = 0, queue = 0;    // byte offsets of the three regions
  uint32_t tile0 = 0, sc0 = 0;             // byte offsets of zone pixel (0, 0) of the strip and of its score
  uint32_t bytes = 0;
  int zw = 0;

  constexpr LdsFastTile(int zx0, int zw_, int zh, int strip_rows, int edge) : LdsFastTile(zx0 - 3 + edge, zw_, zh, strip_rows) {}
  // the layout at the largest pad: TP, hence every region, is at its largest
  static constexpr LdsFastTile worst_pad(int zw_, int zh, int strip_rows) { return LdsFastTile(15, zw_, zh, strip_rows); }

  constexpr uint32_t queue_of(int wave) const { return queue + (uint32_t)(wave * QCAP * 2); }
  constexpr bool entries_fit16() const { return (int64_t)(NSR + 1) * TP <= 65536; }

  constexpr FastDiv div_zw() const { return {(uint32_t)zw, (uint64_t)NSR * zw - 1}; }
  constexpr FastDiv div_tp() const { return {(uint32_t)TP, (uint64_t)(NSR - 1) * TP + zw - 1}; }
  constexpr FastDiv div_tpu() const { return {(uint32_t)TPU, staged((uint64_t)TPU * (NSR + 6), kFastThreads * (FAST_STAGE_DEPTH / 4))}; }
  constexpr FastDiv div_tpw() const { return {(uint32_t)TPW, staged((uint64_t)TPW * (NSR + 6), kFastThreads * FAST_STAGE_DEPTH)}; }

 private:
  constexpr LdsFastTile(int xs, int zw_, int zh, int strip_rows)
      : xa(xs & ~15), sh(xs - (xs & ~15)), TPU((sh + zw_ + 6 + 15) >> 4), TP(TPU * 16), TPW(TPU * 4),
        NSR(strip_rows + 2 < zh ? strip_rows + 2 : zh), RPW((NSR + 3) >> 2), QCAP(RPW * zw_),
        tile(0), sc((uint32_t)(TP * (NSR + 6))), queue(sc + (uint32_t)(TP * (NSR + 2))),
        tile0(tile + (uint32_t)(3 * TP + 3 + sh)), sc0(sc + (uint32_t)(TP + 1)),
        bytes(queue + (uint32_t)(kFastWaves * QCAP * 2)), zw(zw_) {}
  // largest index a staging loop over n items in steps of `step` evaluates
  static constexpr uint64_t staged(uint64_t n, uint64_t step) { return (n + step - 1) / step * step - 1; }
};

// ---- the plan's strip search (orb_plan.cpp), in its own terms ----
constexpr size_t fast_up(size_t v, size_t a) { return (v + a - 1) / a * a; }
// r2 size of a strip of S rows: tile pitch up(zw + 9, 4), score pitch up(zw + 2, 4), S + 2 scored rows whatever the cell's height
constexpr size_t fast_r2_bytes(int zw, int S) {
  return fast_up((size_t)zw + 6 + 3, 4) * (S + 2 + 6) + fast_up((size_t)zw + 2, 4) * (S + 2 + 2) + 2 * kFastWaves * (size_t)((S + 2 + 3) / 4) * zw +
         kFastLdsSlack;
}
// phase C keeps one bit per 64-entry queue chunk in a 64-bit mask: a wave's queue holds at most 4096 entries
constexpr bool fast_queue_chunks_fit(int zw, int S) { return (size_t)((S + 2 + 3) / 4) * zw <= 4096; }
// a launch may ask for 64 KB without opting in, so a request may exceed a budget below that
constexpr size_t fast_request_limit(size_t budget_bytes) { return budget_bytes > 65536 ? budget_bytes : 65536; }

}  // namespace sd
