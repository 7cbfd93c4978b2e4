// ORB extraction on MI355X (gfx950): the hand-written HIP kernels and the pipeline that launches them (sd::orb_launch_pipeline).
// The sd_orb handle and the sd_orb_* C ABI are in orb_host.hip; orb_internal.h is what the two files share.
//
// Replaces SD_SLAM::ORBextractor (reference src/ORBextractor.cc).  Batched-frames-first:
// every kernel takes the frame index as its outermost grid dimension, so one launch covers
// all frames of a batch (and, for blur / selection / descriptors, all pyramid levels).
//
//   k_pyr_split      ComputePyramid: resize + copyMakeBorder   src/ORBextractor.cc:680-700 (one launch per level: aligned 4-pixel
//                    groups of every padded row, table-driven bilinear at REFLECT_101 column indices; border rows as second stores)
//   k_pyr_rows       same, for levels whose rows come in runs on consecutive source rows (scale 1.2): five consecutive rows per
//                    thread, each source row loaded and horizontally resized once
//   k_pyr_level      same, single generic pass    (exact-2x INTER_AREA levels, byte-unaligned inputs, tiny levels)
//   k_fast_cells     cv::FAST per grid cell        src/ORBextractor.cc:501-552 (FAST-9/16, score, cell-local 3x3 NMS)
//   k_select_*       quota loop + retainBest       src/ORBextractor.cc:554-605 (wave-parallel libstdc++ introselect replay)
//   k_blur           GaussianBlur 7x7 s=2          src/ORBextractor.cc:659-660 (8-bit fixed point, separable)
//   k_orient_desc    IC_Angle + steered rBRIEF     src/ORBextractor.cc:78-143, 608-618, 669-674
//   k_undistort      Frame::UndistortKeyPoints     src/Frame.cc:335-366
//
// Streams per handle: main (resize chain, selection, descriptors), fast (FAST of a level as soon as the level is
// complete), aux (blur); see orb_launch_pipeline / pipeline_body and DESIGN.md section 5.
// HBM layout (per frame): padded pyramid block (all levels, 19-px border, 64-B aligned rows),
// blurred block (same geometry), candidate keys (u32: response<<24 | y<<12 | x, per cell, raster
// order), selected keys per level, output keypoints (28 B) + descriptors (32 B).
// Integer / byte work limited by VALU issue and load latency: no MFMA anywhere
// (largest dense object is 7 taps).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "introselect.h"
#include "introselect_wave.h"
#include "orb_fast_lds.h"
#include "orb_internal.h"
#include "sd_sincosf.h"

namespace sd {

// ------------------------------------------------------------------------------------------
// device helpers
// ------------------------------------------------------------------------------------------
// Frame / block of this workgroup for a (blocks, frames) grid such that the workgroups of ONE frame run on ONE XCD: the dispatcher
// deals workgroups to the 8 XCDs round-robin in linear order (MI355X_MICROARCH.md, workgroup dispatch), every XCD has its own 4-MB L2,
// and the workgroups of a frame re-read each other's rows (resize: the two source rows of adjacent output rows; FAST / blur: tile
// halos; 128-B lines shared by neighbouring tiles).  Bijective for any grid size; a speed choice only.
#ifndef SD_XCD_REMAP
#define SD_XCD_REMAP 1
#endif
__device__ __forceinline__ void xcd_frame_block(unsigned& frame, unsigned& blk) {
#if SD_XCD_REMAP
  const unsigned nx = gridDim.x, total = nx * gridDim.y;
  const unsigned lin = blockIdx.y * nx + blockIdx.x;
  const unsigned q = total >> 3, r = total & 7u, xcd = lin & 7u;
  const unsigned logical = (xcd < r ? xcd * (q + 1u) : r * (q + 1u) + (xcd - r) * q) + (lin >> 3);
  frame = logical / nx;
  blk = logical - frame * nx;
#else
  frame = blockIdx.y;
  blk = blockIdx.x;
#endif
}

__device__ __forceinline__ int reflect101(int p, int len) {
  if ((unsigned)p < (unsigned)len) return p;
  if (len == 1) return 0;
  do {
    if (p < 0) p = -p;
    else p = 2 * len - 2 - p;
  } while ((unsigned)p >= (unsigned)len);
  return p;
}

// ------------------------------------------------------------------------------------------
// k_pyr_level: one pyramid level, written over its whole padded domain in a single pass.
// level 0 : copyMakeBorder(image, REFLECT_101)
// level l : resize(level l-1 -> l, INTER_LINEAR) then copyMakeBorder(REFLECT_101|ISOLATED);
//           a border pixel equals the resize result of its reflected interior pixel.
// Each thread produces 4 horizontally adjacent bytes (one u32 store, coalesced).
// ------------------------------------------------------------------------------------------
__device__ __forceinline__ uint32_t ld_u32_unaligned(const uint8_t* p) {
  uint32_t v;
  __builtin_memcpy(&v, p, 4);   // global memory runs in unaligned-access mode: one dword load
  return v;
}

// 16-byte window starting at the 4-byte-aligned address at or below p, as two 64-bit halves;
// *sh = p's offset inside the window (0..3).  Aligned dword loads only: byte-unaligned vector
// loads are legal on gfx950 but ran the bilinear level kernels at ~270 GB/s.
__device__ __forceinline__ void ld_window16(const uint8_t* p, unsigned long long* lo, unsigned long long* hi, int* sh) {
  const uintptr_t a = (uintptr_t)p;
  const uint32_t* q = (const uint32_t*)(a & ~(uintptr_t)3);
  *sh = (int)(a & 3);
  const uint32_t w0 = q[0], w1 = q[1], w2 = q[2], w3 = q[3];
  *lo = w0 | ((unsigned long long)w1 << 32);
  *hi = w2 | ((unsigned long long)w3 << 32);
}
// cv::resize INTER_LINEAR coefficients of destination index d (OpenCV 3.2):
// fx = (float)((d + 0.5) * scale - 0.5); s = floor(fx); fx -= s; alpha = saturate_cast<short>(w * 2048).
// Recomputed per pixel (a handful of IEEE ops, bit-identical to the host tables) so that the
// pixel loads do not wait behind a dependent table load.
__device__ __forceinline__ void resize_coef(int d, double scale, int sn, bool clamp, int* s_out, int* a0, int* a1) {
  float f = (float)((d + 0.5) * scale - 0.5);
  int s = (int)floorf(f);
  f -= (float)s;
  if (clamp) {
    if (s < 0) { f = 0.f; s = 0; }
    if (s >= sn - 1) { f = 0.f; s = sn - 1; }
  }
  *s_out = s;
  *a0 = (int)rintf((1.f - f) * 2048.f);
  *a1 = (int)rintf(f * 2048.f);
}

__device__ __forceinline__ int win_byte(unsigned long long lo, unsigned long long hi, int b) {   // b in 0..15
  return b < 8 ? (int)((lo >> (8 * b)) & 0xff) : (int)((hi >> (8 * (b - 8))) & 0xff);
}

// rows per thread (multi-row unrolling bought nothing and tripped a codegen problem in the byte packing).  The one-iteration
// loops of k_pyr_level stay: written without them the kernel compiles to other machine code (45 instead of 51 VGPRs, another
// instruction stream), and it serves the reference's default 5 x 2.0 pyramid as measured.
#define PYR_ROWS 1

__device__ __forceinline__ uint32_t pyr_px4(const LevelGeom& L, const LevelGeom& S, size_t pyr_frame_bytes, int level, int frame, int px,
                                            int py, const uint8_t* __restrict__ src0, int src_stride, size_t src_frame_stride,
                                            const uint8_t* __restrict__ pyr) {
  const int Y = reflect101(py - SD_EDGE, L.h);
  // fast path: the 4 outputs are interior pixels X0..X0+3 (no reflection, consecutive sources)
  const int X0 = px - SD_EDGE;
  const bool interior = X0 >= 0 && X0 + 3 < L.w;
  uint32_t packed = 0;
  if (level == 0) {
    const uint8_t* s = src0 + (size_t)frame * src_frame_stride + (size_t)Y * src_stride;
    if (interior && X0 >= 4 && X0 + 7 < L.w) {   // aligned window stays inside this source row
      const uintptr_t a = (uintptr_t)(s + X0);
      const uint32_t* q = (const uint32_t*)(a & ~(uintptr_t)3);
      const int sh = (int)(a & 3) * 8;
      const unsigned long long w = q[0] | ((unsigned long long)q[1] << 32);
      packed = (uint32_t)(w >> sh);
    } else if (interior) {
      packed = ld_u32_unaligned(s + X0);
    } else {
      uint32_t v[4];
#pragma unroll
      for (int k = 0; k < 4; k++) v[k] = s[reflect101(min(px + k, L.w + 2 * SD_EDGE - 1) - SD_EDGE, L.w)];   // 4 loads in flight
#pragma unroll
      for (int k = 0; k < 4; k++) packed |= (px + k < L.w + 2 * SD_EDGE ? v[k] : 0u) << (8 * k);
    }
  } else {
    const uint8_t* sb = pyr + (size_t)frame * pyr_frame_bytes + S.off + (size_t)SD_EDGE * S.pstride + SD_EDGE;
    if (L.area2x2) {
      const uint8_t* r0 = sb + (size_t)(2 * Y) * S.pstride;
      const uint8_t* r1 = r0 + S.pstride;
      if (interior) {
        const uint32_t a0 = ld_u32_unaligned(r0 + 2 * X0), a1 = ld_u32_unaligned(r0 + 2 * X0 + 4);
        const uint32_t b0 = ld_u32_unaligned(r1 + 2 * X0), b1 = ld_u32_unaligned(r1 + 2 * X0 + 4);
#pragma unroll
        for (int k = 0; k < 4; k++) {
          const uint32_t ta = k < 2 ? (a0 >> (16 * k)) : (a1 >> (16 * (k - 2)));
          const uint32_t tb = k < 2 ? (b0 >> (16 * k)) : (b1 >> (16 * (k - 2)));
          const uint32_t v = ((ta & 0xff) + ((ta >> 8) & 0xff) + (tb & 0xff) + ((tb >> 8) & 0xff) + 2) >> 2;
          packed |= v << (8 * k);
        }
      } else {
        uint32_t t[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {   // loads of the four pixels first (clamped column, result dropped beyond the padded row)
          const int X = reflect101(min(px + k, L.w + 2 * SD_EDGE - 1) - SD_EDGE, L.w);
          t[k] = r0[2 * X] + r0[2 * X + 1] + r1[2 * X] + r1[2 * X + 1];
        }
#pragma unroll
        for (int k = 0; k < 4; k++) packed |= (px + k < L.w + 2 * SD_EDGE ? (t[k] + 2) >> 2 : 0u) << (8 * k);
      }
    } else {
      int sy0, b0, b1;
      resize_coef(Y, L.scale_y, S.h, false, &sy0, &b0, &b1);
      int sy1 = sy0 + 1;
      sy0 = sy0 < 0 ? 0 : (sy0 < S.h ? sy0 : S.h - 1);
      sy1 = sy1 < 0 ? 0 : (sy1 < S.h ? sy1 : S.h - 1);
      const uint8_t* r0 = sb + (size_t)__mul24(sy0, S.pstride);
      const uint8_t* r1 = sb + (size_t)__mul24(sy1, S.pstride);
      bool done = false;
      if (interior) {
        // the sources of 4 consecutive outputs span <= 12 bytes for scale factors up to 2:
        // fetch each source row as three dwords and pick bytes out of the registers
        int sx[4], wa0[4], wa1[4];
#pragma unroll
        for (int k = 0; k < 4; k++) resize_coef(X0 + k, L.scale_x, S.w, true, &sx[k], &wa0[k], &wa1[k]);
        const int base = sx[0];
        if (sx[3] + 1 - base <= 11 && base + 15 < S.w + SD_EDGE) {   // 16-byte aligned window stays inside the padded row
          unsigned long long lo0, hi0, lo1, hi1;
          int sh0, sh1;
          ld_window16(r0 + base, &lo0, &hi0, &sh0);
          ld_window16(r1 + base, &lo1, &hi1, &sh1);   // sh1 == sh0 (row pitch is a multiple of 64)
#pragma unroll
          for (int k = 0; k < 4; k++) {
            const int o = sx[k] - base;            // 0..10
            const int o1 = (sx[k] + 1 < S.w ? sx[k] + 1 : S.w - 1) - base;
            const int p00 = win_byte(lo0, hi0, sh0 + o), p01 = win_byte(lo0, hi0, sh0 + o1);
            const int p10 = win_byte(lo1, hi1, sh1 + o), p11 = win_byte(lo1, hi1, sh1 + o1);
            const int a0 = wa0[k], a1 = wa1[k];
            // all factors fit 24 bits: v_mul_i32_i24 / v_mad_i32_i24 issue at full rate, v_mul_lo_u32 at a quarter
            const int h0 = __mul24(p00, a0) + __mul24(p01, a1);
            const int h1 = __mul24(p10, a0) + __mul24(p11, a1);
            const int ov = ((__mul24(b0, h0 >> 4) >> 16) + (__mul24(b1, h1 >> 4) >> 16) + 2) >> 2;
            packed |= (uint32_t)(ov < 0 ? 0 : (ov > 255 ? 255 : ov)) << (8 * k);
          }
          done = true;
        }
      }
      if (!done) {
        // border / edge pixels: the 4 x 4 source bytes are fetched first (columns beyond the padded row are clamped, their
        // result is dropped), so a thread has 16 loads in flight instead of four dependent rounds of four
        int p00[4], p01[4], p10[4], p11[4], a0[4], a1[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
          const int x = min(px + k, L.w + 2 * SD_EDGE - 1);
          const int X = reflect101(x - SD_EDGE, L.w);
          int sx;
          resize_coef(X, L.scale_x, S.w, true, &sx, &a0[k], &a1[k]);
          const int sx1 = sx + 1 < S.w ? sx + 1 : S.w - 1;
          p00[k] = r0[sx]; p01[k] = r0[sx1]; p10[k] = r1[sx]; p11[k] = r1[sx1];
        }
#pragma unroll
        for (int k = 0; k < 4; k++) {
          const int h0 = __mul24(p00[k], a0[k]) + __mul24(p01[k], a1[k]);
          const int h1 = __mul24(p10[k], a0[k]) + __mul24(p11[k], a1[k]);
          const int o = ((__mul24(b0, h0 >> 4) >> 16) + (__mul24(b1, h1 >> 4) >> 16) + 2) >> 2;
          const uint32_t v = px + k < L.w + 2 * SD_EDGE ? (uint32_t)(o < 0 ? 0 : (o > 255 ? 255 : o)) : 0u;
          packed |= v << (8 * k);
        }
      }
    }
  }
  return packed;
}

// L / S (this level, source level) travel by value in the kernel arguments: one less dependent
// load before the first pixel fetch.
__global__ __launch_bounds__(256) void k_pyr_level(const LevelGeom L, const LevelGeom S, size_t pyr_frame_bytes, int level,
                                                   const uint8_t* __restrict__ src0, int src_stride,
                                                   size_t src_frame_stride, uint8_t* __restrict__ pyr) {
  const int frame = blockIdx.z;
  const int px = (blockIdx.x * 64 + threadIdx.x) * 4;
  const int py0 = (blockIdx.y * 4 + threadIdx.y) * PYR_ROWS;
  if (px >= L.pstride || py0 >= L.prows) return;
  uint8_t* dstbase = pyr + (size_t)frame * pyr_frame_bytes + L.off;
  uint32_t out[PYR_ROWS];
#pragma unroll
  for (int r = 0; r < PYR_ROWS; r++) {
    const int py = min(py0 + r, L.prows - 1);   // clamped duplicates are computed but not stored
    out[r] = pyr_px4(L, S, pyr_frame_bytes, level, frame, px, py, src0, src_stride, src_frame_stride, pyr);
  }
#pragma unroll
  for (int r = 0; r < PYR_ROWS; r++)
    if (py0 + r < L.prows) *(uint32_t*)(dstbase + (size_t)(py0 + r) * L.pstride + px) = out[r];
}

// ------------------------------------------------------------------------------------------
// Split pyramid construction (the default path).  k_pyr_level above evaluates every padded pixel
// through one code path, so the waves at both ends of a row run the slow reflected-border branch
// as well as the interior one.  Here every thread owns an aligned 4-pixel group (padded columns 4 gi ... 4 gi + 3) of three rows:
// coefficient tables (the host's cv::resize tables) read at the REFLECT_101 column index of each pixel, one aligned 12-byte window
// per source row (the four sources of a group lie within 8 bytes whatever their order), v_perm_b32 gathers the 2 x 4 source bytes.
// (r1-r3 had a second role for the border columns and the interior pixels outside the aligned interior groups, on the generic
// per-byte path pyr_px4: a fifth of every launch's workgroups.)  Level 0 is the frame copied into the padded layout by the same kernel.
// ------------------------------------------------------------------------------------------
// PYR_RPT (orb_plan.h: the plan sizes the launch with it) rows per thread: rows Y, Y + ceil(h / 4), ... share the group's column data and give independent load chains (r1: 3 rows 130.8 k,
// 2 rows 130.4 k frames/s, 4 rows no better than 2; r3, with the per-group / per-row tables as the fixed cost of a thread: 4 rows and
// the descriptor patch on 8-byte loads 226.2 k vs 222.3 k with 3 rows; 4 / 5 / 6 rows 229.4 / 226.9 / 225.4 k, alternating runs)
// **r2**: the rows are PADDED rows (0 .. h + 37): a top / bottom border row is the resize of its REFLECT_101 interior row, computed
// here like any other row instead of being copied by a third kernel after the first two (k_pyr_rows, gone): ONE launch per level
// (k_pyr_split), 8 pyramid launches per step instead of 24.  r3: where the level is tall enough for single reflections the border
// rows are second stores of their source rows (`mirror`).
// r10: rows a quarter of the level apart share no source rows, so every output row loads and horizontally resizes both of its
// own.  The levels whose rows come in runs on consecutive source rows (every resized level of the 8 x 1.2 pyramid) have gone to
// k_pyr_rows below, which gives a thread five CONSECUTIVE rows on six source rows; PYR_RPT and this body remain for level 0 (the
// copy), for levels under 48 rows, and for scale factors whose runs are short (1.5: two rows).
__device__ __forceinline__ void pyr_resize_body(const LevelGeom& L, const LevelGeom& S, size_t pyr_frame_bytes, int level,
                                                const int32_t* __restrict__ coef, const uint8_t* __restrict__ src0, int src_stride,
                                                size_t src_frame_stride, uint8_t* __restrict__ pyr, int G, unsigned magicG, int Hh,
                                                int frame, unsigned e, int mirror) {
  const unsigned Y0 = __umulhi(e, magicG);        // e / G
  if (Y0 >= (unsigned)Hh) return;
  // r3: G counts the 4-pixel groups of the whole PADDED row (padded columns 4 gi ... 4 gi + 3, gi = 0 ... G - 1): the border columns and
  // the few interior pixels outside the aligned interior groups go through the same code at their REFLECT_101 column positions
  // (their four sources still lie within one 8-byte window, in any order) instead of a second role on the generic per-byte path,
  // which was a fifth of every launch's workgroups.  Everything that depends on the group alone -- window base, v_perm selectors,
  // coefficient pairs, the level-0 copy's source column and byte order -- comes from a host-built table (orb_plan.cpp group_table:
  // three aligned 16-byte loads), so the kernel does no reflection, minimum or selector arithmetic.
  const int gi = (int)(e - Y0 * (unsigned)G);
  const int X0 = 4 * gi - SD_EDGE;   // first pixel of the group; negative / beyond w - 1: border
  const int4* gt = (const int4*)(coef + L.cg) + 3 * gi;
  // wave-uniform base pointers + 32-bit per-lane offsets: loads and stores use the SGPR-base addressing form
  uint8_t* dstb = pyr + (size_t)frame * pyr_frame_bytes + L.off;
  const uint32_t dst_x = (uint32_t)(X0 + SD_EDGE);
  uint32_t packed[PYR_RPT];
  bool live[PYR_RPT];
  int Yr[PYR_RPT], PY[PYR_RPT];   // interior (source-side) row, padded (destination) row
#pragma unroll
  for (int r = 0; r < PYR_RPT; r++) {
    if (mirror) {   // interior rows only: the border rows are second stores of their REFLECT_101 source rows (below)
      Yr[r] = (int)Y0 + r * Hh;
      live[r] = Yr[r] < L.h;
      if (!live[r]) Yr[r] = (int)Y0;   // duplicate work, not stored
      PY[r] = Yr[r] + SD_EDGE;
    } else {
      PY[r] = (int)Y0 + r * Hh;
      live[r] = PY[r] < L.prows;
      if (!live[r]) PY[r] = (int)Y0;   // duplicate work, not stored
      Yr[r] = reflect101(PY[r] - SD_EDGE, L.h);
    }
  }
  if (level == 0) {
#pragma unroll
    for (int r = 0; r < PYR_RPT; r++) {
      // k_pyr_resize runs for level 0 only when base pointer and strides are 4-byte aligned (pipeline_body)
      const uint8_t* s = src0 + (size_t)frame * src_frame_stride;
      // (computed, not read from the group table: the copy is latency-bound and the table would be one more dependent round trip)
      int Xr[4];
#pragma unroll
      for (int k = 0; k < 4; k++) {
        if (L.w >= 64) {   // single reflection, branch-free (columns beyond the padded width, whose result is dropped, are clamped)
          int x = X0 + k;
          x = x < 0 ? -x : x;
          x = x >= L.w ? 2 * L.w - 2 - x : x;
          Xr[k] = max(x, 0);
        } else {
          Xr[k] = reflect101(X0 + k, L.w);
        }
      }
      const int Xmin = min(min(Xr[0], Xr[1]), min(Xr[2], Xr[3]));   // the four sources are Xmin ... Xmin + 3 in some order
      const uint32_t sel = (uint32_t)(Xr[0] - Xmin) | (uint32_t)(Xr[1] - Xmin) << 8 | (uint32_t)(Xr[2] - Xmin) << 16 | (uint32_t)(Xr[3] - Xmin) << 24;
      const uint32_t o = (uint32_t)(__mul24(Yr[r], src_stride) + Xmin);
      const uint32_t* q = (const uint32_t*)(s + (o & ~3u));
      // (the second dword is not fetched where it would start beyond the row's last pixel: nothing in it is selected, and the
      // last row of the last frame has nothing behind it)
      const uint32_t last = (uint32_t)(__mul24(Yr[r], src_stride) + L.w - 1);
      const uint32_t q1 = q[((o & 3u) != 0u && (o & ~3u) + 4u <= last) ? 1 : 0];
      packed[r] = __builtin_amdgcn_perm(0u, __builtin_amdgcn_alignbyte(q1, q[0], o & 3u), sel);
    }
  } else {
    const int4* rt = (const int4*)(coef + L.cr);   // per interior row: byte offsets of its two source rows, vertical coefficient pair
    const int4 t0 = gt[0], t1 = gt[1], t2 = gt[2];
    const int base = t0.x;
    // v_perm selector per output pixel: {left source byte, 0, right source byte, 0} of the row's 8-byte window = the two
    // taps as a u16 pair, which v_dot2_u32_u16 multiplies with the packed coefficient pair ab[k] in one instruction
    typedef unsigned short us2 __attribute__((ext_vector_type(2)));
    const uint32_t selP[4] = {(uint32_t)t0.y, (uint32_t)t0.z, (uint32_t)t0.w, (uint32_t)t1.x};
    const uint32_t ab[4] = {(uint32_t)t1.y, (uint32_t)t1.z, (uint32_t)t1.w, (uint32_t)t2.x};
    const uint8_t* sb = pyr + (size_t)frame * pyr_frame_bytes + S.off;   // 64-byte aligned (level offsets and row pitches are)
    uint32_t u[PYR_RPT][3], v[PYR_RPT][3], bbv[PYR_RPT];
    unsigned shv[PYR_RPT];
#pragma unroll
    for (int r = 0; r < PYR_RPT; r++) {   // all loads of both rows first
      const int4 tr = rt[Yr[r]];
      bbv[r] = (uint32_t)tr.z;
      const uint32_t a0 = (uint32_t)(tr.x + base), a1 = (uint32_t)(tr.y + base);
      shv[r] = a0 & 3u;   // same for both source rows: the row pitch is a multiple of 64
      const uint32_t* q0 = (const uint32_t*)(sb + (a0 & ~3u));
      const uint32_t* q1 = (const uint32_t*)(sb + (a1 & ~3u));
#pragma unroll
      for (int k = 0; k < 3; k++) {
        u[r][k] = q0[k];
        v[r][k] = q1[k];
      }
    }
#pragma unroll
    for (int r = 0; r < PYR_RPT; r++) {
      const int b0 = (int)(bbv[r] & 0xffff), b1 = (int)(bbv[r] >> 16);
      const unsigned sh = shv[r];
      // 8 source bytes starting at sx[0], per row
      const uint32_t r0lo = __builtin_amdgcn_alignbyte(u[r][1], u[r][0], sh), r0hi = __builtin_amdgcn_alignbyte(u[r][2], u[r][1], sh);
      const uint32_t r1lo = __builtin_amdgcn_alignbyte(v[r][1], v[r][0], sh), r1hi = __builtin_amdgcn_alignbyte(v[r][2], v[r][1], sh);
      uint32_t pk = 0;
#pragma unroll
      for (int k = 0; k < 4; k++) {
        const us2 w = __builtin_bit_cast(us2, ab[k]);
        const int h0 = (int)__builtin_amdgcn_udot2(__builtin_bit_cast(us2, __builtin_amdgcn_perm(r0hi, r0lo, selP[k])), w, 0u, false);
        const int h1 = (int)__builtin_amdgcn_udot2(__builtin_bit_cast(us2, __builtin_amdgcn_perm(r1hi, r1lo, selP[k])), w, 0u, false);
        // (b * (h >> 4)) >> 16 == mulhi(b << 12, h & ~15): one 32-bit multiply per source row (b <= 2048, h < 2^20)
        // no saturation needed: a0 + a1 = b0 + b1 = 2048, so h <= 255 * 2048 and the sum below is at most (2048 * 32640 >> 16) + 2 = 1022
        const uint32_t ov = (__umulhi((uint32_t)b0 << 12, (uint32_t)h0 & ~15u) + __umulhi((uint32_t)b1 << 12, (uint32_t)h1 & ~15u) + 2u) >> 2;
        pk |= ov << (8 * k);
      }
      packed[r] = pk;
    }
  }
  // r3: the top / bottom REFLECT_101 border rows are COPIES of interior rows of the same level (copyMakeBorder after resize,
  // src/ORBextractor.cc:693-696): padded row 19 - Y holds row Y (1 <= Y <= 19), padded row 2 h + 17 - Y holds row Y
  // (h - 20 <= Y <= h - 2).  With `mirror` a thread's rows are interior rows and the thread that has just computed a pixel group
  // of such a row stores it a second time, instead of 38 more rows of full resize work per level (9 % of level 1, 22 % of level 7).
  // (The same for the border COLUMNS -- byte-reversed second stores by the threads at both ends of a row -- was built and lost:
  // nearly every wave holds a row end, and its 30-40 extra partial-lane store instructions cost more than the edge workgroups.)
  // columns beyond the padded width (the last group of a row when w + 38 is not a multiple of 4) stay zero
  const int nvalid = L.w + 2 * SD_EDGE - (int)dst_x;
  const uint32_t keep = nvalid >= 4 ? 0xffffffffu : (1u << (8 * nvalid)) - 1u;
#pragma unroll
  for (int r = 0; r < PYR_RPT; r++) {
    if (!live[r]) continue;
    packed[r] &= keep;
    *(uint32_t*)(dstb + (dst_x + (uint32_t)__mul24(PY[r], L.pstride))) = packed[r];
    if (mirror) {
      const int Yi = Yr[r];
      const int prow2 = Yi >= 1 && Yi <= SD_EDGE ? SD_EDGE - Yi : (Yi >= L.h - 20 && Yi <= L.h - 2 ? 2 * L.h + 17 - Yi : -1);
      if (prow2 >= 0) *(uint32_t*)(dstb + (dst_x + (uint32_t)__mul24(prow2, L.pstride))) = packed[r];
    }
  }
}

// one launch per level
__global__ __launch_bounds__(256) void k_pyr_split(const LevelGeom L, const LevelGeom S, size_t pyr_frame_bytes, int level,
                                                   const int32_t* __restrict__ coef, const uint8_t* __restrict__ src0, int src_stride,
                                                   size_t src_frame_stride, uint8_t* __restrict__ pyr, int G, unsigned magicG, int Hh,
                                                   int mirror) {
  unsigned uframe, bx;
  xcd_frame_block(uframe, bx);
  pyr_resize_body(L, S, pyr_frame_bytes, level, coef, src0, src_stride, src_frame_stride, pyr, G, magicG, Hh, (int)uframe,
                  bx * 256 + threadIdx.x, mirror);
}

// k_pyr_rows: the resize of a level >= 1 whose rows come in runs that share source rows (orb_plan.cpp row_blocks; scale 1.2).
// k_pyr_split gives a thread four rows a quarter of the level apart, so every output row loads and horizontally resizes both of
// its source rows.  Here a thread owns one 4-pixel group of a row BLOCK: up to SD_PYR_BLOCK_ROWS consecutive interior rows whose
// first source rows are consecutive too, so row r combines horizontal results r and r + 1 of the block's
// SD_PYR_BLOCK_ROWS + 1 source rows -- which two never depends on the block, so nothing is selected per lane and (block, group)
// pairs are dealt flat over the lanes like k_pyr_split's (row, group) pairs.  Per output row 1.2 source rows (3.6 dword loads,
// 1.2 horizontal passes) instead of 2 (6 loads, 2 passes); the integer operations per output pixel are k_pyr_split's.
// A block shorter than SD_PYR_BLOCK_ROWS computes its missing rows and does not store them; source rows are clamped to the
// source level's last interior row (as the per-row table of k_pyr_split clamps them), never branched around.
__global__ __launch_bounds__(256) void k_pyr_rows(const LevelGeom L, const LevelGeom S, size_t pyr_frame_bytes,
                                                  const int32_t* __restrict__ coef, uint8_t* __restrict__ pyr, int G, unsigned magicG) {
  constexpr int R = SD_PYR_BLOCK_ROWS;
  unsigned uframe, bx;
  xcd_frame_block(uframe, bx);
  const unsigned e = bx * 256 + threadIdx.x;
  const unsigned bi = __umulhi(e, magicG);        // e / G
  if (bi >= (unsigned)L.nblk) return;
  const int gi = (int)(e - bi * (unsigned)G);
  const int4* gt = (const int4*)(coef + L.cg) + 3 * gi;
  const int4* bt = (const int4*)(coef + L.cb) + 2 * bi;
  const int4 t0 = gt[0], t1 = gt[1], t2 = gt[2];
  const int4 k0 = bt[0], k1 = bt[1];   // {y0, n | border << 8, sy0, bb[0]}, {bb[1 ... 4]}
  typedef unsigned short us2 __attribute__((ext_vector_type(2)));
  const uint32_t selP[4] = {(uint32_t)t0.y, (uint32_t)t0.z, (uint32_t)t0.w, (uint32_t)t1.x};
  const uint32_t ab[4] = {(uint32_t)t1.y, (uint32_t)t1.z, (uint32_t)t1.w, (uint32_t)t2.x};
  const uint32_t bb[R] = {(uint32_t)k0.w, (uint32_t)k1.x, (uint32_t)k1.y, (uint32_t)k1.z, (uint32_t)k1.w};
  const int y0 = k0.x, n = k0.y & 0xff, sy0 = k0.z;
  const uint8_t* sb = pyr + (size_t)uframe * pyr_frame_bytes + S.off;   // 64-byte aligned (level offsets and row pitches are)
  uint8_t* dstb = pyr + (size_t)uframe * pyr_frame_bytes + L.off;
  // byte offset of the group's first source column in interior row 0 of the source level; the row pitch is a multiple of 64, so
  // the misalignment of the 12-byte window is the same in every source row
  const uint32_t c0 = (uint32_t)(SD_EDGE * S.pstride + SD_EDGE + t0.x);
  const unsigned sh = c0 & 3u;
  uint32_t u[R + 1][3];
#pragma unroll
  for (int j = 0; j <= R; j++) {   // all loads first
    const uint32_t* q = (const uint32_t*)(sb + ((c0 & ~3u) + (uint32_t)__mul24(min(sy0 + j, S.h - 1), S.pstride)));
#pragma unroll
    for (int k = 0; k < 3; k++) u[j][k] = q[k];
  }
  uint32_t hz[R + 1][4];   // horizontal pass, once per source row (with the & ~15 of the vertical multiply)
#pragma unroll
  for (int j = 0; j <= R; j++) {
    const uint32_t lo = __builtin_amdgcn_alignbyte(u[j][1], u[j][0], sh), hi = __builtin_amdgcn_alignbyte(u[j][2], u[j][1], sh);
#pragma unroll
    for (int k = 0; k < 4; k++)
      hz[j][k] = __builtin_amdgcn_udot2(__builtin_bit_cast(us2, __builtin_amdgcn_perm(hi, lo, selP[k])), __builtin_bit_cast(us2, ab[k]), 0u, false) & ~15u;
  }
  const uint32_t dst_x = 4u * (uint32_t)gi;
  const int nvalid = L.w + 2 * SD_EDGE - (int)dst_x;   // columns beyond the padded width (last group of a row) stay zero
  const uint32_t keep = nvalid >= 4 ? 0xffffffffu : (1u << (8 * nvalid)) - 1u;
  uint32_t packed[R];
#pragma unroll
  for (int r = 0; r < R; r++) {
    const uint32_t b0 = (bb[r] & 0xffffu) << 12, b1 = bb[r] >> 16 << 12;
    uint32_t pk = 0;
#pragma unroll
    for (int k = 0; k < 4; k++)   // (b * (h >> 4)) >> 16 == mulhi(b << 12, h & ~15); no saturation needed (k_pyr_split)
      pk |= ((__umulhi(b0, hz[r][k]) + __umulhi(b1, hz[r + 1][k]) + 2u) >> 2) << (8 * k);
    packed[r] = pk & keep;
  }
#pragma unroll
  for (int r = 0; r < R; r++)
    if (r < n) *(uint32_t*)(dstb + (dst_x + (uint32_t)__mul24(y0 + r + SD_EDGE, L.pstride))) = packed[r];
  if (k0.y >> 8) {   // the block holds rows that are border rows as well (k_pyr_split's `mirror` second stores)
#pragma unroll
    for (int r = 0; r < R; r++) {
      const int Yi = y0 + r;
      const int prow2 = Yi >= 1 && Yi <= SD_EDGE ? SD_EDGE - Yi : (Yi >= L.h - 20 && Yi <= L.h - 2 ? 2 * L.h + 17 - Yi : -1);
      if (r < n && prow2 >= 0) *(uint32_t*)(dstb + (dst_x + (uint32_t)__mul24(prow2, L.pstride))) = packed[r];
    }
  }
}

// ------------------------------------------------------------------------------------------
// k_fast_cells: one workgroup per (grid cell, frame).  cv::FAST(cellImage, kps, th, true):
// corner test (>= 9 contiguous ring pixels brighter than v+t or darker than v-t), score =
// max over the 16 nine-arcs of min |v - p| minus 1, strict-greater 3x3 NMS in which pixels
// outside the cell's detection zone count as score 0, survivors emitted in
// raster order (the order cv::FAST produces and retainBest's tie-breaking depends on).
// The cell (+3 px ring halo) is staged once through LDS in aligned 4-byte words; scores live in
// a byte map in LDS; ordered emission uses wave ballots over wave-contiguous pixel ranges.
// ------------------------------------------------------------------------------------------
typedef unsigned short fu16;
__device__ __forceinline__ fu16 fmin16(fu16 a, fu16 b) { return a < b ? a : b; }
__device__ __forceinline__ fu16 fmax16(fu16 a, fu16 b) { return a > b ? a : b; }

// Corner test and cornerScore in one: with A = min over the 16 nine-arcs of max(p) and
// B = max over the arcs of min(p), a 9-arc darker than v - th exists iff v - A > th, a brighter one iff
// B - v > th, and cornerScore = max(v - A, B - v) - 1 (cv's cornerScore<16>: the max over the 16 nine-arcs of min(d) and of
// min(-d) of the ring differences d = v - p, minus 1; min / max of d over an arc are v - max(p) / v - min(p)).  The ring is the
// 16 offsets (dx, dy) clockwise from (0, 3).  Sliding 9-windows on the ring
// are built from 3-windows: 2 x (16 + 16 + 8) three-input min / max.  The pixel is a corner iff score >= th.
// r4: TWO pixels at once (ca: low 16-bit half, cb: high half), every min / max a gfx950 v_pk_minimum3_f16 /
// v_pk_maximum3_f16 (4.16 cycles at 8 waves per SIMD, the rate of v_max3_i32: profiles/r04_valu_microbench_pk3.json), so the
// 80 min / max per pixel become 80 per pair.  The ring bytes go into the halves as they are, i.e. as f16 bit patterns 0..255:
// zero and subnormals, exact and ordered like the integers only because the code object keeps f16 denormals
// (.amdhsa_float_denorm_mode_16_64 3, the compiler default, loaded into MODE from the kernel descriptor at every launch; no
// flag of the build turns on denormal flushing).  A and B come back out of the halves as the same integers.  The halves are
// filled by ds_read_u8 + v_perm: the compiler does not use ds_read_u8_d16_hi for a code object that may run with SRAM ECC on.
typedef _Float16 fh2 __attribute__((ext_vector_type(2)));
typedef unsigned short fu2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ fh2 hmax3(fh2 a, fh2 b, fh2 c) { return __builtin_elementwise_maximum(__builtin_elementwise_maximum(a, b), c); }
__device__ __forceinline__ fh2 hmin3(fh2 a, fh2 b, fh2 c) { return __builtin_elementwise_minimum(__builtin_elementwise_minimum(a, b), c); }
__device__ __forceinline__ fh2 ring_pair(const uint8_t* __restrict__ ca, const uint8_t* __restrict__ cb, int o) {
  const fu2 r = {ca[o], cb[o]};
  return __builtin_bit_cast(fh2, r);
}
__device__ __forceinline__ void fast_ring_score2(const uint8_t* __restrict__ ca, const uint8_t* __restrict__ cb, int tp, int& sa, int& sb) {
  fh2 p[16];
  const int va = ca[0], vb = cb[0];
  p[0] = ring_pair(ca, cb, 3 * tp); p[1] = ring_pair(ca, cb, 3 * tp + 1); p[2] = ring_pair(ca, cb, 2 * tp + 2); p[3] = ring_pair(ca, cb, tp + 3);
  p[4] = ring_pair(ca, cb, 3); p[5] = ring_pair(ca, cb, -tp + 3); p[6] = ring_pair(ca, cb, -2 * tp + 2); p[7] = ring_pair(ca, cb, -3 * tp + 1);
  p[8] = ring_pair(ca, cb, -3 * tp); p[9] = ring_pair(ca, cb, -3 * tp - 1); p[10] = ring_pair(ca, cb, -2 * tp - 2); p[11] = ring_pair(ca, cb, -tp - 3);
  p[12] = ring_pair(ca, cb, -3); p[13] = ring_pair(ca, cb, tp - 3); p[14] = ring_pair(ca, cb, 2 * tp - 2); p[15] = ring_pair(ca, cb, 3 * tp - 1);
  fh2 x3[16], n3[16];
#pragma unroll
  for (int k = 0; k < 16; k++) {
    x3[k] = hmax3(p[k], p[(k + 1) & 15], p[(k + 2) & 15]);
    n3[k] = hmin3(p[k], p[(k + 1) & 15], p[(k + 2) & 15]);
  }
  fh2 x9[16], n9[16];
#pragma unroll
  for (int k = 0; k < 16; k++) {
    x9[k] = hmax3(x3[k], x3[(k + 3) & 15], x3[(k + 6) & 15]);
    n9[k] = hmin3(n3[k], n3[(k + 3) & 15], n3[(k + 6) & 15]);
  }
  fh2 A = hmin3(x9[0], x9[1], x9[2]), B = hmax3(n9[0], n9[1], n9[2]);   // 8 three-input steps each over the 16 windows
#pragma unroll
  for (int k = 3; k < 15; k += 2) {
    A = hmin3(A, x9[k], x9[k + 1]);
    B = hmax3(B, n9[k], n9[k + 1]);
  }
  A = __builtin_elementwise_minimum(A, x9[15]);
  B = __builtin_elementwise_maximum(B, n9[15]);
  const fu2 Au = __builtin_bit_cast(fu2, A), Bu = __builtin_bit_cast(fu2, B);
  sa = max(va - (int)Au.x, (int)Bu.x - va) - 1;
  sb = max(vb - (int)Au.y, (int)Bu.y - vb) - 1;
}

#ifdef SD_PNP_PROF   // stage timers of k_fast_cells (tools/prof_select.py --fast): cycles of thread 0 per phase
// one record per workgroup, plain stores (hot-address atomics from 150 k workgroups back up the memory pipeline the tile
// loads go through and inflate the very phase being measured); summed on the host
#define FPROF_FRAMES 256
#define FPROF_CELLS 192
__device__ unsigned long long g_fast_prof_wg[(size_t)FPROF_FRAMES * FPROF_CELLS * 8];
// per-workgroup sums in LDS, one global atomic per phase at the end of the kernel: an atomic per phase and strip would sit in
// vmcnt and be waited for by the next tile load (the first version of these timers charged that wait to "stage")
#define FPROF_DECL                                   \
  __shared__ unsigned long long s_fprof[8];          \
  if (threadIdx.x < 8) s_fprof[threadIdx.x] = 0;     \
  long long _pt = clock64()
#define FPROF(i)                                                                 \
  do {                                                                           \
    long long _n = clock64();                                                    \
    if (threadIdx.x == 0) s_fprof[i] += (unsigned long long)(_n - _pt);          \
    _pt = _n;                                                                    \
  } while (0)
#define FPROF_FLUSH                                                                                                   \
  do {                                                                                                                \
    if (threadIdx.x == 0 && frame < FPROF_FRAMES && cell < FPROF_CELLS)                                          \
      for (int _i = 0; _i < 8; _i++) g_fast_prof_wg[((size_t)frame * FPROF_CELLS + cell) * 8 + _i] = s_fprof[_i]; \
  } while (0)
#else
#define FPROF_DECL
#define FPROF(i)
#define FPROF_FLUSH
#endif

// Structure of one strip (a cell is one strip unless it is too large for LDS):
//   A. every wave owns a contiguous band of rows; per 64-px row segment a 4-read compass test
//      (a 9-arc always contains two ADJACENT compass points of the same polarity) rejects most
//      pixels; survivors are appended, in raster order, to the wave's LDS queue (ballot prefix);
//   B. the queue is processed densely (all lanes busy): one pass computes cornerScore from sliding
//      min / max windows on the ring (fast_ring_score2, two pixels per lane); score >= th is the corner test; corners are
//      re-compacted in place (still raster order) and their scores go to the LDS score map;
//   C. after a block barrier, NMS on the queued corners against the LDS score map, then ordered
//      emission (wave bands are contiguous in raster order, so per-wave counts give offsets).
// (FAST_STAGE_DEPTH, the tile dwords in flight per thread while staging, is orb_fast_lds.h's: the staging loops' index range depends on it)
typedef uint32_t fast_u4 __attribute__((ext_vector_type(4)));   // one 16-byte staging unit (global_load_dwordx4 / ds_write_b128)

// 8 waves per SIMD: the kernel needed 65 VGPRs, one over the 64-register step; held to 64 it gains a resident wave per SIMD
// and the whole extraction 5 % (169 k -> 177 k frames/s ORB-only)
// Everything the workgroup needs besides its CellGeom arrives as kernel arguments (no dependent cell -> level -> plan loads):
// img0 / frame_stride / src / edge describe the levels' rows -- the padded pyramid (edge = SD_EDGE), or, for level 0, the
// caller's frames themselves (edge = 0; 4-byte aligned base and strides): FAST only touches interior pixels (the zones
// start SD_EDGE - 3 px inside), so level 0 need not wait for the padded copy of the frame.  wide16: base, row pitch and frame
// stride are all 16-byte aligned (always so for the pyramid), the tile is staged in 16-byte units.  One launch covers the cells
// cell0 .. cell0 + gridDim.x - 1, of one level or of several consecutive ones (the small levels go together: each of their
// launches was mostly ramp-up and tail).
struct FastSrc {   // where the rows of a level start inside a frame's block, and their pitch (by value: one launch may span levels)
  uint32_t off[SD_MAX_LEVELS];
  int pstride[SD_MAX_LEVELS];
};

__global__ __launch_bounds__(256, 8) void k_fast_cells(const CellGeom* __restrict__ cells, const uint8_t* __restrict__ img0,
                                                    size_t frame_stride, const FastSrc src, int edge, uint32_t* __restrict__ cand,
                                                    uint32_t cand_per_frame, int32_t* __restrict__ cell_count, int ncells_total,
                                                    int cell0, int th, int wide16) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  __shared__ int wcnt[4];
  unsigned uframe, ucell;
  xcd_frame_block(uframe, ucell);
  const int cell = (int)ucell + cell0;   // launched per level: the cells of a level are contiguous
  const CellGeom C = cells[cell];
  const int frame = (int)uframe;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);   // provably uniform: the band limits and loop counters derived from it stay scalar
  if (C.zw <= 0 || C.zh <= 0) {
    if (tid == 0) cell_count[(size_t)frame * ncells_total + cell] = 0;
    return;
  }
  const uint8_t* img = img0 + (size_t)frame * frame_stride + src.off[C.level];
  const int pstride = src.pstride[C.level];
  uint32_t* out = cand + (size_t)frame * cand_per_frame + C.cand_off;
  const int zw = C.zw, zh = C.zh, S = C.strip_rows;
  // the tile, the score map and the wave queues, and the four flat-index divisions with their checked ranges: orb_fast_lds.h
  const LdsFastTile T(C.zx0, zw, zh, S, edge);
  const int xa = T.xa, TPU = T.TPU, TP = T.TP;
  uint8_t* tile = smem + T.tile;
  uint8_t* sc = smem + T.sc;
  uint16_t* queue = (uint16_t*)(smem + T.queue_of(wave));
  // the wave's queue as a scalar byte offset into the dynamic LDS (phase A stores through SGPR base + lane offset)
  const uint32_t qbase = (uint32_t)__builtin_amdgcn_readfirstlane((int)T.queue_of(wave));
  const unsigned magic = fastdiv_magic((unsigned)zw);    // flat pixel index / zw
  const unsigned magic_tp = fastdiv_magic((unsigned)TP);   // queue entry / TP
  const uint8_t* tile0 = smem + T.tile0;   // zone pixel (0, 0) of the strip
  uint8_t* sc0 = smem + T.sc0;             // its score
  const unsigned long long lt = lanemask_lt((int)__lane_id());
  int total = 0;
  FPROF_DECL;

  for (int r0 = 0; r0 < zh; r0 += S) {
    const int r1 = min(r0 + S, zh);
    const int sr0 = max(r0 - 1, 0), sr1 = min(r1 + 1, zh);   // zone rows whose scores are needed
    const int nsr = sr1 - sr0;
    const int npr = nsr + 6;
    // ---- stage pixels and clear the score map.  The tile's 16-byte units are numbered row-major and dealt to the 256 threads
    // FAST_STAGE_DEPTH / 4 at a time, all loads before the first LDS store: a tile of up to 12 KB is ONE global round trip (the
    // strip's life is mostly this wait: with 8 rows per wave and batch it was three).  Row and column are computed once per unit.
    // Why the last unit of a row never leaves the source row's allocation: a tile row ends at up(xe, 16), xe = zx0 + zw + 3 +
    // edge the first column the ring does not need, and zx0 + zw <= w - SD_EDGE for every cell the plan evaluates.  Pyramid
    // (edge = SD_EDGE): xe <= w + 3 <= w + 2 * SD_EDGE <= pstride, and pstride is a multiple of 64, hence up(xe, 16) <= pstride.
    // Caller frames (edge = 0): xe <= w - 16, hence up(xe, 16) < w <= stride, whatever the stride's alignment (and the last
    // row staged is SD_EDGE - 3 rows above the frame's last, so even a frame allocated without its last row's padding is safe).
    {
      const uint8_t* g = img + (size_t)(C.zy0 + sr0 - 3 + edge) * pstride + xa;
      int t0 = tid;
      asm volatile("" : "+v"(t0));   // opaque per strip: otherwise the row / column of every slot is hoisted out of the strip loop and spilled
      if (wide16) {   // wave-uniform (kernel argument)
        const int nu = __mul24(TPU, npr);
        const unsigned magic_tpu = fastdiv_magic_odd((unsigned)TPU);   // the odd recipe: TPU may be 1
        for (int i0 = t0; i0 < nu; i0 += 256 * (FAST_STAGE_DEPTH / 4)) {
          fast_u4 v[FAST_STAGE_DEPTH / 4];
#pragma unroll
          for (int j = 0; j < FAST_STAGE_DEPTH / 4; j++) {
            const int i = i0 + 256 * j;
            const int row = (int)__umulhi(2u * (unsigned)i + 1u, magic_tpu), uc = i - __mul24(row, TPU);
            v[j] = i < nu ? *(const fast_u4*)(g + (uint32_t)(__mul24(row, pstride) + uc * 16)) : fast_u4{0u, 0u, 0u, 0u};
          }
#pragma unroll
          for (int j = 0; j < FAST_STAGE_DEPTH / 4; j++) {
            const int i = i0 + 256 * j;
            if (i < nu) ((fast_u4*)tile)[i] = v[j];
          }
        }
      } else {   // caller frames that are only 4-byte aligned: the same tile, one dword at a time
        const int TPW = T.TPW;
        const int ndw = __mul24(TPW, npr);
        const unsigned magic_tpw = fastdiv_magic((unsigned)TPW);   // tile dword index / TPW
        for (int i0 = t0; i0 < ndw; i0 += 256 * FAST_STAGE_DEPTH) {
          uint32_t v[FAST_STAGE_DEPTH];
#pragma unroll
          for (int j = 0; j < FAST_STAGE_DEPTH; j++) {
            const int i = i0 + 256 * j;
            const int row = (int)__umulhi((unsigned)i, magic_tpw), wc = i - __mul24(row, TPW);
            v[j] = i < ndw ? *(const uint32_t*)(g + (uint32_t)(__mul24(row, pstride) + wc * 4)) : 0u;
          }
#pragma unroll
          for (int j = 0; j < FAST_STAGE_DEPTH; j++) {
            const int i = i0 + 256 * j;
            if (i < ndw) ((uint32_t*)tile)[i] = v[j];
          }
        }
      }
      FPROF(7);   // kernel / strip start -> this wave's tile words are in LDS
      const int nsc = __mul24(nsr + 2, TPU);
      for (int i = tid; i < nsc; i += 256) ((fast_u4*)sc)[i] = fast_u4{0u, 0u, 0u, 0u};
    }
    __syncthreads();
    FPROF(0);
    // ---- A: compass quick test, ordered queue per wave
    const int rpw = (nsr + 3) >> 2;
    const int y_lo = min(wave * rpw, nsr), y_hi = min(y_lo + rpw, nsr);
    int qn = 0;
    // r3: the wave's band of rows is walked as ONE flat range of pixel indices i = y * zw + x, 64 at a time, instead of row by
    // row: zones are 47...121 pixels wide, so row-wise chunks ran at 57-98 % lane use (74 % on average: a third more chunks, and
    // this phase is bound by LDS-instruction issue as much as by the vector ALU).  Costs one multiply-high and one multiply-add per
    // chunk (row = i / zw by magic number, tile offset = i + row * (TP - zw)); r5: the queue entry is that tile offset, y * TP + x,
    // monotone in i (raster order is unchanged): phases B and C address ring and score with it and never take it apart.
    {
      const int i_lo = __mul24(y_lo, zw), i_hi = __mul24(y_hi, zw);
      const int pad = TP - zw;
#ifdef FAST_SKIP_A
      for (int i0 = i_hi; i0 < i_hi; i0 += 64) {
#else
      for (int i0 = i_lo; i0 < i_hi; i0 += 64) {
#endif
        // straight-line code on 16-bit min / max.  The lanes beyond the band read a clamped position and are masked out
        // of the ballot on the scalar unit; with D = max(min(p0, p8), min(p4, p12)) and Bt = min(max(p0, p8), max(p4, p12))
        // the compass condition ((k0 | k8) & (k4 | k12)) | ((b0 | b8) & (b4 | b12)), k = p < v - th, b = p > v + th, is
        // max(v - D, Bt - v) > th: 9 full-rate 16-bit instructions and ONE compare.
        const int i = min(i0 + lane, i_hi - 1);
        const int y = (int)__umulhi((unsigned)i, magic);
        const int ofs = i + __mul24(y, pad);
        const uint8_t* c = tile0 + ofs;
        const fu16 v = c[0], p0 = c[3 * TP], p4 = c[3], p8 = c[-3 * TP], p12 = c[-3];
        const fu16 D = fmax16(fmin16(p0, p8), fmin16(p4, p12));
        const fu16 Bt = fmin16(fmax16(p0, p8), fmax16(p4, p12));
        const short da = (short)(v - D), db = (short)(Bt - v);
        bool pass = (da > db ? da : db) > (short)th;
        if (i_hi - i0 < 64) pass = pass && (i0 + lane < i_hi);   // wave-uniform branch: only the band's last chunk pays this compare
        const unsigned long long m = __builtin_amdgcn_ballot_w64(pass);
        const int rank = (int)__builtin_amdgcn_mbcnt_hi((unsigned)(m >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)m, 0u));
        if (pass) *(uint16_t*)(smem + (qbase + 2u * (uint32_t)(qn + rank))) = (uint16_t)ofs;
        qn += __popcll(m);
      }
    }
    FPROF(1);
#ifdef FAST_SKIP_B   // instruction-budget experiments only (tools/fast_budget.sh): results are wrong by design
    qn = 0;
#endif
    // ---- B: ring test + score of the queued pixels in one pass (dense); corners re-compacted in place.  r4: 128 entries per
    // chunk, a pair per lane (entry e0 + lane in the low halves, e0 + 64 + lane in the high halves: fast_ring_score2).  A lane
    // whose high entry is past the queue's end scores its low pixel twice and drops the second result.  Corners of the low
    // halves are compacted first, then those of the high halves: raster order.  All reads of a chunk precede its writes, which
    // land below e0 + 128 (cn <= e0).
    int cn = 0;
    for (int e0 = 0; e0 < qn; e0 += 128) {
      const int ea = e0 + lane, eb = ea + 64;
      bool corner_a = false, corner_b = false;
      unsigned qa = 0, qb = 0;
      if (ea < qn) {
        const bool has_b = eb < qn;
        qa = queue[ea];
        qb = has_b ? queue[eb] : qa;
        int sa, sb;
        fast_ring_score2(tile0 + qa, tile0 + qb, TP, sa, sb);
        corner_a = sa >= th;
        corner_b = has_b && sb >= th;
        if (corner_a && sa > 0) sc0[qa] = (uint8_t)sa;
        if (corner_b && sb > 0) sc0[qb] = (uint8_t)sb;
      }
      const int pa = wave_append(corner_a, lt, cn);
      if (corner_a) queue[pa] = (uint16_t)qa;
      const int pb = wave_append(corner_b, lt, cn);
      if (corner_b) queue[pb] = (uint16_t)qb;
    }
    qn = cn;
#ifdef FAST_SKIP_C
    qn = 0;
#endif
    FPROF(2);
    FPROF(3);
    __syncthreads();
    FPROF(4);
    // ---- C: NMS + ordered emission
    {
      unsigned long long bits = 0;
      int cnt = 0;
      const int nj = (qn + 63) >> 6;
      // rows are contiguous ranges of tile offsets: "the corner's row belongs to this strip" (r0 <= sr0 + y < r1) is one unsigned
      // compare of the entry against wave-uniform bounds
      const unsigned own_lo = (unsigned)__mul24(r0 - sr0, TP), own_n = (unsigned)__mul24(r1 - r0, TP);
      for (int j = 0; j < nj; j++) {
        const int e = j * 64 + lane;
        bool keep = false;
        if (e < qn) {
          const unsigned q = queue[e];
          // r3: the nine scores are read FIRST and reduced with max3 (strictly greater than all eight neighbours = greater than their
          // maximum).  Written as a short-circuit && chain this was nine dependent LDS round trips per chunk, each behind a branch
          // (ds_read_u8 -> s_waitcnt -> v_cmp -> s_and_saveexec); rows of the halo are inside the score map too, so nothing is conditional.
          const uint8_t* p = sc0 + q;
          const int s = p[0];
          const int n0 = p[-1], n1 = p[1], n2 = p[-TP - 1], n3 = p[-TP], n4 = p[-TP + 1], n5 = p[TP - 1], n6 = p[TP], n7 = p[TP + 1];
          const int nm = max(max(max(n0, n1), n2), max(max(max(n3, n4), n5), max(n6, n7)));
          keep = (s > 0) & (s > nm) & (q - own_lo < own_n);
        }
        const unsigned long long m = __builtin_amdgcn_ballot_w64(keep);
        cnt += __popcll(m);
        bits |= (unsigned long long)keep << j;
      }
      if (lane == 0) wcnt[wave] = cnt;
      __syncthreads();
      int base = total;
      for (int w = 0; w < wave; w++) base += wcnt[w];
      const int strip_total = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
      for (int j = 0; j < nj; j++) {
        const bool keep = (bits >> j) & 1ull;
        const unsigned long long m = __ballot(keep);   // (wave_append here would merge the two branches below: kept as measured)
        if (keep) {
          const unsigned q = queue[j * 64 + lane];
          const int y = (int)__umulhi(q, magic_tp), x = (int)q - __mul24(y, TP);   // the one place that needs (y, x): the key of a survivor
          const int s = sc0[q];
          const unsigned pos = (unsigned)(base + __popcll(m & lt));
          if (pos < C.cap)
            out[pos] = ((uint32_t)s << 24) | ((uint32_t)(C.zy0 + sr0 + y) << 12) | (uint32_t)(C.zx0 + x);
        }
        base += __popcll(m);
      }
      total += strip_total;
    }
    FPROF(5);
    __syncthreads();
    FPROF(6);
  }
  if (tid == 0) cell_count[(size_t)frame * ncells_total + cell] = min(total, (int)C.cap);
  FPROF_FLUSH;
}

// ------------------------------------------------------------------------------------------
// Selection (src/ORBextractor.cc:541-605), three steps, one launch each (k_select_quota, k_select_cells [+ k_select_bigcells],
// k_select_final):
//   1. quota redistribution loop            :541-575 (serial per level)
//   2. per-cell retainBest + resize         :586-588   one WAVE per cell: the cell's candidates are staged into LDS, trimmed
//      with the wave-parallel introselect replay (introselect_wave.h) and the survivors written straight to their slot of the
//      level list (:591-597; the kept counts, hence the offsets, are known after step 1)
//   3. level-wide retainBest + resize       :601-604   one wave per level, same replay, list in LDS
// Cells with more candidates than the LDS buffers, or levels whose list exceeds the LDS list, fall back to the serial replay
// in HBM (never seen on VGA / 720p frames; kept for correctness, tests/test_orb_gpu.py::test_selection_paths).
// r1 / early r2 ran the three steps in ONE kernel (8 waves per (level, frame)): those waves sat idle through the serial quota
// loop and the one-wave level step, and a level with 30 cells needed 4 rounds of 8 waves: 0.52 ms against 0.28 ms split.
// ------------------------------------------------------------------------------------------
#define SEL_WAVES 8         // big-cell buffer = SEL_WAVES x the per-geometry cell capacity (what the single kernel's 8 waves held)
#define SEL_LIST_CAP 1536   // level list (LDS)
typedef __attribute__((address_space(3))) uint32_t lds_u32;

// ------------------------------------------------------------------------------------------
//   k_select_quota   one wave per frame, lane l runs level l's quota loop (counts staged through LDS); writes the kept count
//                    and list offset of every cell and the list length of every level
//   k_select_cells   one wave per (cell, frame): retainBest of the cell in LDS, survivors to their slot of the level list in
//                    HBM; k_select_bigcells: the (rare) cells with more candidates than that kernel's small buffer
//   k_select_final   one wave per (level, frame): level-wide retainBest (list through LDS), selected keys + count
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void k_select_quota(const OrbPlan* __restrict__ P, const CellGeom* __restrict__ cells,
                                                     const int32_t* __restrict__ cell_count, int32_t* __restrict__ cell_keep,
                                                     int32_t* __restrict__ cell_off, int32_t* __restrict__ lvl_m) {
  extern __shared__ __attribute__((aligned(16))) int s_q[];   // [4][ncells]: total, evaluated / bNoMore, retain, offset
  const int frame = blockIdx.x, lane = threadIdx.x, nc = P->ncells;
  int* s_total = s_q;
  int* s_flag = s_q + nc;
  int* s_retain = s_q + 2 * nc;
  int* s_offv = s_q + 3 * nc;
  const int32_t* cc = cell_count + (size_t)frame * nc;
  for (int c = lane; c < nc; c += 64) {
    s_total[c] = cc[c];
    s_flag[c] = cells[c].evaluated;
  }
  wave_fence();
  if (lane < P->nlevels) {
    const LevelGeom& L = P->lv[lane];
    int M = 0;
    if (L.ncells > 0 && L.quota > 0) {
      const int nC = L.ncells, c0 = L.cell0, nfc = L.nfeaturesCell;
      int nNoMore = 0, nToDistribute = 0;
      for (int c = c0; c < c0 + nC; c++) {
        const int nKeys = s_total[c];
        if (!s_flag[c]) {                // cell not evaluated: the reference `continue`s (nToRetain=0, bNoMore=false)
          s_retain[c] = 0;
          s_flag[c] = 0;                 // from here on: the bNoMore flag
          continue;
        }
        if (nKeys > nfc) {
          s_retain[c] = nfc;
          s_flag[c] = 0;
        } else {
          s_retain[c] = nKeys;
          nToDistribute += nfc - nKeys;
          s_flag[c] = 1;
          nNoMore++;
        }
      }
      while (nToDistribute > 0 && nNoMore < nC) {
        // nfeaturesCell + ceil((float)nToDistribute/(nCells-nNoMore))
        const int nNew = nfc + (int)ceilf((float)nToDistribute / (float)(nC - nNoMore));
        nToDistribute = 0;
        for (int c = c0; c < c0 + nC; c++) {
          if (!s_flag[c]) {
            if (s_total[c] > nNew) {
              s_retain[c] = nNew;
            } else {
              s_retain[c] = s_total[c];
              nToDistribute += nNew - s_total[c];
              s_flag[c] = 1;
              nNoMore++;
            }
          }
        }
      }
      for (int c = c0; c < c0 + nC; c++) {   // kept counts and their offsets in the level list
        const int k = min(s_total[c], s_retain[c]);
        s_retain[c] = k;
        s_offv[c] = M;
        M += k;
      }
    } else {
      for (int c = L.cell0; c < L.cell0 + max(L.ncells, 0); c++) { s_retain[c] = 0; s_offv[c] = 0; }
    }
    lvl_m[(size_t)frame * P->nlevels + lane] = M;
  }
  wave_fence();
  for (int c = lane; c < nc; c += 64) {
    cell_keep[(size_t)frame * nc + c] = s_retain[c];
    cell_off[(size_t)frame * nc + c] = s_offv[c];
  }
}

__global__ __launch_bounds__(64) void k_select_cells(const OrbPlan* __restrict__ P, const CellGeom* __restrict__ cells,
                                                     uint32_t* __restrict__ cand, const int32_t* __restrict__ cell_count,
                                                     const int32_t* __restrict__ cell_keep, const int32_t* __restrict__ cell_off,
                                                     uint32_t* __restrict__ lvl_scratch, int buf_cap) {
  extern __shared__ __attribute__((aligned(16))) uint32_t s_cellbuf[];   // [buf_cap] candidates | u16 [2 * WAVE_SEL_CAP] stop tables
  const int c = blockIdx.x, frame = blockIdx.y, lane = threadIdx.x, nc = P->ncells;
  const int keep = cell_keep[(size_t)frame * nc + c];
  if (keep <= 0) return;
  const int n = cell_count[(size_t)frame * nc + c], o = cell_off[(size_t)frame * nc + c];
  const CellGeom cg = cells[c];
  uint32_t* src = cand + (size_t)frame * P->cand_per_frame + cg.cand_off;
  uint32_t* glist = lvl_scratch + (size_t)frame * P->cand_per_frame + P->lv[cg.level].cand_off + o;
  if (n > buf_cap) return;   // k_select_bigcells
  lds_u32* buf = (lds_u32*)s_cellbuf;
  for (int i = lane; i < n; i += 64) buf[i] = src[i];
  wave_fence();
  if (n > keep) sdsel::wave_nth_element(buf, n, keep, (sdsel::lds_u16*)(s_cellbuf + buf_cap));
  for (int i = lane; i < keep; i += 64) glist[i] = buf[i];
}

// cells with more candidates than k_select_cells' buffer (dense texture, noise): one wave per (level, frame) walks its level's
// cells and trims those, one at a time, in a buffer of big_cap entries; beyond that the serial replay in HBM (lane 0).
// On ordinary frames every workgroup finds nothing to do and leaves after one load.
__global__ __launch_bounds__(64) void k_select_bigcells(const OrbPlan* __restrict__ P, const CellGeom* __restrict__ cells,
                                                        uint32_t* __restrict__ cand, const int32_t* __restrict__ cell_count,
                                                        const int32_t* __restrict__ cell_keep, const int32_t* __restrict__ cell_off,
                                                        uint32_t* __restrict__ lvl_scratch, int small_cap, int big_cap) {
  extern __shared__ __attribute__((aligned(16))) uint32_t s_cellbuf[];   // [big_cap] candidates | u16 [2 * WAVE_SEL_CAP] stop tables
  const int level = blockIdx.x, frame = blockIdx.y, lane = threadIdx.x, nc = P->ncells;
  const LevelGeom& L = P->lv[level];
  if (L.ncells <= 0 || L.quota <= 0) return;
  for (int c0 = 0; c0 < L.ncells; c0 += 64) {
    const int cl = L.cell0 + c0 + lane;
    const bool mine = c0 + lane < L.ncells && cell_count[(size_t)frame * nc + cl] > small_cap && cell_keep[(size_t)frame * nc + cl] > 0;
    unsigned long long todo = __ballot(mine);
    while (todo) {
      const int c = L.cell0 + c0 + __ffsll((long long)todo) - 1;
      todo &= todo - 1;
      const int n = cell_count[(size_t)frame * nc + c], keep = cell_keep[(size_t)frame * nc + c], o = cell_off[(size_t)frame * nc + c];
      uint32_t* src = cand + (size_t)frame * P->cand_per_frame + cells[c].cand_off;
      uint32_t* glist = lvl_scratch + (size_t)frame * P->cand_per_frame + L.cand_off + o;
      if (n <= big_cap) {
        lds_u32* buf = (lds_u32*)s_cellbuf;
        for (int i = lane; i < n; i += 64) buf[i] = src[i];
        wave_fence();
        if (n > keep) sdsel::wave_nth_element(buf, n, keep, (sdsel::lds_u16*)(s_cellbuf + big_cap));
        for (int i = lane; i < keep; i += 64) glist[i] = buf[i];
        wave_fence();   // the buffer is reused by the next cell
      } else if (lane == 0) {
        if (n > keep) sdsel::nth_element(src, n, keep);
        for (int i = 0; i < keep; i++) glist[i] = src[i];
      }
    }
  }
}

__global__ __launch_bounds__(64) void k_select_final(const OrbPlan* __restrict__ P, const int32_t* __restrict__ lvl_m,
                                                     uint32_t* __restrict__ lvl_scratch, uint32_t* __restrict__ sel,
                                                     int32_t* __restrict__ sel_count) {
  __shared__ uint32_t s_list[SEL_LIST_CAP];
  __shared__ uint16_t s_tmp[2 * WAVE_SEL_CAP];
  const int level = blockIdx.x, frame = blockIdx.y, lane = threadIdx.x;
  const LevelGeom& L = P->lv[level];
  int32_t* out_n = sel_count + (size_t)frame * P->nlevels + level;
  if (L.ncells <= 0 || L.quota <= 0) {
    if (lane == 0) *out_n = 0;
    return;
  }
  const int M = lvl_m[(size_t)frame * P->nlevels + level];
  uint32_t* glist = lvl_scratch + (size_t)frame * P->cand_per_frame + L.cand_off;
  uint32_t* dst = sel + (size_t)frame * P->nsel + L.sel_off;
  int Mout = M;
  if (M > L.quota) {
    Mout = L.quota;
    if (M <= SEL_LIST_CAP) {
      for (int i = lane; i < M; i += 64) s_list[i] = glist[i];
      wave_fence();
      sdsel::wave_nth_element((lds_u32*)s_list, M, L.quota, (sdsel::lds_u16*)s_tmp);
      for (int i = lane; i < Mout; i += 64) dst[i] = s_list[i];
    } else {
      if (lane == 0) sdsel::nth_element(glist, M, L.quota);
      wave_fence();
      for (int i = lane; i < Mout; i += 64) dst[i] = glist[i];
    }
  } else {
    for (int i = lane; i < Mout; i += 64) dst[i] = glist[i];
  }
  if (lane == 0) *out_n = Mout;
}

// ------------------------------------------------------------------------------------------
// k_blur: GaussianBlur(7x7, sigma 2, REFLECT_101) in OpenCV's 8-bit fixed point: integer taps
// round(g*256) = {18,34,49,55,49,34,18}, row pass in int32, column pass (sum + 2^15) >> 16,
// saturated.  The padded pyramid already holds the REFLECT_101 border, so no border logic.
// Register sliding window, no LDS: a thread owns 4 adjacent output columns of a 32-row band,
// reads each input row as 3 aligned dwords (12 bytes cover the 4+6 taps), keeps the last 7
// row-pass results in registers (as pairs of vertically adjacent rows) and emits one packed 4-byte
// store per row.  The taps run on the integer dot-product instructions (v_dot4_u32_u8 for the
// row pass over bytes, v_dot2_u32_u16 for the column pass over the 16-bit row results): 997
// vector instructions per 128 outputs instead of 1570 with mul24 / mad chains, same integers.  Only levels that
// own keypoints are blurred by the reference (src/ORBextractor.cc:655-660); here every level is
// (the blurred image is not an output), which frees the stage from waiting for the selection.
// ------------------------------------------------------------------------------------------
#define BLUR_RB 32                  // output rows per wave
#ifndef BLUR_PF
#define BLUR_PF 8                   // input rows in flight per thread (r3, with the 16-lane groups: 8 rows ORB-only 287.8 k, 6 rows 284.4 k, 4 rows 281.1 k)
#endif

__global__ __launch_bounds__(256) void k_blur(const OrbPlan* __restrict__ P, const BlurTile* __restrict__ tiles,
                                              const uint8_t* __restrict__ pyr, uint8_t* __restrict__ blur,
                                              const int32_t* __restrict__ sel_count) {
  unsigned uframe, utile;
  xcd_frame_block(uframe, utile);
  const BlurTile T = tiles[utile];
  const int frame = (int)uframe, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  (void)sel_count;   // every level is blurred: the stage then depends on the pyramid only and overlaps FAST/selection
  const LevelGeom L = P->lv[T.level];
  // r3: the level is cut into 64-column strips x 32-row bands and the (strip, band) pairs are dealt FLAT to 16-lane groups (strip
  // fastest: the four groups of a wave read 256 contiguous columns wherever the level is that wide).  With a whole wave per 256
  // columns the levels' widths (640, 533, 444, 370, 309, 257, 214, 179) left a quarter of all lanes without a column.
  const int pr = T.p0 + wave * 4 + (lane >> 4);
  // (a single strip has no 32-bit magic number: 2^32 / 1 does not fit)
  const int band = T.nstrips == 1 ? pr : (int)__umulhi((unsigned)pr, T.magic), strip = pr - band * T.nstrips;
  const int x0 = strip * 64 + (lane & 15) * 4;
  const int y0 = band * BLUR_RB;
  if (x0 >= L.w || y0 >= L.h) return;
  const size_t fo = (size_t)frame * P->pyr_frame_bytes + L.off;
  // input bytes for outputs x0..x0+3: padded columns x0+16 .. x0+27 (4-byte aligned)
  const uint8_t* src = pyr + fo + (size_t)(y0 + SD_EDGE - 3) * L.pstride + (x0 + SD_EDGE - 3);
  // the blurred level sits ONE column to the right of the pyramid's layout (interior from padded column 20: its rows have the
  // room, and nothing reads its border): a lane's four output pixels are then an aligned dword
  uint8_t* dst = blur + fo + (size_t)(y0 + SD_EDGE) * L.pstride + (x0 + SD_EDGE + SD_BLUR_SHIFT);
  const int nrows = min(BLUR_RB, L.h - y0);
  const bool full = x0 + 3 < L.w;
  // Row pass: out[k] = sum_i tap[i] * byte[k + i] as two v_dot4_u32_u8 over byte windows cut out of the three dwords with
  // v_alignbyte (<= 255 * 257 = 65535: fits 16 bits).  Column pass: vertically adjacent row results packed in pairs
  // P[r] = R[r] | R[r+1] << 16, so an output is three v_dot2_u32_u16 and one mad; (s + 2^15) >> 16 and the saturation to 255
  // are one v_perm (high halves of two sums) + v_sat_pk_u8_i16 per pixel pair.
  typedef unsigned short us2 __attribute__((ext_vector_type(2)));
  const uint32_t T0 = 18u | 34u << 8 | 49u << 16 | 55u << 24, T1 = 49u | 34u << 8 | 18u << 16;
  const us2 T01 = {18, 34}, T23 = {49, 55}, T45 = {49, 34};
  uint32_t PP[6][4], prevR[4];
  // Input rows are fetched BLUR_PF rows ahead of their use (the row index is clamped to the band's last input row instead of
  // being branched around, so the loads are straight-line code): without this every row was load -> s_waitcnt vmcnt(0) ->
  // compute, 38 dependent global round trips per wave.
  uint32_t pf[BLUR_PF][3];
  const int last_in = nrows + 5;
  const uint32_t srow = (uint32_t)L.pstride;
#pragma unroll
  for (int d = 0; d < BLUR_PF; d++) {
    const uint32_t* rp = (const uint32_t*)(src + (size_t)((uint32_t)min(d, last_in) * srow));
    pf[d][0] = rp[0]; pf[d][1] = rp[1]; pf[d][2] = rp[2];
  }
#pragma unroll
  for (int r = 0; r < BLUR_RB + 6; r++) {
    const uint32_t w0 = pf[r % BLUR_PF][0], w1 = pf[r % BLUR_PF][1], w2 = pf[r % BLUR_PF][2];
    if (r + BLUR_PF < BLUR_RB + 6) {
      const uint32_t* rp = (const uint32_t*)(src + (size_t)((uint32_t)min(r + BLUR_PF, last_in) * srow));
      pf[r % BLUR_PF][0] = rp[0]; pf[r % BLUR_PF][1] = rp[1]; pf[r % BLUR_PF][2] = rp[2];
    }
    if (r < nrows + 6) {
      uint32_t R[4];
      R[0] = __builtin_amdgcn_udot4(w0, T0, __builtin_amdgcn_udot4(w1, T1, 0u, false), false);
#pragma unroll
      for (int k = 1; k < 4; k++)
        R[k] = __builtin_amdgcn_udot4(__builtin_amdgcn_alignbyte(w1, w0, k), T0,
                                      __builtin_amdgcn_udot4(__builtin_amdgcn_alignbyte(w2, w1, k), T1, 0u, false), false);
      if (r >= 1) {
#pragma unroll
        for (int k = 0; k < 4; k++) PP[(r - 1) % 6][k] = prevR[k] | (R[k] << 16);
      }
      if (r >= 6) {
        // output row r-6 = taps over row results r-6 .. r = PP[r-6], PP[r-4], PP[r-2] and R[r]
        uint32_t sum[4];
#pragma unroll
        for (int k = 0; k < 4; k++) {
          uint32_t a = (uint32_t)__mul24(18, (int)R[k]) + (1u << 15);
          a = __builtin_amdgcn_udot2(__builtin_bit_cast(us2, PP[(r - 2) % 6][k]), T45, a, false);
          a = __builtin_amdgcn_udot2(__builtin_bit_cast(us2, PP[(r - 4) % 6][k]), T23, a, false);
          sum[k] = __builtin_amdgcn_udot2(__builtin_bit_cast(us2, PP[(r - 6) % 6][k]), T01, a, false);
        }
        uint32_t h01 = __builtin_amdgcn_perm(sum[1], sum[0], 0x07060302u), h23 = __builtin_amdgcn_perm(sum[3], sum[2], 0x07060302u);
        uint32_t p01, p23;
        asm("v_sat_pk_u8_i16 %0, %1" : "=v"(p01) : "v"(h01));   // values 0..257 as i16 -> u8, saturated
        asm("v_sat_pk_u8_i16 %0, %1" : "=v"(p23) : "v"(h23));
        const uint32_t packed = __builtin_amdgcn_perm(p23, p01, 0x05040100u);
        uint8_t* o = dst + (size_t)(r - 6) * L.pstride;
        if (full) {
          *(uint32_t*)o = packed;
        } else {
          for (int k = 0; k < 4; k++)
            if (x0 + k < L.w) o[k] = (uint8_t)(packed >> (8 * k));
        }
      }
#pragma unroll
      for (int k = 0; k < 4; k++) prevR[k] = R[k];
    }
  }
}

// ------------------------------------------------------------------------------------------
// k_orient_desc: one wavefront per selected keypoint.
//   IC_Angle: integer moments over the r=15 disc (umax table), fastAtan2 polynomial in f32.
//   rBRIEF : a = cosf(angle*pi/180), b = sinf(..) (host-libm-exact, sd_sincosf.h), 256 tests
//            t0 < t1 on the blurred level at cvRound-rotated offsets; lane i evaluates tests
//            i, i+64, i+128, i+192 so each __ballot is 8 descriptor bytes.
//   Output keypoint: pt scaled by mvScaleFactor[level] AFTER description (:669-674).
// Compiled with -ffp-contract=off: every float op below is a single IEEE operation.
// ------------------------------------------------------------------------------------------
__constant__ int8_t c_pattern[1024] = {
#include "orb_pattern.inc"
};
// umax[v] of the r = 15 disc (src/ORBextractor.cc:441-456); compile-time so that the unrolled row loop compares against literals
static constexpr int kUmax[16] = {15, 15, 15, 15, 14, 14, 14, 13, 13, 12, 11, 10, 9, 8, 6, 3};

__device__ __forceinline__ float fast_atan2_deg(float y, float x) {
  const float p1 = 0.9997878412794807f * (float)(180 / 3.14159265358979323846);
  const float p3 = -0.3258083974640975f * (float)(180 / 3.14159265358979323846);
  const float p5 = 0.1555786518463281f * (float)(180 / 3.14159265358979323846);
  const float p7 = -0.04432655554792128f * (float)(180 / 3.14159265358979323846);
  const float eps = (float)2.2204460492503131e-16;
  float ax = fabsf(x), ay = fabsf(y);
  float a, c, c2;
  if (ax >= ay) {
    c = ay / (ax + eps);
    c2 = c * c;
    a = (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c;
  } else {
    c = ax / (ay + eps);
    c2 = c * c;
    a = 90.f - (((p7 * c2 + p5) * c2 + p3) * c2 + p1) * c;
  }
  if (x < 0) a = 180.f - a;
  if (y < 0) a = 360.f - a;
  return a;
}

#ifndef DESC_KPW
#define DESC_KPW 2   // keypoints per wave
#endif
#define DESC_PATCH_LD 3                       // 8-byte loads per lane and keypoint: 3 x 64 >= 37 rows x 5 dword pairs
#define DESC_PATCH_DW (2 * DESC_PATCH_LD * 64)
__global__ __launch_bounds__(256) void k_orient_desc(const OrbPlan* __restrict__ P, const uint8_t* __restrict__ pyr,
                                                     const uint8_t* __restrict__ blur,
                                                     const uint32_t* __restrict__ sel,
                                                     const int32_t* __restrict__ sel_count,
                                                     sd_keypoint* __restrict__ kps, uint8_t* __restrict__ desc,
                                                     int32_t* __restrict__ nout, int cap, int n_frames, int bpf) {
  // XCD-aware block order: workgroups are handed to the 8 XCDs round-robin, and each XCD has its own
  // 4 MB L2.  Block b works on frame 8 * (b / (8 * bpf)) + (b % 8), so all workgroups of a frame run on
  // ONE XCD and the frame's two pyramids (2.8 MB at VGA) stay L2-resident while its ~1000 overlapping
  // 31 x 31 patches are read (measured: HBM fetch 6.1 GB -> see DESIGN.md section 6).
  const int bx = blockIdx.x;
  const int xcd = bx & 7, t = bx >> 3;
  const int frame = (t / bpf) * 8 + xcd, blk = t % bpf;
  if (frame >= n_frames) return;
  const int lane = threadIdx.x & 63;
  // Two keypoints per wave, interleaved: the kernel is a chain of dependent gathers (key -> 31 x 31 patch -> angle ->
  // 512 sample points), so a wave with two independent chains in flight keeps twice the loads outstanding.
  // Everything that is the same for the whole wave (keypoint position, level geometry, patch base pointers, angle, cos, sin) is
  // made scalar with readfirstlane / readlane: the gathers then use the SGPR-base + 32-bit-offset addressing form (no 64-bit
  // vector address arithmetic), and the angle / cos / sin of BOTH keypoints are evaluated once, in the two halves of the wave.
  const int g0 = __builtin_amdgcn_readfirstlane((blk * 4 + (int)(threadIdx.x >> 6)) * DESC_KPW);   // output slots g0 .. g0 + DESC_KPW - 1
  const int32_t* sc = sel_count + (size_t)frame * P->nlevels;
  int level[DESC_KPW], idx[DESC_KPW], acc = 0;
#pragma unroll
  for (int q = 0; q < DESC_KPW; q++) { level[q] = -1; idx[q] = 0; }
  for (int l = 0; l < P->nlevels; l++) {
    const int n = sc[l];
#pragma unroll
    for (int q = 0; q < DESC_KPW; q++)
      if (level[q] < 0 && g0 + q < acc + n) {
        level[q] = l;
        idx[q] = g0 + q - acc;
      }
    acc += n;
  }
  if (blk == 0 && threadIdx.x == 0) nout[frame] = min(acc, cap);
  bool live[DESC_KPW];
  int X[DESC_KPW], Y[DESC_KPW], resp[DESC_KPW], step[DESC_KPW];
  const uint8_t* pbase[DESC_KPW];   // pixel (X - 19, Y - 19) of the level: every offset below is non-negative (the border is 19 px)
  const uint8_t* bbase[DESC_KPW];   // same position in the blurred level
  float scale[DESC_KPW], kpsize[DESC_KPW];
#pragma unroll
  for (int q = 0; q < DESC_KPW; q++) {
    live[q] = level[q] >= 0 && g0 + q < cap;
    const int lv = live[q] ? level[q] : 0;
    const LevelGeom& L = P->lv[lv];
    const uint32_t key = live[q] ? sel[(size_t)frame * P->nsel + L.sel_off + idx[q]] : 0u;
    X[q] = live[q] ? (int)(key & 0xfff) : SD_EDGE;     // dead slot: a harmless in-range position
    Y[q] = live[q] ? (int)((key >> 12) & 0xfff) : SD_EDGE;
    resp[q] = key >> 24;
    step[q] = L.pstride;
    scale[q] = L.scale;
    kpsize[q] = L.kpsize;
    const size_t fo = (size_t)frame * P->pyr_frame_bytes + L.off + (size_t)(Y[q] + SD_EDGE - 19) * L.pstride + X[q] + SD_EDGE - 19;
    pbase[q] = pyr + fo;
    bbase[q] = blur + fo + SD_BLUR_SHIFT;
  }
  if (!live[0]) return;   // slots are filled in order: no first keypoint, no second

  // ---- the blurred 37 x 37 patch of each keypoint (the rotated test points reach +-18) goes to LDS as 37 rows of ten aligned
  // dwords, fetched NOW, beside the IC_Angle rows: the 512 sample reads of a keypoint were byte gathers over ~30 cache lines
  // per instruction that could only start once the angle was known
  __shared__ __attribute__((aligned(16))) uint32_t s_patch[4][DESC_KPW][DESC_PATCH_DW];
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  uint2 pdw[DESC_KPW][DESC_PATCH_LD];
  int psh[DESC_KPW];
#pragma unroll
  for (int q = 0; q < DESC_KPW; q++) {
    const uint8_t* a = bbase[q] + step[q] + 1;            // pixel (X - 18, Y - 18)
    psh[q] = (int)((uintptr_t)a & 3);
    const uint8_t* a4 = a - psh[q];
#pragma unroll
    for (int k = 0; k < DESC_PATCH_LD; k++) {
      const int e = min(k * 64 + lane, 37 * 5 - 1);
      const int row = (int)(((unsigned)e * 13108u) >> 16);   // e / 5, e < 192
      const int d = e - row * 5;
      pdw[q][k] = *(const uint2*)(a4 + (uint32_t)(__mul24(row, step[q]) + 8 * d));   // 4-byte aligned: one global_load_dwordx2
    }
  }

  // ---- IC_Angle: m10 = sum u * I, m01 = sum v * I over the disc.  Lane = (column u, half): the lower half of the wave walks
  // the rows +v, the upper half the rows -v; per row one load per keypoint, u * (sum of the column) and +-(sum of v * I) at
  // the end (integer sums: any order is exact).
  int m10[DESC_KPW], m01[DESC_KPW];
  {
    const int u = (lane & 31) - 15;
    const int half = lane >> 5;   // 0: rows +v, 1: rows -v
    const bool act = (lane & 31) < 31;
    const int au = abs(u);
    uint32_t off[DESC_KPW];
    int dstep[DESC_KPW], colsum[DESC_KPW], vsum[DESC_KPW];
#pragma unroll
    for (int q = 0; q < DESC_KPW; q++) {
      off[q] = (uint32_t)(19 * step[q] + 19 + u);
      dstep[q] = half ? -step[q] : step[q];
      colsum[q] = vsum[q] = 0;
    }
    // All 2 x 16 row loads are issued first, unconditionally (every position of the 31 x 31 square around a keypoint lies
    // inside the padded level; lane 31 / 63 reads column +16, also inside): straight-line code, 32 loads in flight.  With the
    // disc test as a branch around each row the generated code was load -> s_waitcnt vmcnt(0) -> add, sixteen dependent
    // round trips.  The disc is applied afterwards: umax[] is non-increasing, so row v counts iff v <= vlim(|u|).
    int vals[16][DESC_KPW];
#pragma unroll
    for (int v = 0; v <= 15; v++) {
#pragma unroll
      for (int q = 0; q < DESC_KPW; q++) {
        vals[v][q] = pbase[q][off[q]];
        off[q] += (uint32_t)dstep[q];
      }
    }
#pragma unroll
    for (int q = 0; q < DESC_KPW; q++)
#pragma unroll
      for (int k = 0; k < DESC_PATCH_LD; k++) ((uint2*)s_patch[wv][q])[k * 64 + lane] = pdw[q][k];   // pair e = dwords 2 e, 2 e + 1 of the patch
    int vlim = -1;   // largest row index of this lane's column inside the disc (-1: lane outside)
#pragma unroll
    for (int v = 0; v <= 15; v++) vlim += (act && au <= kUmax[v]) ? 1 : 0;
#pragma unroll
    for (int v = 0; v <= 15; v++) {
      const bool in = v <= vlim && !(half && v == 0);
#pragma unroll
      for (int q = 0; q < DESC_KPW; q++) {
        const int val = in ? vals[v][q] : 0;
        colsum[q] += val;
        vsum[q] += v * val;
      }
    }
#pragma unroll
    for (int q = 0; q < DESC_KPW; q++) {   // DPP reduction of the device library
      m10[q] = wave_sum_i32(u * colsum[q]);
      m01[q] = wave_sum_i32(half ? -vsum[q] : vsum[q]);
    }
  }
  // ---- angle, cos, sin: keypoint 0 in lanes 0..31, keypoint 1 in lanes 32..63, one evaluation
  const float factorPI = (float)(3.14159265358979323846 / 180.f);
  float angle[DESC_KPW], ca[DESC_KPW], sb[DESC_KPW];
  {
    static_assert(DESC_KPW == 2, "the angle evaluation splits the wave in two");
    const float my = (float)(lane < 32 ? m01[0] : m01[1]), mx = (float)(lane < 32 ? m10[0] : m10[1]);
    const float ang = fast_atan2_deg(my, mx);
    const float arad = ang * factorPI;
    const float c = sdsc::cosf_glibc(arad), sn = sdsc::sinf_glibc(arad);
#pragma unroll
    for (int q = 0; q < DESC_KPW; q++) {
      angle[q] = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, ang), 32 * q));
      ca[q] = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, c), 32 * q));
      sb[q] = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, sn), 32 * q));
    }
  }
  // ---- steered rBRIEF on the blurred level
  unsigned long long words[DESC_KPW][4];
  wave_fence();   // this wave's own patch stores before its sample reads
#pragma unroll
  for (int j = 0; j < 4; j++) {
    const int t = j * 64 + lane;
    const char4 pt = *(const char4*)(&c_pattern[t * 4]);
    const float x0 = (float)pt.x, y0 = (float)pt.y, x1 = (float)pt.z, y1 = (float)pt.w;
    int t0[DESC_KPW], t1[DESC_KPW];
#pragma unroll
    for (int q = 0; q < DESC_KPW; q++) {
      const float a = ca[q], b = sb[q];
      // center[cvRound(x*b + y*a)*step + cvRound(x*a - y*b)]
      const int r0 = __float2int_rn(x0 * b + y0 * a), q0 = __float2int_rn(x0 * a - y0 * b);
      const int r1 = __float2int_rn(x1 * b + y1 * a), q1 = __float2int_rn(x1 * a - y1 * b);
      const uint8_t* pb = (const uint8_t*)s_patch[wv][q] + (18 * 40 + 18 + psh[q]);
      t0[q] = pb[__mul24(r0, 40) + q0];
      t1[q] = pb[__mul24(r1, 40) + q1];
    }
#pragma unroll
    for (int q = 0; q < DESC_KPW; q++) words[q][j] = __builtin_amdgcn_ballot_w64(t0[q] < t1[q]);
  }
#pragma unroll
  for (int q = 0; q < DESC_KPW; q++) {
    if (!live[q]) continue;
    const int g = g0 + q;
    if (lane < 4) {
      unsigned long long w = lane == 0 ? words[q][0] : lane == 1 ? words[q][1] : lane == 2 ? words[q][2] : words[q][3];
      *(unsigned long long*)(desc + ((size_t)frame * cap + g) * 32 + lane * 8) = w;
    }
    if (lane == 0) {
      sd_keypoint k;
      float fx = (float)X[q], fy = (float)Y[q];
      if (level[q] != 0) {
        fx = fx * scale[q];
        fy = fy * scale[q];
      }
      k.x = fx;
      k.y = fy;
      k.size = kpsize[q];
      k.angle = angle[q];
      k.response = (float)resp[q];
      k.octave = level[q];
      k.class_id = -1;
      kps[(size_t)frame * cap + g] = k;
    }
  }
}

// ------------------------------------------------------------------------------------------
// k_undistort: Frame::UndistortKeyPoints (src/Frame.cc:335-366) = cv::undistortPoints(pts, pts, K,
// dist, Mat(), K), OpenCV 3.2: normalise, 5 fixed-point iterations of the radial/tangential
// model in fp64, re-project with P = K, narrow to f32.  One thread per keypoint.
// ------------------------------------------------------------------------------------------
struct DistParams { double fx, fy, cx, cy, k[12]; };

__global__ void k_undistort(const sd_keypoint* __restrict__ kps, sd_keypoint* __restrict__ kps_un, const int32_t* __restrict__ nout,
                            int cap, DistParams D) {
  const int frame = blockIdx.y;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= nout[frame]) return;
  sd_keypoint kp = kps[(size_t)frame * cap + i];
  const double ifx = 1. / D.fx, ify = 1. / D.fy;
  double x = kp.x, y = kp.y;
  x = (x - D.cx) * ifx;
  y = (y - D.cy) * ify;
  const double x0 = x, y0 = y;
  for (int j = 0; j < 5; j++) {
    const double r2 = x * x + y * y;
    const double icdist = (1 + ((D.k[7] * r2 + D.k[6]) * r2 + D.k[5]) * r2) / (1 + ((D.k[4] * r2 + D.k[1]) * r2 + D.k[0]) * r2);
    const double deltaX = 2 * D.k[2] * x * y + D.k[3] * (r2 + 2 * x * x) + D.k[8] * r2 + D.k[9] * r2 * r2;
    const double deltaY = D.k[2] * (r2 + 2 * y * y) + 2 * D.k[3] * x * y + D.k[10] * r2 + D.k[11] * r2 * r2;
    x = (x0 - deltaX) * icdist;
    y = (y0 - deltaY) * icdist;
  }
  const double xx = D.fx * x + 0.0 * y + D.cx;
  const double yy = 0.0 * x + D.fy * y + D.cy;
  const double ww = 1. / (0.0 * x + 0.0 * y + 1.0);
  kp.x = (float)(xx * ww);
  kp.y = (float)(yy * ww);
  kps_un[(size_t)frame * cap + i] = kp;
}

}  // namespace sd

// ==========================================================================================
// host side: the launch pipeline (the handle and the C ABI are in orb_host.hip)
// ==========================================================================================
using namespace sd;

namespace {

// One call of pipeline_body: its arguments, what it chose at the fork, and its profiling state.  The steps are the member
// functions, in the order pipeline_body calls them; every step queues its records, waits and launches in program order.
struct Pipeline {
  sd_orb* const h;
  const uint8_t* const d_imgs;
  const int n, stride;
  const size_t frame_stride;
  const bool prof;
  hipEvent_t* const ev;
  const bool frames_ready, capturing;
  const HostPlan& hp = h->hp;
  const OrbPlan& P = hp.plan;
  const hipStream_t s = h->stream;
  const bool src_aligned = (((uintptr_t)d_imgs | (uintptr_t)stride | (uintptr_t)frame_stride) & 3) == 0;
  // FAST of level 0 reads the frames themselves when they are 4-byte aligned: it starts at once, beside the resize chain
  // (in 16-byte units when base and strides allow, else dword by dword)
  const bool src_wide = (((uintptr_t)d_imgs | (uintptr_t)stride | (uintptr_t)frame_stride) & 15) == 0;
  const bool fast0_direct = src_aligned && P.lv[0].ncells > 0 && opt(OPT_FAST0_FROM_FRAMES) != 0;
  const int ring_slot = h->ev_calls % sd_orb::kRing;
  bool fast_early = false, pyr_early = false;
  hipStream_t ps = nullptr;   // stream of the resize chain: main, or auxiliary (pyr_early)
  bool fast_started = false;
  int nfp = 0;   // FAST launches timed so far

  int mark(StageEvent e, hipStream_t stream) {
    if (prof) SD_HIP_CHECK(hipEventRecord(ev[e], stream));
    return SD_OK;
  }

  int fork() {
    // The previous call's selection (main stream) read d_cand / d_cell_count: FAST must not overwrite them before it is done.
    // r3: FAST of level 0 reads the caller's frames and needs nothing else of THIS call, so with frames that are already on the
    // device (frames_ready: the device-input entry point) it is ordered behind the previous SELECTION only (ev_select_done)
    // and runs beside the previous batch's descriptor kernel, a gather-latency-bound kernel that leaves the vector ALUs idle.
    // The upload of these frames is then ordered by sd_orb_stream_fence, which makes the FAST and auxiliary streams wait as
    // well.  Only on the handle's own stream: on a caller's stream the producer of the frames may be queued on that very
    // stream, and stream order is the contract.  Otherwise (host frames copied on this stream, a caller's stream, a captured
    // graph, option off, first call) behind everything queued so far.
    fast_early = frames_ready && !capturing && h->select_recorded && h->stream == h->own_stream && opt(OPT_FAST0_EARLY) != 0;
    if (fast_early) SD_HIP_CHECK(hipStreamWaitEvent(h->fast_stream, h->ev_select_done, 0));
    SD_HIP_CHECK(hipEventRecord(h->ev_body_start, s));
    if (!fast_early) SD_HIP_CHECK(hipStreamWaitEvent(h->fast_stream, h->ev_body_start, 0));
    // r3: with two output sets (a tracker is attached) the pyramid of this call goes into the set the previous call does NOT read,
    // so the resize chain, too, may run beside the previous call's descriptor kernel -- on the auxiliary stream in front of the
    // blur, which follows it anyway (a FIFTH stream lands on the hardware queue of the FAST stream and the two serialise: HIP
    // spreads a process's streams over four hardware queues) -- behind the previous selection, the upload of the frames and the
    // tracker's last read of that set (orb_launch_pipeline); the FAST launches of levels 1... then follow level 0 without waiting for
    // the descriptors to end (they were idle for 0.6 ms per step).  OFF by default: bit-exact (tests run it), but the full step with
    // the PnP solve loses 8 % (172 k vs 194.6 k frames/s, three alternating runs) -- the tracking kernels of the previous batch
    // then share the machine with two FAST launches instead of one; with TrackWithMotionModel it is even (187 k both).
    pyr_early = fast_early && h->nsets == 2 && opt(OPT_PYR_EARLY) != 0;
    ps = pyr_early ? h->aux_stream : s;
    if (pyr_early) SD_HIP_CHECK(hipStreamWaitEvent(ps, h->ev_select_done, 0));
    return mark(EV_PYR_BEGIN, ps);   // (the pyramid stage is timed on the stream it runs on)
  }

  // One k_fast_cells launch on the FAST stream: ncl cells from the first cell of level `first`, rows read at src
  int launch_fast(const uint8_t* src, size_t src_frame_stride, const FastSrc& fs, int edge, int first, int ncl, size_t lds, bool wide) {
    if (!fast_started) SD_TRY(mark(EV_FAST_BEGIN, h->fast_stream));
    fast_started = true;
    const bool timed = prof && h->evf_ready && nfp < sd_orb::kFastPairs;
    if (timed) (void)hipEventRecord(h->evf[ring_slot][2 * nfp], h->fast_stream);
    hipLaunchKernelGGL(k_fast_cells, dim3(ncl, n), dim3(256), lds, h->fast_stream, h->d_cells, src, src_frame_stride, fs, edge, h->d_cand,
                       P.cand_per_frame, h->d_cell_count, P.ncells, P.lv[first].cell0, P.thFAST, wide ? 1 : 0);
    if (timed) (void)hipEventRecord(h->evf[ring_slot][2 * nfp + 1], h->fast_stream);
    nfp++;
    return SD_OK;
  }

  int fast_level0_direct() {
    FastSrc fs0;
    memset(&fs0, 0, sizeof(fs0));
    fs0.pstride[0] = stride;
    return launch_fast(d_imgs, frame_stride, fs0, 0, 0, P.lv[0].ncells, hp.fast_lds_level[0], src_wide);
  }

  int pyramid_level(int l) {
    const LevelGeom& L = P.lv[l];
    const LevelGeom& S = P.lv[l > 0 ? l - 1 : 0];
    const bool split = L.w >= 16 && L.fast_resize != 0 && (l > 0 || src_aligned);
    if (!split) {   // generic single-pass kernel (exact-2x INTER_AREA levels, odd source alignment, tiny levels)
      dim3 grid((L.pstride + 255) / 256, (L.prows + 4 * PYR_ROWS - 1) / (4 * PYR_ROWS), n), block(64, 4, 1);
      hipLaunchKernelGGL(k_pyr_level, grid, block, 0, ps, L, S, (size_t)P.pyr_frame_bytes, l, d_imgs, stride, frame_stride, h->d_pyr);
      return SD_OK;
    }
    const PyrGroups& D = hp.pyr[l];   // groups per padded row, their checked magic number, k_pyr_split's row slots (orb_plan.cpp)
    if (l > 0 && L.nblk > 0) {   // rows in runs that share source rows (orb_plan.cpp row_blocks): one thread per (row block, group)
      hipLaunchKernelGGL(k_pyr_rows, dim3(pyr_blocks(L.nblk, D.G), n), dim3(256), 0, ps, L, S, (size_t)P.pyr_frame_bytes, h->d_coef, h->d_pyr,
                         D.G, D.magic);
      return SD_OK;
    }
    hipLaunchKernelGGL(k_pyr_split, dim3(pyr_blocks(D.Hh, D.G), n), dim3(256), 0, ps, L, S, (size_t)P.pyr_frame_bytes, l, h->d_coef, d_imgs,
                       stride, frame_stride, h->d_pyr, D.G, D.magic, D.Hh, D.mirror);
    return SD_OK;
  }

  // FAST of level l starts as soon as the level is complete, on its own stream
  int fast_of_level(int l, const FastSrc& fsrc) {
    // levels >= merge_from share ONE launch after the last level is complete (cells of consecutive levels are contiguous)
    const int merge_from = hp.fast_merge_from;   // orb_plan.cpp
    const bool merged = l >= merge_from;
    int ncl = P.lv[l].ncells;
    size_t lds = hp.fast_lds_level[l];
    if (merged) {
      if (l != P.nlevels - 1) return SD_OK;
      ncl = 0;
      lds = 0;
      for (int m = merge_from; m < P.nlevels; m++) {
        ncl += P.lv[m].ncells;
        lds = std::max(lds, hp.fast_lds_level[m]);
      }
    }
    if (ncl == 0 || (l == 0 && fast0_direct)) return SD_OK;
    SD_HIP_CHECK(hipEventRecord(h->ev_level[l], ps));
    SD_HIP_CHECK(hipStreamWaitEvent(h->fast_stream, h->ev_level[l], 0));
    // (d_pyr, the levels' offsets, their row pitches and the frame stride are multiples of 64)
    return launch_fast(h->d_pyr, (size_t)P.pyr_frame_bytes, fsrc, SD_EDGE, merged ? merge_from : l, ncl, lds, true);
  }

  // blur on the auxiliary stream, beside FAST + selection (d_blur exists once: behind the previous call's descriptors)
  int blur() {
    SD_HIP_CHECK(hipEventRecord(h->ev_pyr_done, ps));
    SD_HIP_CHECK(hipStreamWaitEvent(h->aux_stream, h->ev_pyr_done, 0));
    if (pyr_early) SD_HIP_CHECK(hipStreamWaitEvent(h->aux_stream, h->ev_body_start, 0));
    SD_TRY(mark(EV_BLUR_BEGIN, h->aux_stream));
    hipLaunchKernelGGL(k_blur, dim3((unsigned)hp.blur_tiles.size(), n), dim3(256), 0, h->aux_stream, h->d_plan, h->d_tiles, h->d_pyr,
                       h->d_blur, h->d_sel_count);
    SD_TRY(mark(EV_BLUR_END, h->aux_stream));
    SD_HIP_CHECK(hipEventRecord(h->ev_blur_done, h->aux_stream));
    return SD_OK;
  }

  int join_fast() {
    if (!fast_started) SD_TRY(mark(EV_FAST_BEGIN, h->fast_stream));
    SD_TRY(mark(EV_FAST_END, h->fast_stream));
    if (prof) h->evf_n[ring_slot] = h->evf_ready ? nfp : 0;
    // ev_fast_done stands for "pyramid AND FAST complete" (a tracker's ImageAlign waits for it alone, track_handle.h wait_inputs): a
    // level without grid cells launches no FAST, so the FAST stream has not necessarily waited for that level's resize
    // (few features: no cells at all on the merged small levels) -- order it behind the whole pyramid explicitly
    SD_HIP_CHECK(hipStreamWaitEvent(h->fast_stream, h->ev_pyr_done, 0));
    SD_HIP_CHECK(hipEventRecord(h->ev_fast_done, h->fast_stream));
    SD_HIP_CHECK(hipStreamWaitEvent(s, h->ev_fast_done, 0));
    return SD_OK;
  }

  int select() {
    SD_TRY(mark(EV_SELECT_BEGIN, s));
    const int sel_cap = hp.max_cell_pixels > 12000 ? 1024 : 512;
    if (P.ncells > 0) {
      hipLaunchKernelGGL(k_select_quota, dim3(n), dim3(64), (size_t)P.ncells * 16, s, h->d_plan, h->d_cells, h->d_cell_count, h->d_cell_keep,
                         h->d_cell_off, h->d_lvl_m);
      // small buffer = 2 x sel_cap entries (5 KB at VGA: 32 one-wave workgroups per CU; 4 x was 0.385 ms, 2 x and 1 x 0.275 ms);
      // big buffer = SEL_WAVES x sel_cap
      int small_cap = 2 * sel_cap, big_cap = SEL_WAVES * sel_cap;
      if (const int e = opt(OPT_SELECT_SMALL_CAP)) small_cap = std::max(1, std::min(e, small_cap));   // tests: force the other paths
      if (const int e = opt(OPT_SELECT_BIG_CAP)) big_cap = std::max(small_cap, std::min(e, big_cap));
      hipLaunchKernelGGL(k_select_cells, dim3(P.ncells, n), dim3(64), (size_t)small_cap * 4 + 2 * WAVE_SEL_CAP * 2, s, h->d_plan, h->d_cells,
                         h->d_cand, h->d_cell_count, h->d_cell_keep, h->d_cell_off, h->d_scratch, small_cap);
      hipLaunchKernelGGL(k_select_bigcells, dim3(P.nlevels, n), dim3(64), (size_t)big_cap * 4 + 2 * WAVE_SEL_CAP * 2, s, h->d_plan, h->d_cells,
                         h->d_cand, h->d_cell_count, h->d_cell_keep, h->d_cell_off, h->d_scratch, small_cap, big_cap);
    }
    // (also without any grid cell -- nfeatures so small that every level's levelCols is 0: the per-level counts the descriptor
    // kernel reads must still be written, as zeros)
    hipLaunchKernelGGL(k_select_final, dim3(P.nlevels, n), dim3(64), 0, s, h->d_plan, h->d_lvl_m, h->d_scratch, h->d_sel, h->d_sel_count);
    if (!capturing) {   // d_cand / d_cell_count are free again: the next call's level-0 FAST may start (see fork)
      SD_HIP_CHECK(hipEventRecord(h->ev_select_done, s));
      h->select_recorded = true;
    }
    return mark(EV_SELECT_END, s);
  }

  int describe() {
    SD_HIP_CHECK(hipStreamWaitEvent(s, h->ev_blur_done, 0));
    SD_TRY(mark(EV_DESC_BEGIN, s));
    const int cap = std::max(P.nsel, 1);
    const int bpf = (cap + 4 * DESC_KPW - 1) / (4 * DESC_KPW);   // 4 waves x DESC_KPW keypoints per workgroup
    hipLaunchKernelGGL(k_orient_desc, dim3((unsigned)(((n + 7) / 8) * 8 * bpf)), dim3(256), 0, s, h->d_plan, h->d_pyr, h->d_blur, h->d_sel,
                       h->d_sel_count, h->d_kps, h->d_desc, h->d_nout, cap, n, bpf);
    if (h->have_dist) {   // mvKeysUn != mvKeys only when k1 != 0 (src/Frame.cc:336-339)
      DistParams D;
      D.fx = h->dist_K[0]; D.fy = h->dist_K[1]; D.cx = h->dist_K[2]; D.cy = h->dist_K[3];
      for (int i = 0; i < 12; i++) D.k[i] = i < 5 ? (double)h->dist[i] : 0.0;
      hipLaunchKernelGGL(k_undistort, dim3((cap + 255) / 256, n), dim3(256), 0, s, h->d_kps, h->d_kps_un, h->d_nout, cap, D);
    }
    return mark(EV_DESC_END, s);
  }
};

// The kernels of one extraction on the handle's three streams (main: pyramid chain, select, descriptors; fast: FAST per
// level; aux: blur), forked and joined with events only -- also what gets captured into a hipGraph.
int pipeline_body(sd_orb* h, const uint8_t* d_imgs, int n, int stride, size_t frame_stride, bool prof, hipEvent_t* ev, bool frames_ready,
                  bool capturing) {
  Pipeline p{h, d_imgs, n, stride, frame_stride, prof, ev, frames_ready, capturing};
  SD_TRY(p.fork());
  if (p.fast0_direct) SD_TRY(p.fast_level0_direct());
  FastSrc fsrc;
  memset(&fsrc, 0, sizeof(fsrc));
  for (int l = 0; l < p.P.nlevels; l++) {
    fsrc.off[l] = p.P.lv[l].off;
    fsrc.pstride[l] = p.P.lv[l].pstride;
  }
  for (int l = 0; l < p.P.nlevels; l++) {
    SD_TRY(p.pyramid_level(l));
    SD_TRY(p.fast_of_level(l, fsrc));
  }
  SD_TRY(p.mark(EV_PYR_END, p.ps));
  SD_TRY(p.blur());
  SD_TRY(p.join_fast());
  SD_TRY(p.select());
  SD_TRY(p.describe());
  SD_HIP_CHECK(hipGetLastError());
  return SD_OK;
}

// The cached graph of this call's arguments into ge, captured and instantiated on first use
int graph_for(sd_orb* h, const uint8_t* d_imgs, int n, int stride, size_t frame_stride, sd_orb::GraphEntry*& ge) {
  const sd_orb::GraphKey key = graph_key(h, d_imgs, n, stride, frame_stride);
  for (auto& g : h->graphs)
    if (g.exec && g.key == key) ge = &g;
  if (ge) return SD_OK;
  hipStream_t s = h->stream;
  hipGraph_t graph = nullptr;
  SD_HIP_CHECK(hipStreamBeginCapture(s, hipStreamCaptureModeThreadLocal));
  int rc = pipeline_body(h, d_imgs, n, stride, frame_stride, false, nullptr, false, true);
  h->select_recorded = false;   // the graph's selection is not an event record a later call could wait for
  hipError_t e = hipStreamEndCapture(s, &graph);
  if (rc == SD_OK && e != hipSuccess) {
    set_error(std::string("hipStreamEndCapture: ") + hipGetErrorString(e));
    rc = SD_ERR_HIP;
  }
  if (rc == SD_OK) {
    sd_orb::GraphEntry& slot = h->graphs[h->graph_next++ % 4];
    if (slot.exec) (void)hipGraphExecDestroy(slot.exec);
    slot = sd_orb::GraphEntry();
    e = hipGraphInstantiate(&slot.exec, graph, nullptr, nullptr, 0);
    if (e != hipSuccess) {
      set_error(std::string("hipGraphInstantiate: ") + hipGetErrorString(e));
      rc = SD_ERR_HIP;
    } else {
      slot.key = key;
      ge = &slot;
    }
  }
  if (graph) (void)hipGraphDestroy(graph);
  return rc;
}

}  // namespace

namespace sd {

void orb_drop_graphs(sd_orb* h) {
  for (auto& g : h->graphs) {
    if (g.exec) (void)hipGraphExecDestroy(g.exec);
    g = sd_orb::GraphEntry();
  }
}

int orb_launch_pipeline(sd_orb* h, const uint8_t* d_imgs, int n, int stride, size_t frame_stride, bool frames_ready) {
  hipStream_t s = h->stream;
  const bool prof = h->profiling;
  // next output set; a tracker may still be reading its previous contents on another stream
  select_set(h, (h->set + 1) % h->nsets);
  if (h->set_busy[h->set]) {
    SD_HIP_CHECK(hipStreamWaitEvent(s, h->ev_set_free[h->set], 0));
    if (h->nsets == 2) SD_HIP_CHECK(hipStreamWaitEvent(h->aux_stream, h->ev_set_free[h->set], 0));   // (an early pyramid, pipeline_body)
    h->set_busy[h->set] = false;
  }
  // hipGraph replay is opt-in (option "extract.use_graph"): measured on ROCm 7.2 / MI355X the single-frame call takes 0.43 ms through
  // the graph against 0.37 ms with direct launches (tools/exp_pcie.py), so direct launches stay the default
  const bool use_graph = opt(OPT_USE_GRAPH) != 0;
  if (prof || !use_graph) {
    SD_TRY(pipeline_body(h, d_imgs, n, stride, frame_stride, prof, h->ev[h->ev_calls % sd_orb::kRing], frames_ready, false));
  } else {
    sd_orb::GraphEntry* ge = nullptr;
    SD_TRY(graph_for(h, d_imgs, n, stride, frame_stride, ge));
    SD_HIP_CHECK(hipGraphLaunch(ge->exec, s));
    // a replayed selection records no event either: the next direct call's level-0 FAST must not wait for an older one
    // (it would overwrite d_cand / d_cell_count under this graph's FAST and selection)
    h->select_recorded = false;
  }
  // inside a captured graph ev_pyr_done is a graph node, not an event record a later hipStreamWaitEvent could see
  h->pyr_event_live = prof || !use_graph;
  SD_HIP_CHECK(hipEventRecord(h->ev_extract_done, s));
  h->extract_recorded = true;
  h->extract_serial++;
  if (prof) h->ev_calls++;
  h->last_frames = n;
  return SD_OK;
}

int read_sel_prof(unsigned long long* out64, int reset) {   // out64[8 * i + 7] = FAST phase i (the other slots: 0)
#ifdef SD_PNP_PROF
  SD_HIP_CHECK(hipDeviceSynchronize());
  for (int i = 0; i < 64; i++) out64[i] = 0;   // the selection kernels carry no timers since the split (a rocprofv3 trace times them)
  unsigned long long f[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  {
    std::vector<unsigned long long> wg((size_t)FPROF_FRAMES * FPROF_CELLS * 8);
    SD_HIP_CHECK(hipMemcpyFromSymbol(wg.data(), HIP_SYMBOL(g_fast_prof_wg), wg.size() * 8));
    for (size_t i = 0; i < wg.size(); i++) f[i & 7] += wg[i];
    if (reset) {
      std::fill(wg.begin(), wg.end(), 0ull);
      SD_HIP_CHECK(hipMemcpyToSymbol(HIP_SYMBOL(g_fast_prof_wg), wg.data(), wg.size() * 8));
    }
  }
  for (int l = 0; l < 8; l++) out64[l * 8 + 7] = f[l];   // slot 7 of every level row carries FAST phase l
  return SD_OK;
#else
  set_error("library built without -DSD_PNP_PROF");
  return SD_ERR_INVALID_ARG;
#endif
}

}  // namespace sd
