// Dynamic-LDS layouts of the matcher kernels (track_match.hip, track_bf.hip, track_tri.hip): one struct per kernel, built from the launch's
// capacities.  The kernel carves its pointers from the struct (lds_at, track_match_dev.h) and the launcher passes .bytes, so the two cannot
// disagree.  Plain C++ (no HIP): tests/native/match_lds_check.cpp sweeps every capacity on the host.
#pragma once
#include <stdint.h>

namespace sd {

#ifndef MT_LIST_CAP
#define MT_LIST_CAP 4096   // candidate keys per frame kept in LDS (more: per-point slow path)
#endif
#define GRID_COLS 64
#define GRID_ROWS 48
#define GRID_CSTART (GRID_COLS * GRID_ROWS + 2)   // first sorted position of every cell, one past the last, one spare
#define HISTO_LENGTH 30
#define BF_K 4          // smallest keys kept per currentKF point
#define BF_TILE 512     // pKF descriptors per LDS tile (16 KB)

// Base of every layout: take() appends an array at the next multiple of its element size (the only place alignment is
// handled) and returns its byte offset; `bytes` is the total so far.  constexpr: usable on the host and in kernels.
struct LdsLayout {
  uint32_t bytes = 0;
  template <typename T>
  constexpr uint32_t take(uint32_t n) {
    bytes += (0u - bytes) & ((uint32_t)sizeof(T) - 1u);
    const uint32_t off = bytes;
    bytes += n * (uint32_t)sizeof(T);
    return off;
  }
};

// KP2 = power of two >= keypoint capacity, MP = max_points; (MP + 31) / 32 mask words hold one bit per point
struct LdsMatch : LdsLayout {   // k_match
  uint32_t key = 0, list = 0, pt = 0, kang = 0, obs = 0, valid = 0, match = 0, ev = 0, cstart = 0, hist = 0, nlist = 0;
  constexpr LdsMatch(int KP2, int MP) {
    key = take<uint32_t>(KP2);                     // sorted (cell << 11 | index)
    list = take<uint32_t>(MT_LIST_CAP);            // candidate keys
    pt = take<uint32_t>(MP);                       // offset << 16 | count of every point's keys
    kang = take<float>(KP2);                       // keypoint angles
    obs = take<uint32_t>((MP + 31) >> 5);          // bit m: point m has Observations() > 0
    valid = take<uint32_t>((MP + 31) >> 5);
    match = take<int16_t>(KP2);                    // CurrentFrame.mvpMapPoints
    // one entry per ASSIGNMENT (rotHist[bin].push_back), a keypoint may be assigned again: up to n_last <= MP entries
    ev = take<uint16_t>(KP2 > MP ? KP2 : MP);
    cstart = take<uint16_t>(GRID_CSTART);
    hist = take<int32_t>(HISTO_LENGTH);
    nlist = take<int32_t>(1);
  }
};

struct LdsMatchCand : LdsLayout {   // k_match_cand
  uint32_t key = 0, off = 0, cnt = 0, valid = 0, cstart = 0;
  constexpr LdsMatchCand(int KP2, int MP) {
    key = take<uint32_t>(KP2);
    off = take<uint32_t>(MP);                      // exclusive prefix of the counts (may exceed the list)
    cnt = take<uint16_t>(MP);                      // 0xFFFF: window too large for the 11-bit order field
    valid = take<uint32_t>((MP + 31) >> 5);
    cstart = take<uint16_t>(GRID_CSTART);
  }
};

struct LdsMatchAssign : LdsLayout {   // k_match_assign, k_match_assign_retry
  uint32_t ev = 0, obs = 0, hist = 0, match = 0;
  constexpr LdsMatchAssign(int KP2, int MP) {
    ev = take<uint32_t>(MP);                       // one entry per ASSIGNMENT (rotHist[bin].push_back): <= n_last
    obs = take<uint32_t>((MP + 31) >> 5);
    hist = take<int32_t>(HISTO_LENGTH + 2);
    match = take<int16_t>(KP2);                    // -1 | point index | 0x4000 where that point has observations
  }
};

struct LdsMatchLocal : LdsLayout {   // k_match_local; the seen-point exclusion borrows `list` for KP2 ids
  uint32_t key = 0, list = 0, pt = 0, obs = 0, kclaim = 0, match = 0, cstart = 0, koct = 0, nlist = 0;
  constexpr LdsMatchLocal(int KP2, int MP) {
    key = take<uint32_t>(KP2);
    list = take<uint32_t>(MT_LIST_CAP);
    pt = take<uint32_t>(MP);
    obs = take<uint32_t>((MP + 31) >> 5);
    kclaim = take<uint32_t>(KP2 >> 5);             // bit idx: keypoint idx already held a point with observations
    match = take<int16_t>(KP2);
    cstart = take<uint16_t>(GRID_CSTART);
    koct = take<uint8_t>(KP2);                     // keypoint octaves
    nlist = take<int32_t>(1);
  }
};

struct LdsFeaturesInArea : LdsLayout {   // k_features_in_area
  uint32_t key = 0, list = 0, cstart = 0;
  constexpr explicit LdsFeaturesInArea(int KP2) {
    key = take<uint32_t>(KP2);
    list = take<uint32_t>(KP2);
    cstart = take<uint16_t>(GRID_CSTART);
  }
};

struct LdsSeenIds : LdsLayout {   // k_seen_ids
  uint32_t ids = 0;
  constexpr explicit LdsSeenIds(int KP2) {
    ids = take<uint32_t>(KP2);
  }
};

struct LdsSearchPoints : LdsLayout {   // k_search_points; capw = keypoint capacity rounded up to 64
  uint32_t tile = 0, list = 0, i1 = 0, match = 0, v2 = 0, m2 = 0, hist = 0, n1v = 0;
  constexpr explicit LdsSearchPoints(int capw) {
    tile = take<uint32_t>(BF_TILE * 8);            // one tile of pKF descriptors
    list = take<uint32_t>(capw * BF_K);            // the BF_K smallest keys of every currentKF point
    i1 = take<uint16_t>(capw);                     // currentKF points with a map point, ascending
    match = take<int16_t>(capw);
    v2 = take<uint32_t>(capw >> 5);                // bit j: pKF point j has a map point
    m2 = take<uint32_t>(capw >> 5);                // bit j: pKF point j is given away (vbMatched2)
    hist = take<int32_t>(32);
    n1v = take<int32_t>(1);
  }
};

struct LdsQuad { uint32_t w[4]; };   // 16 bytes: what take<> aligns to for arrays read as uint4 / float4

struct LdsSearchTri : LdsLayout {   // k_search_triangulation; capw = keypoint capacity rounded up to 64
  uint32_t tile = 0, aux = 0, i1 = 0, match = 0, elig = 0, erej = 0, hist = 0, n1v = 0;
  constexpr explicit LdsSearchTri(int capw) {
    tile = take<LdsQuad>(BF_TILE * 2);             // one tile of KF2 descriptors
    aux = take<LdsQuad>(BF_TILE);                  // ... and per keypoint x, y, 3.84 * mvLevelSigma2[octave] rounded up, 0
    i1 = take<uint16_t>(capw);                     // KF1 rows without a map point, ascending
    match = take<int16_t>(capw);
    elig = take<uint32_t>(capw >> 5);              // bit j: KF2 keypoint j exists and holds no map point
    erej = take<uint32_t>(capw >> 5);              // bit j: ... is mono and inside the epipole's radius (rejects mono rows)
    hist = take<int32_t>(32);
    n1v = take<int32_t>(1);
  }
};

struct LdsFuse : LdsLayout {   // k_fuse (track_fuse.hip)
  uint32_t key = 0, cstart = 0, pose = 0, nfound = 0;
  constexpr explicit LdsFuse(int KP2) {
    key = take<uint32_t>(KP2);                     // sorted (cell << 11 | index) of the keyframe's keypoints
    cstart = take<uint16_t>(GRID_CSTART);
    pose = take<double>(16);                       // Rcw row-major, tcw, Ow (15 used)
    nfound = take<int32_t>(1);
  }
};

}  // namespace sd
