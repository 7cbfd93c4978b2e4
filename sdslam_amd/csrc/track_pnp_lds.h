// LDS address maps of k_pnp's EPnP work areas.  Plain C++ (no HIP): track_pnp.hip addresses its LDS through these functions
// and tests/native/pnp_lds_check.cpp walks every step of the Jacobi sweeps through them on the host, so the two cannot disagree.
#pragma once

#ifndef PNP_CHUNK
#define PNP_CHUNK 8    // RANSAC hypotheses evaluated side by side (typical runs accept within the first few);
                       // 3 lanes per hypothesis (one per EPnP beta variant)
#endif

namespace sd {
namespace pnp_lds {

// ---- the 12 x 12 Gram / singular-vector matrix `ut` and its squared row norms W, PNP_CHUNK matrices side by side -------------
// Element (row, k) of hypothesis h lies at double index  (row * 13 + k) * PNP_CHUNK + ((h + row) % PNP_CHUNK);  W[row] is the
// 13th element (k = 12) of its row, so matrix + W take the 156 elements per hypothesis they always took.
//
// Why: the sweeps (jacobi_sweeps12_coop) run lane g * PNP_CHUNK + h on pair g of anti-diagonal `st` of hypothesis h:
// rows i = max(0, st - 11) + g and j = st - i, i.e. in one LDS instruction the lanes g = 0..5 of a hypothesis touch CONSECUTIVE
// rows at the same k.  An LDS bank is 4 bytes, a double covers two; call the pair a slot: slot = double index mod 32 for
// ds_read_b64 (serviced in lane groups {0-31}, {32-63}), double index mod 16 for ds_write_b64 / ds_read2_b64 (groups of 16
// consecutive lanes).  With the unpadded stride (row * 12 + k) * 8 + h the slot is (8 k + h) mod 32 whatever the row: the four
// rows of a 32-lane group collide (4-way ds_read_b64; 2-way for the ds_read2_b64 the compiler emits today and for the stores),
// and the refit, whose six lanes share ONE matrix (h = 0), is 6-way.
// Here the slot is (8 (row + k) + (h + row) % 8) mod 32:
//   * chunk (h = 0..7, four consecutive rows per 32-lane group, two per 16-lane group): a row owns the eight slots
//     [8 (row + k) mod 32, + 8), permuted by h; consecutive rows own different eights              -> conflict-free;
//   * refit (h = 0, six consecutive rows in one group): slot (8 (row + k) + row % 8) mod 32 resp. mod 16 -- the rotation moves
//     rows r and r + 4 (r and r + 2 for the stores), which share an eight, to different slots inside it -> conflict-free.
// Worst case over all 21 steps, k = 0..12, both rows of a pair, reads and writes, any number of active hypotheses: 1 (no
// conflict); pnp_lds_check.cpp enumerates it (and shows 4 / 6 for the unpadded map).  The rotation by row is one add + and per
// row pointer; the 13 elements of a row keep compile-time offsets.
constexpr int kMatRow = 13;                   // elements per row: 12 matrix entries + W
constexpr int kMatElems = 12 * kMatRow;       // per hypothesis
constexpr int kMatW = 12;                     // W[row] = element (row, kMatW)
constexpr int mat_index(int row, int k, int h) { return (row * kMatRow + k) * PNP_CHUNK + (int)((unsigned)(h + row) % PNP_CHUNK); }
constexpr int kWorkDoubles = PNP_CHUNK * kMatElems;   // s_work

// ---- the call-local scratch area s_scr (doubles) ----------------------------------------------------------------------------
// epnp_minimal:  [0, kMrows)            rows of M of the chunk's minimal sets, consumed by the M^T M pass BEFORE the SVD; after
//                                       it the same doubles hold
//                [kPark, + kParkSize)   the barycentric coordinates of each hypothesis (16 per hypothesis, lane-interleaved) and
//                [kL, + kLSize)         L (6 x 10 per hypothesis, lane-interleaved), written after the SVD.
// epnp_refit_wave: [kTerms, + 576) ordered-sum terms / M^T M staging, [kMtm, + 144) M^T M, [kRed, + 64) reduction and broadcast
//                slots.  The refit's L (hypothesis 0's view of [kRefitL, + kLSize)) lies inside the terms area: it is written after
//                the SVD, when the M^T M staging is over, and last read by epnp_betas, before the first ordered sum that follows;
//                mtm (copied to ut before the SVD) and red (live all the time) stay outside it.
constexpr int kMrows = PNP_CHUNK * 4 * 24;
constexpr int kPark = 0, kParkSize = PNP_CHUNK * 16;
constexpr int kLElems = 60, kLSize = kLElems * PNP_CHUNK;
constexpr int kL = kPark + kParkSize;
constexpr int kTerms = 0, kTermsSize = 64 * 9;
constexpr int kMtm = kTerms + kTermsSize, kMtmSize = 144;
constexpr int kRed = kMtm + kMtmSize, kRedSize = 64;
constexpr int kRefitL = kTerms;
constexpr int kRefitScr = kRed + kRedSize;
constexpr int kScrDoubles = kMrows > kRefitScr ? kMrows : kRefitScr;
static_assert(kL + kLSize <= kMrows, "park + L reuse the M-row area");
static_assert(kRefitL >= kTerms && kRefitL + kLSize <= kTerms + kTermsSize, "the refit's L lies inside the (then idle) terms area");
static_assert(kRefitL + kLSize <= kMtm && kMtm + kMtmSize <= kRed, "the refit's L, mtm and red do not overlap");

}  // namespace pnp_lds
}  // namespace sd
