// The lifetime of every result a tracker caches between calls: the PnP and Sim3 solvers an iterate() continues, the
// SearchForTriangulation matches, their triangulation, the Fuse search, the map-point refresh, the append of new points.  One stamp type says what a result was computed on, one
// table says which entry point ends which results.  Plain C++ on plain values (extraction serials, the broadcast setting, slot
// counts), no HIP and no handle: tests/native/result_stamps_check.cpp checks the table and the bindings on the host.
#pragma once

namespace sd {

enum Result : unsigned { R_PNP = 1, R_SIM3 = 2, R_TRI = 4, R_TRIANG = 8, R_FUSE = 16, R_REFRESH = 32, R_APPEND = 64 };

// What a result is bound to: it dies when that extractor extracts again / when the broadcast setting changes
enum Bind : unsigned { BIND_CUR = 1, BIND_REF = 2, BIND_BCAST = 4 };
constexpr unsigned BIND_PNP = BIND_CUR;   // (PnP has no broadcast test; its slot count and its serial fail with a message each)
constexpr unsigned BIND_SIM3 = BIND_CUR | BIND_REF | BIND_BCAST;
constexpr unsigned BIND_TRI = BIND_CUR | BIND_REF | BIND_BCAST;
constexpr unsigned BIND_TRIANG = BIND_CUR;   // ... and lives only while the search it triangulated does (Results::triang_live)
constexpr unsigned bind_fuse(int kf_side) { return (kf_side ? BIND_REF : BIND_CUR) | BIND_BCAST; }   // the side it searched

constexpr unsigned BIND_REFRESH = BIND_CUR | BIND_REF | BIND_BCAST;   // observations name frames of both extractors and the cur frame in use
// An append's result is a record of what went into the rows (base / appended / dropped, and the list of the points, which only
// the next triangulation overwrites): no later change of an input makes it wrong, only the entry points of kEnds / kEndsAppend end it
constexpr unsigned BIND_APPEND = 0;

// What a tracker's results are computed on: the serials of the cur and ref extractions, the broadcast setting
struct ResultInputs {
  unsigned long long cur_serial = 0, ref_serial = 0;
  int bcast = -1;
};

// "Slots < n hold a result computed on these inputs."  n == 0: no result.
struct ResultStamp {
  int n = 0;
  unsigned bind = 0;
  ResultInputs on;
  int payload = 0;        // tri: the rotation check ran; triang: its points have been appended to the local rows; Fuse: kf_side;
                          // refresh: the number of points; append: the slots of the triangulation it appended
  // RunStamp::covers compares the `cur` pointer as well.  The pointer changes in one place, sd_track_advance, which swaps the
  // extractors' roles: a Sim3 / tri / triang result does not answer for the swapped pair (Results::swap_roles), and does
  // again once a second advance has swapped them back.  Fuse never compared it: its serial is its side's, whoever holds it.
  bool swapped = false;

  void set(int n_frames, unsigned bind_, const ResultInputs& now, int payload_ = 0) { *this = ResultStamp{n_frames, bind_, now, payload_, false}; }
  bool covers(int n_frames) const { return n > 0 && n_frames <= n; }
  // The result for slots < n_frames is still the one its inputs describe
  bool live(int n_frames, const ResultInputs& now) const {
    return covers(n_frames) && !swapped && (!(bind & BIND_CUR) || now.cur_serial == on.cur_serial) &&
           (!(bind & BIND_REF) || now.ref_serial == on.ref_serial) && (!(bind & BIND_BCAST) || now.bcast == on.bcast);
  }
};

struct Results {
  ResultStamp pnp, sim3, tri, triang, fuse, refresh, append;
  bool triang_live(int n_frames, const ResultInputs& now) const { return tri.live(n_frames, now) && triang.live(n_frames, now); }
  void swap_roles() { sim3.swapped ^= true, tri.swapped ^= true, triang.swapped ^= true; }
};

// Something the results in `mask` were computed from is being replaced: their consumers refuse until the stage runs again
inline void end_results(Results& r, unsigned mask) {
  if (mask & R_TRI) mask |= R_TRIANG;   // the triangulation of those matches goes with them
  if (mask & R_PNP) r.pnp = ResultStamp{};
  if (mask & R_SIM3) r.sim3 = ResultStamp{};
  if (mask & R_TRI) r.tri = ResultStamp{};
  if (mask & R_TRIANG) r.triang = ResultStamp{};
  if (mask & R_FUSE) r.fuse = ResultStamp{};
  if (mask & R_REFRESH) r.refresh = ResultStamp{};
  if (mask & R_APPEND) r.append = ResultStamp{};
}

// What each entry point ends, and why.  An entry point calls end_results with its own row and nothing else (END_RESULTS).
struct EndsRow { const char* entry; unsigned mask; };
constexpr EndsRow kEnds[] = {
    {"sd_track_set_camera", R_FUSE | R_TRIANG},           // a Fuse result was projected with the old K and image bounds, a triangulation used K and mbf
    {"sd_track_set_poses", R_SIM3 | R_TRI | R_FUSE | R_REFRESH},   // the Sim3 solvers' keyframe poses; the poses F12 and the epipole came from; Fuse's keyframe pose; the refresh's camera centres
    {"sd_track_set_rand", R_PNP | R_SIM3},                // a resumed iterate() continues at a position of the OLD stream
    {"sd_track_set_last", R_PNP},                         // the solvers' 3-D points are being replaced
    {"sd_track_set_matches", R_PNP},                      // the saved best-inlier mask indexes the old correspondence list
    {"sd_track_match", R_PNP},                            // mvpMapPoints is rewritten: solvers built on the old vector cannot be continued
    {"sd_track_with_motion_model", R_PNP},                // ... likewise
    {"sd_track_stereo_init", R_PNP},                      // ... likewise
    {"sd_track_advance", R_PNP},                          // ... and `cur` becomes the other extractor
    {"sd_track_set_local", R_FUSE | R_REFRESH | R_APPEND},   // sd_track_fuse reads these rows too; the refresh read Xw of one; an append's positions are overwritten
    {"sd_track_set_local_view", R_FUSE | R_APPEND},       // lm_n and lm_desc are rows sd_track_fuse reads, and an append counted from lm_n
    {"sd_track_set_uright", R_TRI | R_FUSE},              // KF1's stereo bits, and the mvuRight row of a Fuse result's chi-square gate
    {"sd_track_set_uright_ref", R_TRI | R_FUSE},          // KF2's
    {"sd_track_stereo_from_depth", R_TRI},                // mvuRight and mvDepth of KF1 are being replaced
    {"sd_track_stereo_from_depth_device", R_TRI},         // ... likewise
    {"sd_track_set_point_flags", R_SIM3 | R_TRI},         // the Sim3 solvers' validity test, the map-point flags of a SearchForTriangulation result
    {"sd_track_search_by_points", R_SIM3},                // matches12 is rewritten: Sim3 solvers built on the old vector cannot be continued
    {"sd_track_set_point_matches", R_SIM3},               // ... likewise
    {"sd_track_set_sim3_points", R_SIM3},                 // the solvers' 3-D points
    {"sd_track_sim3", R_SIM3},                            // a stage ends its own old result before it runs: a refused or failed call leaves none
    {"sd_track_search_for_triangulation", R_TRI},         // ... likewise
    {"sd_track_fuse", R_FUSE},                            // ... likewise
    {"sd_track_set_f12", R_TRI},                          // the F12 a search with use_set_f12 reads
    {"sd_track_set_tri_depth", R_TRIANG},                 // mvDepth of either side
    {"sd_track_set_tri_median_depth", R_TRIANG},          // the median depth of the monocular baseline gate
    {"sd_track_set_fuse_scw", R_FUSE},                    // the Scw a search with sim3 = 1 projects with
};

// The map-point refresh's own entry points (track_refresh.hip).  A table beside kEnds, not more rows of it:
// tests/native/result_stamps_check.cpp holds kEnds to a matrix typed in when the results were five, and
// tests/native/refresh_stamps_check.cpp holds these rows and the R_REFRESH bits above to one of its own.
constexpr EndsRow kEndsRefresh[] = {
    {"sd_track_set_observations", R_REFRESH},             // the lists the result was computed on
    {"sd_track_refresh_points", R_REFRESH},               // a stage ends its own old result before it runs
    // write_local = 1 rewrites desc, normal and the distances of a local row: whatever a sd_track_set_local on that row ends
    {"sd_track_refresh_points(write_local)", R_FUSE | R_REFRESH | R_APPEND},
};

// The append of new points to the local rows (track_append.hip), a table of its own for the same reason;
// tests/native/append_stamps_check.cpp holds these rows and the R_APPEND bits above to a matrix of its own.
constexpr EndsRow kEndsAppend[] = {
    // it rewrites lm_n and the fields of local rows: whatever a sd_track_set_local on them ends (its own old result among them)
    {"sd_track_append_new_points", R_FUSE | R_REFRESH | R_APPEND},
    // mark_flags = 1 also rewrites the "holds a map point" flags: whatever sd_track_set_point_flags ends besides
    {"sd_track_append_new_points(mark_flags)", R_FUSE | R_REFRESH | R_APPEND | R_SIM3 | R_TRI},
    {"sd_track_triangulate", R_APPEND},                   // the point list sd_track_get_new_points reads after an append is overwritten
};

// The local bundle adjustment (track_ba.hip), a table of its own for the same reason.  Its own result is a record of the run
// (like an append's) and is not in this table; write_back = 0 ends nothing.
constexpr EndsRow kEndsBa[] = {
    // write_back = 1 rewrites Tref / Tcur and Xw of a local row: whatever sd_track_set_poses and a write-through refresh end
    {"sd_track_local_ba(write_back)", R_SIM3 | R_TRI | R_FUSE | R_REFRESH | R_APPEND},
    // ... and so does the global one's (the nLoopKF == 0 branch).  Its own result (mTcwGBA / mPosGBA with write_back = 0) is kept
    // in the same scratch as the local one's, answers only its own getter, and is ended by sd_track_set_poses besides
    {"sd_track_global_ba(write_back)", R_SIM3 | R_TRI | R_FUSE | R_REFRESH | R_APPEND},
};

// The erasure of observations (track_cull.hip), a table of its own for the same reason.  sd_track_cull_keyframes changes nothing
// and ends nothing; its own result and the erase's are records stamped with the lists' serial (RefreshBuffers::serial).
constexpr EndsRow kEndsCull[] = {
    {"sd_track_erase_observations", R_REFRESH},           // the lists the result was computed on are compacted: what an upload ends
};

constexpr bool same_name(const char* a, const char* b) {
  while (*a && *a == *b) ++a, ++b;
  return *a == *b;
}
// The row of `entry`; -1 (no mask) for a name the table does not hold, which END_RESULTS turns into a compile error
constexpr int ends_of(const char* entry) {
  for (const EndsRow& row : kEnds)
    if (same_name(row.entry, entry)) return (int)row.mask;
  for (const EndsRow& row : kEndsRefresh)
    if (same_name(row.entry, entry)) return (int)row.mask;
  for (const EndsRow& row : kEndsAppend)
    if (same_name(row.entry, entry)) return (int)row.mask;
  for (const EndsRow& row : kEndsBa)
    if (same_name(row.entry, entry)) return (int)row.mask;
  for (const EndsRow& row : kEndsCull)
    if (same_name(row.entry, entry)) return (int)row.mask;
  return -1;
}

static_assert(ends_of("sd_track_refresh_points(write_local)") == (ends_of("sd_track_set_local") | (int)R_REFRESH),
              "a write-through ends what sd_track_set_local ends");
static_assert(ends_of("sd_track_append_new_points") == ends_of("sd_track_set_local"), "an append ends what sd_track_set_local ends");
static_assert(ends_of("sd_track_append_new_points(mark_flags)") == (ends_of("sd_track_set_local") | ends_of("sd_track_set_point_flags")),
              "... and with mark_flags what sd_track_set_point_flags ends");
static_assert(ends_of("sd_track_local_ba(write_back)") == (ends_of("sd_track_set_poses") | ends_of("sd_track_refresh_points(write_local)")),
              "a write-back ends what sd_track_set_poses and a write-through refresh end");
static_assert(ends_of("sd_track_erase_observations") == ends_of("sd_track_set_observations"), "an erasure ends what an upload of the lists ends");
static_assert(ends_of("sd_track_global_ba(write_back)") == ends_of("sd_track_local_ba(write_back)"), "... whichever bundle adjustment wrote");

}  // namespace sd
