// Host check of the append result's lifetime (sdslam_amd/csrc/track_results.h), beside result_stamps_check.cpp (the five older
// results and the rows of kEnds) and refresh_stamps_check.cpp (the refresh).  Typed in from the interface's text
// (include/sdslam_hip.h), NOT read from the table: which entry point ends the append's result, what an append ends, what
// mark_flags ends besides, and that no change of an input ends it.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "track_results.h"

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

static const ResultInputs kIn = {7, 11, -1};

static Results all_set(int kf_side) {
  Results r;
  r.pnp.set(3, BIND_PNP, kIn);
  r.sim3.set(3, BIND_SIM3, kIn);
  r.tri.set(3, BIND_TRI, kIn, 0);
  r.triang.set(3, BIND_TRIANG, kIn);
  r.fuse.set(3, bind_fuse(kf_side), kIn, kf_side);
  r.refresh.set(1, BIND_REFRESH, kIn, 40);
  r.append.set(3, BIND_APPEND, kIn, 3);
  return r;
}

// 1: ends it
struct Expect { const char* entry; int append, fuse, refresh, tri, triang, sim3, pnp; };
static const Expect kExpect[] = {
    {"sd_track_append_new_points", 1, 1, 1, 0, 0, 0, 0},
    {"sd_track_append_new_points(mark_flags)", 1, 1, 1, 1, 1, 1, 0},
    {"sd_track_triangulate", 1, 0, 0, 0, 0, 0, 0},
    {"sd_track_set_local", 1, 1, 1, 0, 0, 0, 0},
    {"sd_track_set_local_view", 1, 1, 0, 0, 0, 0, 0},
    {"sd_track_refresh_points(write_local)", 1, 1, 1, 0, 0, 0, 0},
    {"sd_track_refresh_points", 0, 0, 1, 0, 0, 0, 0},
    {"sd_track_set_point_flags", 0, 0, 0, 1, 1, 1, 0},
    {"sd_track_fuse", 0, 1, 0, 0, 0, 0, 0},
    {"sd_track_set_poses", 0, 1, 1, 1, 1, 1, 0},
    {"sd_track_set_camera", 0, 1, 0, 0, 1, 0, 0},
    {"sd_track_search_for_triangulation", 0, 0, 0, 1, 1, 0, 0},
    {"sd_track_set_tri_depth", 0, 0, 0, 0, 1, 0, 0},
    {"sd_track_advance", 0, 0, 0, 0, 0, 0, 1},
};

int main() {
  int cells = 0;
  for (const Expect& x : kExpect)
    for (int kf_side = 0; kf_side < 2; kf_side++, cells++) {
      const int mask = ends_of(x.entry);
      CHECK(mask >= 0, "%s has no row", x.entry);
      Results r = all_set(kf_side);
      CHECK(r.append.live(3, kIn) && r.append.payload == 3, "not live after set()");
      end_results(r, (unsigned)mask);
      CHECK(r.append.live(3, kIn) == !x.append, "append after %s", x.entry);
      CHECK(r.fuse.live(3, kIn) == !x.fuse, "fuse after %s", x.entry);
      CHECK(r.refresh.live(1, kIn) == !x.refresh, "refresh after %s", x.entry);
      CHECK(r.tri.live(3, kIn) == !x.tri, "tri after %s", x.entry);
      CHECK(r.triang_live(3, kIn) == !x.triang, "triang after %s", x.entry);
      CHECK(r.sim3.live(3, kIn) == !x.sim3, "sim3 after %s", x.entry);
      CHECK(r.pnp.live(3, kIn) == !x.pnp, "pnp after %s", x.entry);
    }
  // every row of any table that names R_APPEND is expected above, and the append's own table has no other row
  const EndsRow* tables[3] = {kEnds, kEndsRefresh, kEndsAppend};
  const size_t sizes[3] = {sizeof(kEnds) / sizeof(kEnds[0]), sizeof(kEndsRefresh) / sizeof(kEndsRefresh[0]),
                           sizeof(kEndsAppend) / sizeof(kEndsAppend[0])};
  for (int t = 0; t < 3; t++)
    for (size_t i = 0; i < sizes[t]; i++) {
      const EndsRow& row = tables[t][i];
      bool expected = false, found = false;
      for (const Expect& x : kExpect) {
        found = found || std::strcmp(x.entry, row.entry) == 0;
        expected = expected || (std::strcmp(x.entry, row.entry) == 0 && x.append);
      }
      CHECK(((row.mask & R_APPEND) != 0) == expected, "row %s", row.entry);
      CHECK(t < 2 || (found && (row.mask & R_APPEND)), "kEndsAppend row %s", row.entry);
    }
  CHECK(ends_of("sd_track_append_new_points") == ends_of("sd_track_set_local"), "append = set_local");
  CHECK(ends_of("sd_track_append_new_points(mark_flags)") == (ends_of("sd_track_set_local") | ends_of("sd_track_set_point_flags")),
        "mark_flags = set_local + set_point_flags");
  // a record of what went into the rows: no changed input ends it, nor the extractors' role swap; an empty stamp is not live
  for (int change = 0; change < 3; change++, cells++) {
    Results r = all_set(0);
    ResultInputs now = kIn;
    if (change == 0) now.cur_serial++;
    if (change == 1) now.ref_serial++;
    if (change == 2) now.bcast = 0;
    CHECK(r.append.live(3, now), "append ended by change %d", change);
  }
  {
    Results r = all_set(0);
    r.swap_roles();
    CHECK(r.append.live(3, kIn) && !r.append.live(4, kIn) && !Results{}.append.live(1, kIn), "swap / slots / empty");
  }
  {   // "appended" is the triangulation's payload: a new triangulation starts at 0, and the flag goes with the stamp
    Results r = all_set(0);
    r.triang.payload = 1;
    r.triang.set(3, BIND_TRIANG, kIn);
    CHECK(r.triang.payload == 0, "a new triangulation has not been appended");
    r.triang.payload = 1;
    end_results(r, R_TRI);
    CHECK(r.triang.payload == 0 && r.triang.n == 0, "ended with the search");
  }
  std::printf("append_stamps_check OK (%d cells)\n", cells);
  return 0;
}
