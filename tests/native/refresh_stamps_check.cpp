// Host check of the refresh result's lifetime (sdslam_amd/csrc/track_results.h), beside result_stamps_check.cpp, whose matrix
// covers the five older results and the rows of kEnds.  Typed in from the interface's text (include/sdslam_hip.h), NOT read from
// the table: which entry point ends the refresh result, what a write-through ends besides, that write_local = 0 ends nothing
// else, and which change of an input ends it.
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
  r.tri.set(3, BIND_TRI, kIn, 1);
  r.triang.set(3, BIND_TRIANG, kIn);
  r.fuse.set(3, bind_fuse(kf_side), kIn, kf_side);
  r.refresh.set(1, BIND_REFRESH, kIn, 40);
  return r;
}

struct Expect { const char* entry; int refresh, fuse, others; };   // 1: ends it; others = PnP, Sim3, tri, triang
static const Expect kExpect[] = {
    {"sd_track_set_observations", 1, 0, 0},
    {"sd_track_refresh_points", 1, 0, 0},
    {"sd_track_refresh_points(write_local)", 1, 1, 0},
    {"sd_track_set_local", 1, 1, 0},
    {"sd_track_set_poses", 1, 1, -1},      // (the others: result_stamps_check.cpp)
    {"sd_track_set_local_view", 0, 1, 0},
    {"sd_track_set_camera", 0, 1, -1},
    {"sd_track_fuse", 0, 1, 0},
    {"sd_track_set_uright", 0, 1, -1},
    {"sd_track_set_rand", 0, 0, -1},
    {"sd_track_match", 0, 0, -1},
    {"sd_track_advance", 0, 0, -1},
    {"sd_track_search_for_triangulation", 0, 0, -1},
};

int main() {
  int cells = 0;
  for (const Expect& x : kExpect)
    for (int kf_side = 0; kf_side < 2; kf_side++, cells++) {
      const int mask = ends_of(x.entry);
      CHECK(mask >= 0, "%s has no row", x.entry);
      Results r = all_set(kf_side);
      CHECK(r.refresh.live(1, kIn) && r.refresh.payload == 40, "not live after set()");
      end_results(r, (unsigned)mask);
      CHECK(r.refresh.live(1, kIn) == !x.refresh, "refresh after %s", x.entry);
      CHECK(r.fuse.live(3, kIn) == !x.fuse, "fuse after %s", x.entry);
      if (x.others == 0)
        CHECK(r.pnp.live(3, kIn) && r.sim3.live(3, kIn) && r.tri.live(3, kIn) && r.triang_live(3, kIn), "%s ends an older result", x.entry);
    }
  // every row of either table that names R_REFRESH is expected above, and the refresh's own table has no other row
  for (const EndsRow& row : kEnds) {
    bool expected = false;
    for (const Expect& x : kExpect) expected = expected || (std::strcmp(x.entry, row.entry) == 0 && x.refresh);
    CHECK(((row.mask & R_REFRESH) != 0) == expected, "kEnds row %s", row.entry);
  }
  for (const EndsRow& row : kEndsRefresh) {
    bool found = false;
    for (const Expect& x : kExpect) found = found || std::strcmp(x.entry, row.entry) == 0;
    CHECK(found && (row.mask & R_REFRESH), "kEndsRefresh row %s", row.entry);
  }
  CHECK(ends_of("sd_track_refresh_points(write_local)") == (ends_of("sd_track_set_local") | (int)R_REFRESH), "write-through = set_local");
  // inputs: a new extraction on either side and another broadcast setting end it
  for (int change = 0; change < 3; change++, cells++) {
    Results r = all_set(0);
    ResultInputs now = kIn;
    if (change == 0) now.cur_serial++;
    if (change == 1) now.ref_serial++;
    if (change == 2) now.bcast = 0;
    CHECK(!r.refresh.live(1, now), "refresh survives change %d", change);
  }
  {   // the extractors' role swap of sd_track_advance does not touch it; an empty stamp is not live
    Results r = all_set(0);
    r.swap_roles();
    CHECK(r.refresh.live(1, kIn) && !Results{}.refresh.live(1, kIn), "swap / empty");
  }
  std::printf("refresh_stamps_check OK (%d cells)\n", cells);
  return 0;
}
