// Host check of the cached results' lifetimes (sdslam_amd/csrc/track_results.h), plain C++ and built once more with
// AddressSanitizer and UBSan.  The matrix below is typed in from the behaviour of the entry points, NOT read from the header's
// table: for every (result, entry point) the stamp is set, must be live, the entry point's row is applied, and the result must
// have ended or survived as the matrix says.  Then the bindings: which change of an extraction serial or of the broadcast
// setting ends which result, the slot count, TRI taking TRIANG with it, and the extractors' role swap of sd_track_advance.
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "track_results.h"

using namespace sd;

#define CHECK(cond, ...)                       \
  do {                                         \
    if (!(cond)) {                             \
      std::printf("FAILED %s: ", #cond);       \
      std::printf(__VA_ARGS__);                \
      std::printf("\n");                       \
      std::exit(1);                            \
    }                                          \
  } while (0)

typedef ResultInputs Inputs;   // the handle's inputs, as plain values
static const Inputs kInputs = {7, 11, -1};

enum { PNP, SIM3, TRI, TRIANG, FUSE, N_RESULTS };
static const char* const kResultName[N_RESULTS] = {"PNP", "SIM3", "TRI", "TRIANG", "FUSE"};

static void set_all(Results& r, const Inputs& in, int n, int kf_side) {
  r.pnp.set(n, BIND_PNP, in);
  r.sim3.set(n, BIND_SIM3, in);
  r.tri.set(n, BIND_TRI, in, 1);
  r.triang.set(n, BIND_TRIANG, in);
  r.fuse.set(n, bind_fuse(kf_side), in, kf_side);
}
static bool is_live(const Results& r, int which, const Inputs& in, int n) {
  switch (which) {
    case PNP: return r.pnp.live(n, in);
    case SIM3: return r.sim3.live(n, in);
    case TRI: return r.tri.live(n, in);
    case TRIANG: return r.triang_live(n, in);
    default: return r.fuse.live(n, in);
  }
}

// 1: the entry point ends the result, 0: the result survives it.  (A row that ends TRI ends TRIANG.)
struct Expect {
  const char* entry;
  int ends[N_RESULTS];   // PNP SIM3 TRI TRIANG FUSE
};
static const Expect kExpect[] = {
    {"sd_track_set_camera", {0, 0, 0, 1, 1}},
    {"sd_track_set_poses", {0, 1, 1, 1, 1}},
    {"sd_track_set_rand", {1, 1, 0, 0, 0}},
    {"sd_track_set_last", {1, 0, 0, 0, 0}},
    {"sd_track_set_matches", {1, 0, 0, 0, 0}},
    {"sd_track_match", {1, 0, 0, 0, 0}},
    {"sd_track_with_motion_model", {1, 0, 0, 0, 0}},
    {"sd_track_stereo_init", {1, 0, 0, 0, 0}},
    {"sd_track_advance", {1, 0, 0, 0, 0}},
    {"sd_track_set_local", {0, 0, 0, 0, 1}},
    {"sd_track_set_local_view", {0, 0, 0, 0, 1}},
    {"sd_track_set_uright", {0, 0, 1, 1, 1}},
    {"sd_track_set_uright_ref", {0, 0, 1, 1, 1}},
    {"sd_track_stereo_from_depth", {0, 0, 1, 1, 0}},
    {"sd_track_stereo_from_depth_device", {0, 0, 1, 1, 0}},
    {"sd_track_set_point_flags", {0, 1, 1, 1, 0}},
    {"sd_track_search_by_points", {0, 1, 0, 0, 0}},
    {"sd_track_set_sim3_points", {0, 1, 0, 0, 0}},
    {"sd_track_set_point_matches", {0, 1, 0, 0, 0}},
    {"sd_track_sim3", {0, 1, 0, 0, 0}},
    {"sd_track_set_f12", {0, 0, 1, 1, 0}},
    {"sd_track_search_for_triangulation", {0, 0, 1, 1, 0}},
    {"sd_track_set_tri_depth", {0, 0, 0, 1, 0}},
    {"sd_track_set_tri_median_depth", {0, 0, 0, 1, 0}},
    {"sd_track_set_fuse_scw", {0, 0, 0, 0, 1}},
    {"sd_track_fuse", {0, 0, 0, 0, 1}},
};

int main() {
  const Inputs in = kInputs;
  const int n = 3;
  // the matrix, both ways: every expected row is in the table and behaves, and the table has no row the matrix lacks
  int cells = 0;
  for (const Expect& x : kExpect) {
    const int mask = ends_of(x.entry);
    CHECK(mask >= 0, "%s has no row in kEnds", x.entry);
    for (int kf_side = 0; kf_side < 2; kf_side++)
      for (int which = 0; which < N_RESULTS; which++, cells++) {
        Results r;
        set_all(r, in, n, kf_side);
        CHECK(is_live(r, which, in, n), "%s is not live after set()", kResultName[which]);
        end_results(r, (unsigned)mask);
        CHECK(is_live(r, which, in, n) == !x.ends[which], "%s after %s: expected %s", kResultName[which], x.entry,
              x.ends[which] ? "ended" : "live");
      }
  }
  for (const EndsRow& row : kEnds) {
    bool found = false;
    for (const Expect& x : kExpect) found = found || std::strcmp(x.entry, row.entry) == 0;
    CHECK(found, "kEnds row %s is not in the expected matrix", row.entry);
  }
  CHECK(ends_of("sd_track_align") == -1, "a name without a row must be reported");

  {   // TRI takes TRIANG with it; TRIANG alone leaves TRI
    Results r;
    set_all(r, in, n, 0);
    end_results(r, R_TRIANG);
    CHECK(is_live(r, TRI, in, n) && !is_live(r, TRIANG, in, n), "R_TRIANG alone");
    set_all(r, in, n, 0);
    end_results(r, R_TRI);
    CHECK(!is_live(r, TRI, in, n) && !is_live(r, TRIANG, in, n), "R_TRI takes R_TRIANG");
    CHECK(r.triang.n == 0, "R_TRI clears the triangulation's own stamp");
  }

  // what a changed input ends: {cur serial, ref serial, broadcast} x kf_side -> PNP SIM3 TRI TRIANG FUSE
  static const int kChange[3][2][N_RESULTS] = {
      {{1, 1, 1, 1, 1}, {1, 1, 1, 1, 0}},   // cur re-extracted: a side-1 Fuse result survives, a side-0 one does not
      {{0, 1, 1, 1, 0}, {0, 1, 1, 1, 1}},   // ref re-extracted (TRIANG goes with TRI)
      {{0, 1, 1, 1, 1}, {0, 1, 1, 1, 1}},   // broadcast setting changed: PnP survives
  };
  for (int change = 0; change < 3; change++)
    for (int kf_side = 0; kf_side < 2; kf_side++) {
      Results r;
      set_all(r, in, n, kf_side);
      Inputs now = in;
      if (change == 0) now.cur_serial++;
      if (change == 1) now.ref_serial++;
      if (change == 2) now.bcast = 0;
      for (int which = 0; which < N_RESULTS; which++, cells++)
        CHECK(is_live(r, which, now, n) == !kChange[change][kf_side][which], "%s after change %d (kf_side %d)", kResultName[which],
              change, kf_side);
    }

  {   // slots: live(n + 1) fails after set(n), fewer slots pass, an empty stamp covers nothing
    Results r;
    set_all(r, in, n, 0);
    for (int which = 0; which < N_RESULTS; which++) {
      CHECK(!is_live(r, which, in, n + 1), "%s covers n + 1", kResultName[which]);
      CHECK(is_live(r, which, in, 1), "%s does not cover 1", kResultName[which]);
      CHECK(!is_live(Results{}, which, in, 1) && !is_live(Results{}, which, in, 0), "an empty %s is live", kResultName[which]);
    }
    CHECK(r.pnp.covers(n) && !r.pnp.covers(n + 1), "covers");
    CHECK(r.tri.payload == 1 && r.fuse.payload == 0, "payloads");
    // only the triangulation ran on fewer slots than the search
    r.triang.set(2, BIND_TRIANG, in);
    CHECK(is_live(r, TRIANG, in, 2) && !is_live(r, TRIANG, in, 3) && is_live(r, TRI, in, 3), "triangulation on fewer slots");
  }

  {   // sd_track_advance swaps the extractors: Sim3 / tri / triang do not answer for the swapped pair, even where the serials
      // happen to agree; a second swap restores them; Fuse follows its side's serial alone; a new set() starts unswapped
    Inputs same = kInputs;
    same.ref_serial = same.cur_serial;
    Results r;
    set_all(r, same, n, 0);
    r.swap_roles();
    CHECK(!is_live(r, SIM3, same, n) && !is_live(r, TRI, same, n) && !is_live(r, TRIANG, same, n), "swapped roles");
    CHECK(is_live(r, FUSE, same, n) && is_live(r, PNP, same, n), "swap_roles touches Sim3, tri and triang only");
    r.sim3.set(n, BIND_SIM3, same);
    CHECK(is_live(r, SIM3, same, n), "set() after a swap");
    r.swap_roles();
    CHECK(is_live(r, TRI, same, n) && is_live(r, TRIANG, same, n) && !is_live(r, SIM3, same, n), "second swap");
  }

  std::printf("result_stamps_check OK (%d cells)\n", cells);
  return 0;
}
