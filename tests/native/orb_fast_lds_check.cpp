// Host check of the extraction path's flat-index divisions (sdslam_amd/csrc/sd_fastdiv.h), of k_fast_cells' LDS layout
// (orb_fast_lds.h) and of what plan_geometry (orb_plan.cpp) derives from them.  Stand-alone program, linked with orb_plan.cpp and
// sd_options.cpp, built with AddressSanitizer and UBSan by tests/test_host_cpu.py.  Five parts:
//   1. both multiply-high recipes against plain division, up to and just beyond their predicates' bounds
//   2. every geometry the test suite extracts at (typed in below), 1280 x 720 and 1920 x 1080: every cell's layout, every division
//   3. the VGA plan replayed: every index of the four in-kernel loops, row and column by / and % against multiply-high
//   4. a frame with a one-pixel-wide zone is refused with the message it has always had
//   5. the plans are the ones the hand-written formulas gave before the layout header existed (constants recorded then)
#define __HIP_PLATFORM_AMD__ 1
#include <algorithm>
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <thread>
#include <vector>

#include "orb_fast_lds.h"
#include "orb_plan.h"
#include "sd_common.h"

namespace sd {
void set_error(const std::string&) {}   // (sd_options.cpp reports through the library's error slot)
}
using namespace sd;

#define CHECK(cond, ...)                                 \
  do {                                                   \
    if (!(cond)) {                                       \
      std::printf("FAILED %s:%d %s: ", __FILE__, __LINE__, #cond); \
      std::printf(__VA_ARGS__);                          \
      std::printf("\n");                                 \
      std::exit(1);                                      \
    }                                                    \
  } while (0)

// ---- 1. the recipes --------------------------------------------------------------------------------------------------------
template <typename F>
static void dividends(uint32_t d, uint64_t bound, F&& f) {   // 0 ... 2 d, every multiple of d and its neighbours, the bound
  for (uint64_t e = 0; e <= std::min<uint64_t>(2ull * d, bound); e++) f((uint32_t)e);
  for (uint64_t q = 1; q * d <= bound + 1; q++)
    for (uint64_t e = q * d - 1; e <= q * d + 1; e++)
      if (e <= bound) f((uint32_t)e);
  for (uint64_t e = bound > 2 * (uint64_t)d ? bound - 2 * d : 0; e <= bound; e++) f((uint32_t)e);
}

// every dividend 0 ... bound of one divisor; the quotient is counted up, not divided out (2.3e10 dividends in all for d <= 64,
// dealt to a few threads in runs of 2^26).
__attribute__((optimize("O3"))) static bool exhaustive(uint32_t d, uint64_t q_lo, uint64_t q_hi, uint64_t bound, bool odd) {
  const uint64_t m = odd ? fastdiv_magic_odd(d) : fastdiv_magic(d);
  uint64_t wrong = 0;
  for (uint64_t q = q_lo; q < q_hi; q++) {   // the d dividends whose quotient is q
    const uint64_t e0 = q * d, n = std::min<uint64_t>(d, bound + 1 - e0);
    for (uint64_t s = 0; s < n; s++) wrong |= ((((odd ? 2 * (e0 + s) + 1 : e0 + s) * m) >> 32) ^ q);
  }
  return wrong == 0;
}

static long check_exhaustive(uint32_t d_max) {
  struct Job { uint32_t d; uint64_t q_lo, q_hi, bound; bool odd; };
  std::vector<Job> jobs;
  long n = 0;
  auto add = [&](uint32_t d, uint64_t bound, bool odd) {
    const uint64_t nq = bound / d + 1, step = std::max<uint64_t>(1, (1ull << 26) / d);
    for (uint64_t q = 0; q < nq; q += step) jobs.push_back({d, q, std::min(q + step, nq), bound, odd});
    n += (long)bound + 1;
  };
  for (uint32_t d = 1; d <= d_max; d++) {
    if (d >= 2) add(d, ((1ull << 32) - 1) / d, false);
    add(d, d == 1 ? (1ull << 31) - 1 : std::min<uint64_t>((1ull << 31) - 1, ((1ull << 31) / (d - 1) - 1) / 2), true);
  }
  std::atomic<size_t> next{0};
  std::atomic<long> bad{-1};
  std::vector<std::thread> pool;
  for (unsigned t = 0; t < std::min(8u, std::max(1u, std::thread::hardware_concurrency())); t++)
    pool.emplace_back([&] {
      for (size_t j; (j = next.fetch_add(1)) < jobs.size();)
        if (!exhaustive(jobs[j].d, jobs[j].q_lo, jobs[j].q_hi, jobs[j].bound, jobs[j].odd)) bad = (long)j;
    });
  for (std::thread& t : pool) t.join();
  CHECK(bad < 0, "%s recipe, d %u: a wrong quotient among the dividends %llu ... %llu, bound %llu", jobs[bad].odd ? "odd" : "plain", jobs[bad].d,
        (unsigned long long)(jobs[bad].q_lo * jobs[bad].d), (unsigned long long)(jobs[bad].q_hi * jobs[bad].d - 1), (unsigned long long)jobs[bad].bound);
  return n;
}

static long check_recipes() {
  constexpr uint32_t kExhaustive = 64;   // divisors up to here: every dividend; beyond: every multiple and its neighbours
  long n = check_exhaustive(kExhaustive);
  int beyond = 0, beyond_odd = 0;
  for (uint32_t d = 1; d <= 4200; d++) {
    if (d >= 2) {
      const uint64_t bound = ((1ull << 32) - 1) / d;   // largest max_e with max_e * d < 2^32
      CHECK(fastdiv_exact(d, bound) && !fastdiv_exact(d, bound + 1), "d %u", d);
      const uint32_t m = fastdiv_magic(d);
      CHECK((uint64_t)m * d >= (1ull << 32) && (uint64_t)m * d < (1ull << 32) + d, "d %u: the magic is not ceil(2^32 / d)", d);
      if (d > kExhaustive) dividends(d, bound, [&](uint32_t e) { CHECK(fastdiv_apply(e, m) == e / d, "d %u e %u", d, e); n++; });
      // not merely loose: a wrong quotient within 100000 multiples of d beyond the bound, where there is one (remainder d - 1 fails first)
      for (uint64_t e = (bound / d + 1) * d + d - 1, k = 0; k < 100000 && e <= 0xFFFFFFFFull; e += d, k++)
        if (fastdiv_apply((uint32_t)e, m) != (uint32_t)e / d) { beyond++; break; }
    }
    const uint64_t bound = d == 1 ? (1ull << 31) - 1 : std::min<uint64_t>((1ull << 31) - 1, ((1ull << 31) / (d - 1) - 1) / 2);
    CHECK(fastdiv_odd_exact(d, bound) && !fastdiv_odd_exact(d, bound + 1), "odd d %u", d);
    const uint32_t M = fastdiv_magic_odd(d);
    if (d > kExhaustive) dividends(d, bound, [&](uint32_t e) { CHECK(fastdiv_apply_odd(e, M) == e / d, "odd d %u e %u", d, e); n++; });
    for (uint64_t e = (bound / d + 1) * d, k = 0; d > 1 && k < 100000 && e <= (1ull << 31) - 1; e += d, k++)   // remainder 0 fails first
      if (fastdiv_apply_odd((uint32_t)e, M) != (uint32_t)e / d) { beyond_odd++; break; }
  }
  CHECK(!fastdiv_exact(1, 0) && !fastdiv_exact(0, 0) && fastdiv_magic(1) == 0, "a divisor of 1 has no magic number");
  CHECK(fastdiv_odd_exact(1, 0x7FFFFFFFull) && !fastdiv_odd_exact(1, 0x80000000ull) && !fastdiv_odd_exact(0, 0), "odd recipe, d = 1");
  // one counter-example each, worked by hand: d = 3 (3 | 2^32 - 1, and 2^31 = 2 mod 3)
  CHECK(fastdiv_exact(3, 1431655765ull) && fastdiv_apply(0x80000000u, fastdiv_magic(3)) != 0x80000000u / 3, "d 3, e 2^31");
  CHECK(fastdiv_odd_exact(3, 536870911ull) && !fastdiv_odd_exact(3, 536870912ull) &&
        fastdiv_apply_odd(536870913u, fastdiv_magic_odd(3)) != 536870913u / 3, "odd d 3, e 2^29 + 1");
  CHECK(beyond > 1000 && beyond_odd > 1000, "%d / %d divisors with a wrong quotient just beyond the bound", beyond, beyond_odd);
  return n;
}

// ---- 2. the geometries -----------------------------------------------------------------------------------------------------
struct Geo { int nf; float sf; int nl, w, h, merge, kb, whole; };   // merge / kb / whole: "extract.fast_*" options, 0 = default
static const Geo kGeo[] = {
    // tests/geometries.py
    {300, 1.2f, 8, 640, 480, 0, 0, 0}, {300, 1.2f, 8, 637, 479, 0, 0, 0}, {300, 1.2f, 8, 752, 480, 0, 0, 0}, {300, 1.2f, 8, 480, 640, 0, 0, 0},
    {300, 1.5f, 5, 321, 243, 0, 0, 0},
    // tests/test_orb_gpu.py: the two configurations, the edge inputs, the FAST plan options, odd and further geometries
    {1000, 1.2f, 8, 640, 480, 0, 0, 0}, {1000, 2.0f, 5, 640, 480, 0, 0, 0}, {1000, 1.2f, 8, 752, 480, 0, 0, 0},
    {1000, 1.2f, 8, 640, 480, 3, 0, 0}, {1000, 1.2f, 8, 640, 480, 5, 0, 0}, {1000, 1.2f, 8, 640, 480, 8, 0, 0}, {1000, 1.2f, 8, 640, 480, 1, 0, 0},
    {1000, 1.2f, 8, 640, 480, 0, 12, 12},
    {1000, 1.2f, 8, 637, 479, 0, 0, 0}, {500, 1.2f, 6, 321, 242, 0, 0, 0}, {1000, 2.0f, 4, 640, 480, 0, 0, 0}, {800, 1.5f, 5, 486, 360, 0, 0, 0},
    {2000, 1.2f, 8, 1241, 376, 0, 0, 0}, {500, 1.2f, 8, 320, 240, 0, 0, 0}, {1000, 1.2f, 8, 320, 240, 0, 0, 0}, {2000, 1.2f, 8, 1920, 1080, 0, 0, 0}, {1500, 1.3f, 6, 800, 600, 0, 0, 0},
    {1000, 1.1f, 12, 640, 480, 0, 0, 0}, {200, 1.2f, 4, 131, 97, 0, 0, 0},
    // ... test_pyramid_paths_at_their_size_thresholds
    {150, 1.2f, 3, 64, 48, 0, 0, 0}, {150, 1.2f, 3, 67, 47, 0, 0, 0}, {150, 1.2f, 3, 65, 49, 0, 0, 0}, {150, 1.2f, 3, 200, 48, 0, 0, 0},
    {150, 1.2f, 3, 63, 100, 0, 0, 0}, {150, 1.2f, 3, 77, 57, 0, 0, 0}, {150, 1.2f, 3, 66, 120, 0, 0, 0},
    // larger frames (the bench default is the sixth row)
    {1000, 1.2f, 8, 1280, 720, 0, 0, 0}, {1000, 1.2f, 8, 1920, 1080, 0, 0, 0},
};

static void plan(const Geo& g, HostPlan& hp) {
  CHECK(sd_set_option("extract.fast_merge_from", g.merge ? g.merge : 6) == SD_OK && sd_set_option("extract.fast_lds_kb", g.kb ? g.kb : 24) == SD_OK &&
            sd_set_option("extract.fast_lds_whole_kb", g.whole ? g.whole : 40) == SD_OK, "options");
  plan_tables(g.nf, g.sf, g.nl, hp);
  const char* why = "";
  CHECK(plan_geometry(g.nf, g.nl, 20, g.w, g.h, hp, &why), "%d x %d refused: %s", g.w, g.h, why);
}

static bool is_vga(const Geo& g) { return g.nf == 1000 && g.nl == 8 && g.w == 640 && g.h == 480 && !g.merge && !g.kb; }

// ---- 3. one cell at one edge, as the kernel walks it --------------------------------------------------------------------------
static long replay(const CellGeom& c, const LdsFastTile& T) {
  long n = 0;
  const uint32_t m_zw = fastdiv_magic(c.zw), m_tp = fastdiv_magic(T.TP), m_tpu = fastdiv_magic_odd(T.TPU), m_tpw = fastdiv_magic(T.TPW);
  std::vector<uint8_t> lds(T.bytes, 0);   // exact size: the sanitizer sees any index past the layout
  for (int r0 = 0; r0 < c.zh; r0 += c.strip_rows) {
    const int r1 = std::min(r0 + c.strip_rows, c.zh), sr0 = std::max(r0 - 1, 0), sr1 = std::min(r1 + 1, c.zh), nsr = sr1 - sr0, npr = nsr + 6;
    CHECK(nsr <= T.NSR, "strip at row %d scores %d rows, NSR %d", r0, nsr, T.NSR);
    const int nu = T.TPU * npr, ndw = T.TPW * npr;
    for (int tid = 0; tid < kFastThreads; tid++) {
      for (int i0 = tid; i0 < nu; i0 += kFastThreads * (FAST_STAGE_DEPTH / 4))
        for (int j = 0; j < FAST_STAGE_DEPTH / 4; j++, n++) {
          const int i = i0 + kFastThreads * j;
          CHECK((uint64_t)i <= T.div_tpu().max_e && fastdiv_apply_odd(i, m_tpu) == (uint32_t)(i / T.TPU), "unit %d of %d", i, nu);
          if (i < nu) lds[T.tile + 16 * (size_t)i + 15]++;
        }
      for (int i0 = tid; i0 < ndw; i0 += kFastThreads * FAST_STAGE_DEPTH)
        for (int j = 0; j < FAST_STAGE_DEPTH; j++, n++) {
          const int i = i0 + kFastThreads * j;
          CHECK((uint64_t)i <= T.div_tpw().max_e && fastdiv_apply(i, m_tpw) == (uint32_t)(i / T.TPW), "dword %d of %d", i, ndw);
          if (i < ndw) lds[T.tile + 4 * (size_t)i + 3]++;
        }
    }
    CHECK(T.tile + 16 * (size_t)nu <= T.sc, "the strip's tile runs into the score map");
    for (int i = 0; i < (nsr + 2) * T.TPU; i++) lds[T.sc + 16 * (size_t)i + 15]++;
    CHECK(T.sc + 16 * (size_t)(nsr + 2) * T.TPU <= T.queue, "the score map runs into the queues");
    const int rpw = (nsr + 3) >> 2;
    CHECK(rpw <= T.RPW, "rows per wave");
    for (int wave = 0; wave < kFastWaves; wave++) {
      const int y_lo = std::min(wave * rpw, nsr), y_hi = std::min(y_lo + rpw, nsr);
      int qn = 0;
      for (int i = y_lo * c.zw; i < y_hi * c.zw; i++, n++) {
        CHECK((uint64_t)i <= T.div_zw().max_e, "pixel %d", i);
        const uint32_t y = fastdiv_apply(i, m_zw);
        CHECK(y == (uint32_t)(i / c.zw), "pixel %d / %d", i, c.zw);
        const uint32_t ofs = i + y * (T.TP - c.zw), x = i % c.zw;
        CHECK(ofs == y * T.TP + x && ofs < 65536 && ofs <= T.div_tp().max_e, "entry %u", ofs);
        CHECK(fastdiv_apply(ofs, m_tp) == y && ofs - y * T.TP == x, "entry %u / %d", ofs, T.TP);
        // the ring of the pixel lies in the tile, its 3 x 3 score neighbourhood in the score map, its queue slot in the wave's queue
        CHECK(T.tile0 + ofs >= T.tile + 3 * T.TP + 3 && T.tile0 + ofs + 3 * T.TP + 3 < T.sc, "ring of entry %u", ofs);
        CHECK(T.sc0 + ofs >= T.sc + T.TP + 1 && T.sc0 + ofs + T.TP + 1 < T.queue, "scores around entry %u", ofs);
        lds[T.tile0 + ofs]++;
        lds[T.sc0 + ofs]++;
        CHECK(qn < T.QCAP, "queue of wave %d", wave);
        lds[T.queue_of(wave) + 2 * (size_t)qn++ + 1]++;
      }
    }
  }
  return n;
}

// ---- 5. what the plans were before -------------------------------------------------------------------------------------------
static uint64_t fnv(uint64_t h, uint32_t v) {
  for (int i = 0; i < 4; i++) h = (h ^ ((v >> (8 * i)) & 0xff)) * 0x100000001b3ull;
  return h;
}
struct Run { int value, count; };
struct TileRun { int level, nstrips; unsigned magic; int count; };   // `count` tiles of a level, p0 = 0, 16, 32, ...
struct Recorded { std::vector<Run> strips; std::vector<size_t> lds_level; size_t lds_bytes; std::vector<TileRun> tiles; };
static const Recorded kVga = {
    {{74, 25}, {72, 5}, {61, 25}, {57, 5}, {59, 20}, {48, 20}, {49, 9}, {46, 3}, {39, 9}, {38, 3}, {31, 9}, {30, 3}, {24, 12}},
    {40920, 29376, 28432, 19680, 21400, 14160, 9440, 6800},
    40920,
    {{0, 10, 429496730u, 10}, {1, 9, 477218589u, 8}, {2, 7, 613566757u, 5}, {3, 6, 715827883u, 4}, {4, 5, 858993460u, 3}, {5, 5, 858993460u, 3},
     {6, 4, 1073741824u, 2}, {7, 3, 1431655766u, 1}}};
static const Recorded k720 = {
    {{14, 28}, {17, 28}, {22, 28}, {20, 15}, {24, 12}, {26, 3}, {51, 12}, {47, 3}, {24, 6}, {30, 4}, {29, 1}, {33, 1}},
    {23456, 23632, 23728, 24656, 25208, 37720, 24480, 26488},
    37720,
    {{0, 20, 214748365u, 29}, {1, 17, 252645136u, 21}, {2, 14, 306783379u, 14}, {3, 12, 357913942u, 11}, {4, 10, 429496730u, 7},
     {5, 9, 477218589u, 6}, {6, 7, 613566757u, 4}, {7, 6, 715827883u, 3}}};
static const uint64_t kAllPlans = 0x2d04ebc278ca4161ull;   // FNV-1a over every geometry of kGeo in order: strip_rows of every cell,
                                                           // fast_lds_level[0 ... 15], fast_lds_bytes, every BlurTile's four fields

static void check_recorded(const HostPlan& hp, const Recorded& R, const char* name) {
  size_t c = 0;
  for (const Run& r : R.strips)
    for (int k = 0; k < r.count; k++, c++) CHECK(c < hp.cells.size() && hp.cells[c].strip_rows == r.value, "%s: strip_rows of cell %zu", name, c);
  CHECK(c == hp.cells.size(), "%s: %zu cells", name, hp.cells.size());
  for (size_t l = 0; l < SD_MAX_LEVELS; l++)
    CHECK(hp.fast_lds_level[l] == (l < R.lds_level.size() ? R.lds_level[l] : 0), "%s: fast_lds_level[%zu] = %zu", name, l, hp.fast_lds_level[l]);
  CHECK(hp.fast_lds_bytes == R.lds_bytes, "%s: fast_lds_bytes %zu", name, hp.fast_lds_bytes);
  size_t t = 0;
  for (const TileRun& r : R.tiles)
    for (int k = 0; k < r.count; k++, t++) {
      CHECK(t < hp.blur_tiles.size(), "%s: %zu blur tiles", name, hp.blur_tiles.size());
      const BlurTile& b = hp.blur_tiles[t];
      CHECK(b.level == r.level && b.p0 == 16 * k && b.nstrips == r.nstrips && b.magic == r.magic, "%s: blur tile %zu", name, t);
    }
  CHECK(t == hp.blur_tiles.size(), "%s: %zu blur tiles", name, hp.blur_tiles.size());
}

int main() {
  const long n_div = check_recipes();

  long n_cells = 0, n_replayed = 0;
  uint64_t all = 0xcbf29ce484222325ull;
  for (const Geo& g : kGeo) {
    HostPlan hp;
    plan(g, hp);
    const OrbPlan& P = hp.plan;
    for (size_t ci = 0; ci < hp.cells.size(); ci++) {
      const CellGeom& c = hp.cells[ci];
      all = fnv(all, (uint32_t)c.strip_rows);
      if (c.zw <= 0) continue;
      CHECK(c.zw >= 2 && c.zh >= 1 && c.strip_rows >= 1 && c.strip_rows <= c.zh, "%d x %d cell %zu", g.w, g.h, ci);
      const size_t req = hp.fast_lds_level[c.level];
      CHECK(req <= 65536 && req <= hp.fast_lds_bytes, "%d x %d level %d requests %zu bytes", g.w, g.h, c.level, req);
      for (int edge : {0, SD_EDGE}) {
        if (edge == 0 && c.level != 0) continue;
        const LdsFastTile T(c.zx0, c.zw, c.zh, c.strip_rows, edge);
        n_cells++;
        CHECK(T.xa % 16 == 0 && T.sh >= 0 && T.sh < 16 && T.xa + T.sh == c.zx0 - 3 + edge && T.TP == 16 * T.TPU && T.TPW == 4 * T.TPU, "pad");
        // a tile row reaches the last ring column, and stays inside the source row (pyramid pitch / frame width)
        CHECK(T.TP >= T.sh + c.zw + 6 && T.TP < T.sh + c.zw + 6 + 16, "pitch %d", T.TP);
        CHECK(T.xa >= 0 && T.xa + T.TP <= (edge ? P.lv[c.level].pstride : P.w0), "tile row ends at %d", T.xa + T.TP);
        CHECK(T.tile == 0 && T.tile % 16 == 0 && T.sc % 16 == 0 && T.queue % 2 == 0, "alignment");
        CHECK(T.tile + (uint32_t)T.TP * (T.NSR + 6) <= T.sc && T.sc + (uint32_t)T.TP * (T.NSR + 2) <= T.queue, "regions in order");
        for (int w = 0; w < kFastWaves; w++) CHECK(T.queue_of(w) + 2u * T.QCAP <= (w < 3 ? T.queue_of(w + 1) : T.bytes), "queue of wave %d", w);
        CHECK(T.bytes <= (LdsFastTile::worst_pad(c.zw, c.zh, c.strip_rows).bytes + kFastLdsSlack) && (LdsFastTile::worst_pad(c.zw, c.zh, c.strip_rows).bytes + kFastLdsSlack) <= req, "%u bytes of %zu", T.bytes, req);
        CHECK((T.NSR + 1) * T.TP <= 65536 && T.entries_fit16() && T.QCAP <= 4096, "queue entries");
        CHECK(fastdiv_exact(T.div_zw().d, T.div_zw().max_e) && T.div_zw().d == (uint32_t)c.zw, "div_zw");
        CHECK(fastdiv_exact(T.div_tp().d, T.div_tp().max_e) && T.div_tp().d == (uint32_t)T.TP, "div_tp");
        CHECK(fastdiv_odd_exact(T.div_tpu().d, T.div_tpu().max_e) && T.div_tpu().d == (uint32_t)T.TPU, "div_tpu");
        CHECK(fastdiv_exact(T.div_tpw().d, T.div_tpw().max_e) && T.div_tpw().d == (uint32_t)T.TPW, "div_tpw");
        if (is_vga(g)) n_replayed += replay(c, T);
      }
    }
    for (int l = 0; l < SD_MAX_LEVELS; l++) all = fnv(all, (uint32_t)hp.fast_lds_level[l]);
    all = fnv(all, (uint32_t)hp.fast_lds_bytes);
    for (const BlurTile& t : hp.blur_tiles) {
      all = fnv(fnv(fnv(fnv(all, (uint32_t)t.level), (uint32_t)t.p0), (uint32_t)t.nstrips), t.magic);
      const LevelGeom& L = P.lv[t.level];
      CHECK(t.nstrips == (L.w + 63) / 64 && t.p0 % 16 == 0 && t.p0 < t.nstrips * ((L.h + 31) / 32), "blur tile");
      for (int pr = t.p0; pr < t.p0 + 16; pr++)   // the kernel's own branch
        CHECK((t.nstrips == 1 ? (uint32_t)pr : fastdiv_apply(pr, t.magic)) == (uint32_t)(pr / t.nstrips), "pair %d / %d", pr, t.nstrips);
      CHECK(t.nstrips == 1 ? t.magic == 0 : (t.magic == fastdiv_magic(t.nstrips) && fastdiv_exact(t.nstrips, t.p0 + 15)), "blur magic");
    }
    for (int l = 0; l < P.nlevels; l++) {   // both resize kernels' launches, every thread
      const LevelGeom& L = P.lv[l];
      const PyrGroups& D = hp.pyr[l];
      CHECK(D.G == (L.w + 2 * SD_EDGE + 3) / 4 && D.magic == fastdiv_magic(D.G) && D.mirror == (L.h >= 48), "level %d groups", l);
      CHECK(D.Hh * PYR_RPT >= (D.mirror ? L.h : L.prows) && (D.Hh - 1) * PYR_RPT < (D.mirror ? L.h : L.prows), "level %d row slots", l);
      for (int rows : {D.Hh, L.nblk}) {
        const uint64_t threads = 256ull * pyr_blocks(rows, D.G);
        CHECK(threads >= (uint64_t)rows * D.G && fastdiv_exact(D.G, threads ? threads - 1 : 0), "level %d: %llu threads", l, (unsigned long long)threads);
        for (uint64_t e = 0; e < threads; e++) CHECK(fastdiv_apply((uint32_t)e, D.magic) == e / D.G, "level %d thread %llu", l, (unsigned long long)e);
      }
    }
    if (is_vga(g)) check_recorded(hp, kVga, "640 x 480");
    if (g.w == 1280) check_recorded(hp, k720, "1280 x 720");
  }
  CHECK(all == kAllPlans, "checksum of all plans %016llx, recorded %016llx", (unsigned long long)all, (unsigned long long)kAllPlans);
  CHECK(n_replayed > 0, "the VGA plan was not replayed");

  // 4. a zone one pixel wide: 44 x 44 with 500 features on two levels -- level 0 has 6 columns between its borders and a grid of 7
  {
    CHECK(sd_set_option("extract.fast_merge_from", 6) == SD_OK, "option");
    HostPlan hp;
    plan_tables(500, 1.2f, 2, hp);
    const char* why = "";
    CHECK(!plan_geometry(500, 2, 20, 44, 44, hp, &why), "44 x 44 with 500 features was accepted");
    CHECK(std::strcmp(why, "a grid cell's FAST zone is one pixel wide (frame too small for this many features per level)") == 0, "refused with: %s", why);
    plan_tables(100, 1.2f, 2, hp);
    CHECK(plan_geometry(100, 2, 20, 44, 44, hp, &why), "44 x 44 with 100 features refused: %s", why);
  }
  std::printf("orb_fast_lds_check OK (%ld divisions, %ld cell layouts, %ld replayed indices)\n", n_div, n_cells, n_replayed);
  return 0;
}
