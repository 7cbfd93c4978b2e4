// Host check of the matchers' dynamic-LDS layouts (sdslam_amd/csrc/track_match_lds.h), built with AddressSanitizer and UBSan:
// for every capacity the launchers can pass, every array of every layout is aligned to its element size, the arrays do not
// overlap, the last one ends inside `bytes`, and `bytes` equals the byte formula the launchers used before the layouts had one
// description (restated literally below) minus the slack that formula carried ("LDS layouts of the matchers").
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "track_match_lds.h"

using namespace sd;

struct Arr { const char* name; uint32_t off, elem, count; };

static void check(const char* layout, int a, int b, std::vector<Arr> arrs, uint32_t bytes, size_t old_formula, size_t slack) {
  auto fail = [&](const char* what, const Arr& x) {
    std::printf("%s(%d, %d): %s: %s at %u, %u x %u bytes, total %u\n", layout, a, b, what, x.name, x.off, x.count, x.elem, bytes);
    std::exit(1);
  };
  for (const Arr& x : arrs)
    if (x.off % x.elem) fail("misaligned", x);
  std::sort(arrs.begin(), arrs.end(), [](const Arr& p, const Arr& q) { return p.off < q.off; });
  for (size_t i = 0; i + 1 < arrs.size(); i++)
    if (arrs[i].off + arrs[i].elem * arrs[i].count > arrs[i + 1].off) fail("overlaps its successor", arrs[i]);
  if (arrs.back().off + arrs.back().elem * arrs.back().count > bytes) fail("ends past the total", arrs.back());
  if ((size_t)bytes + slack != old_formula) {
    std::printf("%s(%d, %d): %u bytes + %zu slack != the launcher's old formula %zu\n", layout, a, b, bytes, slack, old_formula);
    std::exit(1);
  }
}

int main() {
  const uint32_t CS = GRID_COLS * GRID_ROWS + 2;
  long n = 0;
  for (int KP2 = 64; KP2 <= 2048; KP2 <<= 1) {
    for (int MP = 1; MP <= 2048; MP++, n++) {
      const uint32_t MW = (MP + 31) >> 5;
      {
        const LdsMatch L(KP2, MP);
        const size_t old = (size_t)KP2 * 4 + MT_LIST_CAP * 4 + (size_t)MP * 4 + (size_t)KP2 * 4 + (size_t)((MP + 31) >> 5) * 8 + (size_t)KP2 * 2 +
                           (size_t)std::max(KP2, MP) * 2 + (GRID_COLS * GRID_ROWS + 2) * 2 + 4 + (HISTO_LENGTH + 1) * 4;
        // the old formula always reserved 4 bytes for the pad in front of s_hist; the pad is 2 when s_ev holds an odd count
        const size_t slack = (std::max(KP2, MP) & 1) ? 2 : 4;
        check("LdsMatch", KP2, MP, {{"key", L.key, 4, (uint32_t)KP2}, {"list", L.list, 4, MT_LIST_CAP}, {"pt", L.pt, 4, (uint32_t)MP},
                                    {"kang", L.kang, 4, (uint32_t)KP2}, {"obs", L.obs, 4, MW}, {"valid", L.valid, 4, MW},
                                    {"match", L.match, 2, (uint32_t)KP2}, {"ev", L.ev, 2, (uint32_t)std::max(KP2, MP)},
                                    {"cstart", L.cstart, 2, CS}, {"hist", L.hist, 4, HISTO_LENGTH}, {"nlist", L.nlist, 4, 1}},
              L.bytes, old, slack);
      }
      {
        const LdsMatchCand L(KP2, MP);
        const size_t old = (size_t)KP2 * 4 + (size_t)MP * 4 + (size_t)(MP + (MP & 1)) * 2 + (size_t)((MP + 31) >> 5) * 4 +
                           (GRID_COLS * GRID_ROWS + 2) * 2 + 8;
        check("LdsMatchCand", KP2, MP, {{"key", L.key, 4, (uint32_t)KP2}, {"off", L.off, 4, (uint32_t)MP}, {"cnt", L.cnt, 2, (uint32_t)MP},
                                        {"valid", L.valid, 4, MW}, {"cstart", L.cstart, 2, CS}},
              L.bytes, old, 8);   // 8 spare bytes nothing used
      }
      {
        const LdsMatchAssign L(KP2, MP);
        const size_t old = (size_t)MP * 4 + (size_t)((MP + 31) >> 5) * 4 + (HISTO_LENGTH + 2) * 4 + (size_t)KP2 * 2;
        check("LdsMatchAssign", KP2, MP, {{"ev", L.ev, 4, (uint32_t)MP}, {"obs", L.obs, 4, MW}, {"hist", L.hist, 4, HISTO_LENGTH + 2},
                                          {"match", L.match, 2, (uint32_t)KP2}},
              L.bytes, old, 0);
      }
      {
        const LdsMatchLocal L(KP2, MP);
        const size_t old = (size_t)KP2 * 4 + MT_LIST_CAP * 4 + (size_t)MP * 4 + (size_t)((MP + 31) >> 5) * 4 + (size_t)(KP2 >> 5) * 4 +
                           (size_t)KP2 * 2 + (GRID_COLS * GRID_ROWS + 2) * 2 + (size_t)KP2 + 4 + 8;
        check("LdsMatchLocal", KP2, MP, {{"key", L.key, 4, (uint32_t)KP2}, {"list", L.list, 4, MT_LIST_CAP}, {"pt", L.pt, 4, (uint32_t)MP},
                                         {"obs", L.obs, 4, MW}, {"kclaim", L.kclaim, 4, (uint32_t)KP2 >> 5}, {"match", L.match, 2, (uint32_t)KP2},
                                         {"cstart", L.cstart, 2, CS}, {"koct", L.koct, 1, (uint32_t)KP2}, {"nlist", L.nlist, 4, 1}},
              L.bytes, old, 8);   // 8 spare bytes nothing used (s_nlist's 4 were counted, its pad is always 0)
      }
    }
    {
      const LdsFeaturesInArea L(KP2);
      const size_t old = (size_t)KP2 * 8 + (GRID_COLS * GRID_ROWS + 2) * 2;
      check("LdsFeaturesInArea", KP2, 0, {{"key", L.key, 4, (uint32_t)KP2}, {"list", L.list, 4, (uint32_t)KP2}, {"cstart", L.cstart, 2, CS}}, L.bytes,
            old, 0);
      const LdsSeenIds S(KP2);
      check("LdsSeenIds", KP2, 0, {{"ids", S.ids, 4, (uint32_t)KP2}}, S.bytes, (size_t)KP2 * 4, 0);
    }
  }
  for (int capw = 64; capw <= 2048; capw += 64, n++) {
    const LdsSearchPoints L(capw);
    const size_t old = (size_t)BF_TILE * 32 + (size_t)capw * BF_K * 4 + (size_t)capw * 2 * 2 + (size_t)(capw >> 5) * 4 * 2 + 8 + 33 * 4 + 16;
    check("LdsSearchPoints", capw, 0, {{"tile", L.tile, 4, BF_TILE * 8}, {"list", L.list, 4, (uint32_t)capw * BF_K}, {"i1", L.i1, 2, (uint32_t)capw},
                                       {"match", L.match, 2, (uint32_t)capw}, {"v2", L.v2, 4, (uint32_t)capw >> 5},
                                       {"m2", L.m2, 4, (uint32_t)capw >> 5}, {"hist", L.hist, 4, 32}, {"n1v", L.n1v, 4, 1}},
          L.bytes, old, 24);   // 8 + 16 spare bytes nothing used
  }
  std::printf("match_lds_check OK (%ld capacities)\n", n);
  return 0;
}
