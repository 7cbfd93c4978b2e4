// MapPoint::ComputeDistinctiveDescriptors + UpdateNormalAndDepth (src/MapPoint.cc:225-343) as a straight C++ loop over CSR
// observation lists: the host side of tools/bench_refresh.py (what a caller runs between Fuse and the next search without
// sd_track_refresh_points).  Same arguments as sd_debug_refresh_points; g++ -O2 -ffp-contract=off -shared -fPIC.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstring>
#include <vector>

static inline int hamming(const uint8_t* a, const uint8_t* b) {
  const uint64_t* x = (const uint64_t*)a;
  const uint64_t* y = (const uint64_t*)b;
  return __builtin_popcountll(x[0] ^ y[0]) + __builtin_popcountll(x[1] ^ y[1]) + __builtin_popcountll(x[2] ^ y[2]) +
         __builtin_popcountll(x[3] ^ y[3]);
}

extern "C" int refresh_host(int n_points, const int32_t* off, const uint8_t* desc, const double* centre, const int32_t* octave,
                            const uint8_t* kf_bad, const int32_t* ref_obs, const uint8_t* point_bad, const double* Xw, const float* sf,
                            int nlevels, uint8_t* status, int32_t* best_obs, int32_t* best_median, uint8_t* out_desc, double* normal,
                            float* max_dist, float* min_dist) {
  std::vector<int> kept, row;
  std::vector<int> D;
  for (int p = 0; p < n_points; p++) {
    const int a = off[p], n = off[p + 1] - a;
    if ((point_bad && point_bad[p]) || n == 0) { status[p] = 16; continue; }
    if (n > 256) { status[p] = 64; continue; }
    int st = 2;
    kept.clear();
    for (int o = 0; o < n; o++)
      if (!kf_bad || !kf_bad[a + o]) kept.push_back(o);
    const int N = (int)kept.size();
    if (N > 0) {
      D.assign((size_t)N * N, 0);
      for (int i = 0; i < N; i++)
        for (int j = i + 1; j < N; j++)
          D[(size_t)i * N + j] = D[(size_t)j * N + i] = hamming(desc + (size_t)(a + kept[i]) * 32, desc + (size_t)(a + kept[j]) * 32);
      int bm = 1 << 30, bi = 0;
      for (int i = 0; i < N; i++) {
        row.assign(D.begin() + (size_t)i * N, D.begin() + (size_t)(i + 1) * N);
        std::sort(row.begin(), row.end());
        const int med = row[(size_t)(0.5 * (N - 1))];
        if (med < bm) bm = med, bi = i;
      }
      best_obs[p] = kept[bi];
      best_median[p] = bm;
      std::memcpy(out_desc + (size_t)p * 32, desc + (size_t)(a + kept[bi]) * 32, 32);
      st |= 1;
    }
    const double* X = Xw + (size_t)p * 3;
    double s[3] = {0, 0, 0};
    for (int o = 0; o < n; o++) {
      const double* c = centre + (size_t)(a + o) * 3;
      const double d[3] = {X[0] - c[0], X[1] - c[1], X[2] - c[2]};
      const double len = std::sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
      for (int k = 0; k < 3; k++) s[k] = s[k] + d[k] / len;
    }
    for (int k = 0; k < 3; k++) normal[(size_t)p * 3 + k] = s[k] / n;
    const double* c = centre + (size_t)(a + ref_obs[p]) * 3;
    const double d[3] = {X[0] - c[0], X[1] - c[1], X[2] - c[2]};
    const float dist = (float)std::sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
    max_dist[p] = dist * sf[std::min(std::max(octave[a + ref_obs[p]], 0), nlevels - 1)];
    min_dist[p] = max_dist[p] / sf[nlevels - 1];
    status[p] = (uint8_t)st;
  }
  return 0;
}
