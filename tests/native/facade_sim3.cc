// The C++ facade's Sim3Solver and LoopClosing::ComputeSim3Candidates on three loop candidates.
//   facade_sim3                link check: prints "facade sim3 ok" (no GPU work)
//   facade_sim3 IN OUT         extracts the frames in IN, uploads poses, flags, points, matches and rand() streams, runs the
//                              round-robin and writes the winning slot, every slot's mnIterations and the winner's T12 to OUT
//                              (layout: tests/test_sim3_facade.py)
#include <sdslam/sdslam.hpp>

#include <cstdio>
#include <vector>

template <typename T>
static bool rd(FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n);
  return fread(v.data(), sizeof(T), n, f) == n;
}
template <typename T>
static void wr(FILE* f, const T* p, size_t n) { fwrite(p, sizeof(T), n, f); }

int main(int argc, char** argv) {
  using namespace SD_SLAM;
  if (argc < 3) {
    auto it = &Sim3Solver::iterateAgain;
    auto res = &Sim3Solver::Result;
    auto sc = &Sim3Solver::GetEstimatedScale;
    int (*cand)(TrackBatch&, int, Sim3Solver&, int) = &LoopClosing::ComputeSim3Candidates;
    if (!it || !res || !sc || !cand) return 1;
    std::printf("facade sim3 ok\n");
    return 0;
  }
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<int32_t> hdr;   // W, H, nfeatures, nlevels, n (slots), rand values per slot
  std::vector<float> fl;      // scaleFactor, fx, fy, cx, cy
  if (!rd(f, hdr, 6) || !rd(f, fl, 5)) return 3;
  const int W = hdr[0], H = hdr[1], NF = hdr[2], NL = hdr[3], n = hdr[4], per = hdr[5];
  std::vector<uint8_t> cur_img, ref_img, has1, has2;
  std::vector<double> Tref, Tcur, Xw1, Xw2;
  std::vector<int32_t> m12, rnd;
  const bool ok = rd(f, cur_img, (size_t)n * W * H) && rd(f, ref_img, (size_t)n * W * H) && rd(f, Tref, (size_t)n * 16) &&
                  rd(f, Tcur, (size_t)n * 16) && rd(f, has1, (size_t)n * NF) && rd(f, has2, (size_t)n * NF) && rd(f, Xw1, (size_t)n * NF * 3) &&
                  rd(f, Xw2, (size_t)n * NF * 3) && rd(f, m12, (size_t)n * NF) && rd(f, rnd, (size_t)n * per);
  std::fclose(f);
  if (!ok) return 4;
  ORBextractor a(NF, fl[0], NL, 20, W, H, n), b(NF, fl[0], NL, 20, W, H, n);
  TrackBatch batch(a, b, NF, n, 300);
  batch.SetCamera(fl[1], fl[2], fl[3], fl[4], 0.f, 0.f, (float)W, 0.f, (float)H);
  std::vector<sd_keypoint> kps((size_t)n * NF);
  std::vector<uint8_t> dsc((size_t)n * NF * 32);
  std::vector<int32_t> nkp(n);
  check(sd_orb_extract_batch(a.handle(), cur_img.data(), n, W, H, W, (size_t)W * H, kps.data(), dsc.data(), NF, nkp.data()));
  check(sd_orb_extract_batch(b.handle(), ref_img.data(), n, W, H, W, (size_t)W * H, kps.data(), dsc.data(), NF, nkp.data()));
  for (int i = 0; i < n; i++) batch.SetPoses(i, Tref.data() + (size_t)i * 16, Tcur.data() + (size_t)i * 16);
  check(sd_track_set_point_flags(batch.handle(), 0, n, has1.data(), has2.data(), NF));
  Sim3Solver::SetPoints(batch, 0, n, Xw1.data(), Xw2.data(), NF);
  for (int i = 0; i < n; i++) Sim3Solver::SetMatches(batch, i, m12.data() + (size_t)i * NF, NF);
  check(sd_track_set_rand(batch.handle(), 0, n, rnd.data(), per));
  Sim3Solver solver(false);
  solver.SetRansacParameters(0.99, 20, 300);   // src/LoopClosing.cc:264
  std::vector<int> its;
  std::vector<uint8_t> discarded;
  const int32_t winner = LoopClosing::ComputeSim3Candidates(batch, n, solver, NF, &discarded, [](int) { return true; }, &its);
  double T12[16] = {0};
  std::vector<uint8_t> inl;
  bool no_more = false;
  int n_inl = 0;
  if (winner >= 0) solver.Result(batch, winner, T12, no_more, inl, n_inl, NF);
  const float scale = winner >= 0 ? solver.GetEstimatedScale(batch, winner) : 0.f;
  FILE* o = std::fopen(argv[2], "wb");
  if (!o) return 5;
  wr(o, &winner, 1);
  std::vector<int32_t> it32(its.begin(), its.end());
  wr(o, it32.data(), it32.size());
  const int32_t ni = n_inl;
  wr(o, &ni, 1);
  wr(o, T12, 16);
  wr(o, &scale, 1);
  std::fclose(o);
  std::printf("facade sim3 ran %d candidates\n", n);
  return 0;
}
