// The C++ facade's RGB-D calls on one camera stream: ComputeStereoFromRGBD on a 16-bit depth map in device memory and
// TrackBatch::CloseTrackedPoints / CloseTrackedPointsResult.
//   facade_close_points             link check: prints "facade close points ok" (no GPU work)
//   facade_close_points IN OUT      tracks frame 1 of IN against frame 0 (RGB-D TrackWithMotionModel, then TrackLocalMap) and
//                                   writes the counts after each (layout: tests/test_close_points_facade.py)
#include <sdslam/sdslam.hpp>

#include <cstdio>
#include <vector>

template <typename T>
static bool rd(FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n);
  return fread(v.data(), sizeof(T), n, f) == n;
}

int main(int argc, char** argv) {
  using namespace SD_SLAM;
  if (argc < 3) {
    auto q = &TrackBatch::CloseTrackedPoints;
    auto r = &TrackBatch::CloseTrackedPointsResult;
    void (TrackBatch::*dev)(int, const void*, int, int, int, int, size_t, float) = &TrackBatch::ComputeStereoFromRGBD;
    if (!q || !r || !dev) return 1;
    std::printf("facade close points ok\n");
    return 0;
  }
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<int32_t> hdr;   // W, H, n (map points), max_points
  std::vector<float> par;     // bf, th_depth, DepthMapFactor
  if (!rd(f, hdr, 4) || !rd(f, par, 3)) return 3;
  const int W = hdr[0], H = hdr[1], n = hdr[2], M = hdr[3];
  std::vector<uint8_t> frames, desc, valid;
  std::vector<uint16_t> depth;
  std::vector<float> mind, maxd, mfmax, angle;
  std::vector<double> T0, vel, Xw, normal;
  std::vector<int32_t> obs, octave;
  bool ok = rd(f, frames, (size_t)2 * W * H) && rd(f, depth, (size_t)W * H) && rd(f, T0, 16) && rd(f, vel, 16) && rd(f, Xw, (size_t)n * 3) &&
            rd(f, normal, (size_t)n * 3) && rd(f, mind, n) && rd(f, maxd, n) && rd(f, mfmax, n) && rd(f, desc, (size_t)n * 32) &&
            rd(f, obs, n) && rd(f, valid, n) && rd(f, octave, n) && rd(f, angle, n);
  std::fclose(f);
  if (!ok) return 4;
  ORBextractor a(1000, 1.2f, 8, 20, W, H, 1), b(1000, 1.2f, 8, 20, W, H, 1);
  TrackBatch batch(a, b, M, 1, 100);
  batch.SetCamera(500.f, 500.f, 320.f, 240.f, par[0], 0.f, (float)W, 0.f, (float)H);
  std::vector<KeyPoint> kps;
  std::vector<uint8_t> dsc;
  b(frames.data(), W, H, W, kps, dsc);   // frame 0 is the last frame
  LastFrameView last{valid, Xw, desc, octave, angle, obs};
  batch.SetLastFrame(0, last);
  TrackBatch::LocalMapView local{std::vector<uint8_t>(n, 1), Xw, normal, mind, maxd, mfmax, desc, obs};
  batch.SetLocalMap(0, local, nullptr);
  batch.SetPoses(0, T0.data(), T0.data());
  batch.CurrentExtractor()(frames.data() + (size_t)W * H, W, H, W, kps, dsc);
  void* d_depth = nullptr;
  check(sd_dev_alloc(depth.size() * 2, &d_depth));
  check(sd_dev_upload(d_depth, depth.data(), depth.size() * 2));
  batch.ComputeStereoFromRGBD(1, d_depth, SD_DEPTH_U16, W, H, W, (size_t)W * H, par[2]);
  batch.SetPrior(0, 1, vel.data(), true);
  int32_t c[4];
  Tracking::TrackWithMotionModel(batch, 1, 15.f, false);
  batch.CloseTrackedPoints(1, 0, par[1]);
  batch.CloseTrackedPointsResult(0, c[0], c[1]);
  Tracking::TrackLocalMap(batch, 1, 3.f);
  batch.CloseTrackedPoints(1, 1, par[1]);
  batch.CloseTrackedPointsResult(0, c[2], c[3]);   // (synchronises: the depth map is free again)
  check(sd_dev_free(d_depth));
  FILE* o = std::fopen(argv[2], "wb");
  if (!o) return 5;
  fwrite(c, sizeof(int32_t), 4, o);
  std::fclose(o);
  std::printf("facade close points ran: %d %d %d %d\n", c[0], c[1], c[2], c[3]);
  return 0;
}
