// The C++ facade's IMU sensor-model calls (TrackBatch::SetSensorModel / SetMeasurements / ImuState with PredictMotion /
// UpdateMotion) on one camera stream.
//   facade_imu                 link check: prints "facade imu ok" (no GPU work)
//   facade_imu IN OUT          tracks the frames in IN with the device's IMU prior, writes per frame X, P, gravity and the
//                              final pose to OUT (layout: tests/test_imu_facade.py)
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
    auto mod = &TrackBatch::SetSensorModel;
    auto mea = &TrackBatch::SetMeasurements;
    auto get = &TrackBatch::ImuState;
    if (!mod || !mea || !get || SD_SENSOR_IMU != 1) return 1;
    std::printf("facade imu ok\n");
    return 0;
  }
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<int32_t> hdr;   // W, H, T, n (map points), max_points
  std::vector<double> dt, meas;
  if (!rd(f, hdr, 5) || !rd(f, dt, 1)) return 3;
  const int W = hdr[0], H = hdr[1], T = hdr[2], n = hdr[3], M = hdr[4];
  std::vector<uint8_t> frames, desc, valid;
  std::vector<double> T0, Xw, normal;
  std::vector<float> mind, maxd, mfmax, angle;
  std::vector<int32_t> obs, ids, octave;
  bool ok = rd(f, meas, (size_t)T * 6) && rd(f, frames, (size_t)T * W * H) && rd(f, T0, 16) && rd(f, Xw, (size_t)n * 3) &&
            rd(f, normal, (size_t)n * 3) && rd(f, mind, n) && rd(f, maxd, n) && rd(f, mfmax, n) && rd(f, desc, (size_t)n * 32) &&
            rd(f, obs, n) && rd(f, ids, n) && rd(f, valid, n) && rd(f, octave, n) && rd(f, angle, n);
  std::fclose(f);
  if (!ok) return 4;
  ORBextractor a(1000, 1.2f, 8, 20, W, H, 1), b(1000, 1.2f, 8, 20, W, H, 1);
  TrackBatch batch(a, b, M, 1, 100);
  batch.SetCamera(500.f, 500.f, 320.f, 240.f, 0.f, 0.f, (float)W, 0.f, (float)H);
  std::vector<KeyPoint> kps;
  std::vector<uint8_t> dsc;
  b(frames.data(), W, H, W, kps, dsc);   // frame 0 is the first last frame
  LastFrameView last{valid, Xw, desc, octave, angle, obs};
  batch.SetLastFrame(0, last);
  TrackBatch::LocalMapView local{std::vector<uint8_t>(n, 1), Xw, normal, mind, maxd, mfmax, desc, obs};
  batch.SetLocalMap(0, local, nullptr);
  batch.SetMapIds(0, 0, ids.data(), n);
  batch.SetMapIds(0, 1, ids.data(), n);
  batch.SetPoses(0, T0.data(), T0.data());
  batch.SetSensorModel(SD_SENSOR_IMU);
  FILE* o = std::fopen(argv[2], "wb");
  if (!o) return 5;
  for (int t = 1; t < T; t++) {
    batch.CurrentExtractor()(frames.data() + (size_t)t * W * H, W, H, W, kps, dsc);
    batch.SetMeasurements(0, 1, meas.data() + (size_t)t * 6);
    batch.PredictMotion(1, dt[0]);
    Tracking::TrackWithMotionModel(batch, 1, 15.f, true);
    Tracking::TrackLocalMap(batch, 1, 1.f);
    batch.UpdateMotion(1, 1);
    double X[16], P[256], g[3], Tcw[16];
    const int32_t started = batch.ImuState(0, X, P, g) ? 1 : 0;
    ImageAlign().Result(batch, 0, Tcw);   // the frame's final pose
    wr(o, &started, 1);
    wr(o, X, 16);
    wr(o, P, 256);
    wr(o, g, 3);
    wr(o, Tcw, 16);
    batch.AdvanceLastFrame(1, 1);
  }
  std::fclose(o);
  std::printf("facade imu ran %d frames\n", T - 1);
  return 0;
}
