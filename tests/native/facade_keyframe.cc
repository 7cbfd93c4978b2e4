// The C++ facade's RGB-D map point calls on one camera stream: TrackBatch::StereoInitialization, Tracking::NeedNewKeyFrame,
// Tracking::CreateNewKeyFrame, TrackBatch::CreatedPoints.
//   facade_keyframe             link check: prints "facade keyframe ok" (no GPU work)
//   facade_keyframe IN OUT      initialises on frame 0 of IN, tracks frame 1 from the created points (RGB-D TrackWithMotionModel,
//                               TrackLocalMap with an empty local map), decides, creates, and writes both creation records and
//                               the decision (layout: tests/test_keyframe_facade.py)
#include <sdslam/sdslam.hpp>

#include <cstdio>
#include <vector>

template <typename T>
static bool rd(FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n);
  return fread(v.data(), sizeof(T), n, f) == n;
}

static void put(FILE* o, const SD_SLAM::TrackBatch::CreatedMapPoints& c) {
  const int32_t h[4] = {c.mode, (int32_t)c.keypoint.size(), c.processed, c.candidates};
  fwrite(h, 4, 4, o);
  fwrite(c.keypoint.data(), 4, c.keypoint.size(), o);
  fwrite(c.id.data(), 4, c.id.size(), o);
  fwrite(c.Xw.data(), 8, c.Xw.size(), o);
}

int main(int argc, char** argv) {
  using namespace SD_SLAM;
  if (argc < 3) {
    auto a = &TrackBatch::StereoInitialization;
    auto b = &TrackBatch::CreatedPoints;
    auto c = &Tracking::NeedNewKeyFrame;
    auto d = &Tracking::CreateNewKeyFrame;
    if (!a || !b || !c || !d) return 1;
    std::printf("facade keyframe ok\n");
    return 0;
  }
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<int32_t> hdr, state;   // W, H, max_points, next id, MinFrames, MaxFrames | 8 ints of keyframe state
  std::vector<float> par;            // bf, th_depth, DepthMapFactor
  std::vector<uint8_t> frames;
  std::vector<uint16_t> depth;
  std::vector<double> vel;
  if (!rd(f, hdr, 6) || !rd(f, state, 8) || !rd(f, par, 3)) return 3;
  const int W = hdr[0], H = hdr[1], M = hdr[2];
  const bool ok = rd(f, frames, (size_t)2 * W * H) && rd(f, depth, (size_t)2 * W * H) && rd(f, vel, 16);
  std::fclose(f);
  if (!ok) return 4;
  ORBextractor a(1000, 1.2f, 8, 20, W, H, 1), b(1000, 1.2f, 8, 20, W, H, 1);
  TrackBatch batch(a, b, M, 1, 100);
  batch.SetCamera(500.f, 500.f, 320.f, 240.f, par[0], 0.f, (float)W, 0.f, (float)H);
  void* d_depth = nullptr;
  check(sd_dev_alloc(depth.size() * 2, &d_depth));
  check(sd_dev_upload(d_depth, depth.data(), depth.size() * 2));
  std::vector<KeyPoint> kps;
  std::vector<uint8_t> dsc;
  const int32_t next_id = hdr[3];
  batch.SetNextMapPointId(0, 1, &next_id);
  batch.SetKeyFrameState(0, 1, state.data());
  batch.CurrentExtractor()(frames.data(), W, H, W, kps, dsc);
  batch.ComputeStereoFromRGBD(1, d_depth, SD_DEPTH_U16, W, H, W, (size_t)W * H, par[2]);
  batch.StereoInitialization(1);
  const TrackBatch::CreatedMapPoints c0 = batch.CreatedPoints(0);
  batch.AdvanceLastFrame(1, 2);
  batch.CurrentExtractor()(frames.data() + (size_t)W * H, W, H, W, kps, dsc);
  batch.ComputeStereoFromRGBD(1, (const uint16_t*)d_depth + (size_t)W * H, SD_DEPTH_U16, W, H, W, (size_t)W * H, par[2]);
  batch.SetPrior(0, 1, vel.data(), true);
  Tracking::TrackWithMotionModel(batch, 1, 15.f, false);
  Tracking::TrackLocalMap(batch, 1, 3.f);
  batch.CloseTrackedPoints(1, 1, par[1]);
  Tracking::NeedNewKeyFrame(batch, 1, true, 1, hdr[4], hdr[5]);
  Tracking::CreateNewKeyFrame(batch, 1, 1, par[1], true, 1);
  const int32_t flag = batch.KeyFrameFlags(0);
  const TrackBatch::CreatedMapPoints c1 = batch.CreatedPoints(0);
  batch.AdvanceLastFrame(1, 1);
  LastFrameView last;
  std::vector<int32_t> ids;
  batch.GetLastFrame(0, last, &ids);
  check(sd_dev_free(d_depth));
  FILE* o = std::fopen(argv[2], "wb");
  if (!o) return 5;
  put(o, c0);
  fwrite(&flag, 4, 1, o);
  put(o, c1);
  const int32_t n = (int32_t)ids.size();
  fwrite(&n, 4, 1, o);
  fwrite(ids.data(), 4, ids.size(), o);
  std::fclose(o);
  std::printf("facade keyframe ran: %zu + %zu points, flag %d\n", c0.keypoint.size(), c1.keypoint.size(), flag);
  return 0;
}
