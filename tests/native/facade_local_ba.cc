// Optimizer::LocalBundleAdjustment of include/sdslam/sdslam.hpp on reference-shaped KeyFrame / MapPoint classes.
// Without RUN_ON_GPU (tests/test_local_ba_cpu.py, built with AddressSanitizer + UBSan, links nothing): the host part -- the three
// lists of src/Optimizer.cc:418-460, the roles, the CSR lists (BuildLocalBaLists) and the walk that applies a result (ApplyLocalBa:
// the erase order, SetPose, SetWorldPos) -- against lists and results typed in below.
// With RUN_ON_GPU (tests/test_local_ba_facade.py, linked against the library): the whole method on planted keyframes, once with
// wrong observations (erasures) and once without, against sd_debug_local_ba on lists the test builds with straight loops, and the
// refresh against a straight restatement of MapPoint::UpdateNormalAndDepth over the observations as they are afterwards.
#include "mock_map.h"

using namespace mock;
using Lists = SD_SLAM::Optimizer::LocalBaLists<KeyFrame, MapPoint>;

static void host_part() {
  // keyframes by mnId: 0 (local, fixed by its id), 1 (local), 2 (covisible but bad), 3 and 4 (see local points: fixed cameras),
  // 6 (sees a local point, bad: no fixed camera), 5 the current keyframe.  Frames: id 0 -> 2, 1 -> 0, 3 -> 4, 4 not resident.
  std::vector<KeyFrame> kfs(7);
  for (int i = 0; i < 7; i++) kfs[i].mnId = (unsigned long)i;
  kfs[2].bad = kfs[6].bad = true;
  KeyFrame* cur = &kfs[5];
  cur->covisible = {&kfs[1], &kfs[2], &kfs[0]};
  auto frameOf = [&](KeyFrame* k) { return k->mnId == 0 ? 2 : k->mnId == 1 ? 0 : k->mnId == 3 ? 4 : k->mnId == 6 ? 5 : -1; };
  std::vector<MapPoint> pts(5);
  for (int i = 0; i < 5; i++) pts[i].id = i;
  // the current keyframe's matches: point 1, a hole, point 0; keyframe 1: point 0 again, point 2 (bad), point 3; keyframe 0: point 4
  observe(*cur, pts[1], 1, 1, 0, -1.f);
  cur->add_keypoint(0, 0, 0, -1.f);
  observe(*cur, pts[0], 2, 2, 0, 5.f);
  observe(kfs[1], pts[0], 3, 3, 0, -1.f);
  observe(kfs[1], pts[2], 4, 4, 0, -1.f);
  observe(kfs[1], pts[3], 5, 5, 0, 7.f);
  observe(kfs[0], pts[4], 6, 6, 0, -1.f);
  pts[2].bad = true;
  observe(kfs[3], pts[1], 7, 7, 0, 9.f);
  observe(kfs[4], pts[3], 8, 8, 0, -1.f);
  observe(kfs[6], pts[4], 9, 9, 0, -1.f);
  observe(kfs[3], pts[4], 10, 10, 0, -1.f);
  observe(kfs[2], pts[1], 11, 11, 0, -1.f);   // the bad covisible keyframe: neither local nor fixed, its observation carries kf_bad
  pts[0].ref = &kfs[1]; pts[1].ref = cur; pts[3].ref = &kfs[1]; pts[4].ref = &kfs[1];   // point 4's reference does not observe it
  Lists L;
  SD_SLAM::Optimizer::BuildLocalBaLists(cur, frameOf, L);
  CHECK(L.local == (std::vector<KeyFrame*>{cur, &kfs[1], &kfs[0]}), "lLocalKeyFrames");
  CHECK(L.points == (std::vector<MapPoint*>{&pts[1], &pts[0], &pts[3], &pts[4]}), "lLocalMapPoints");
  CHECK(L.fixed == (std::vector<KeyFrame*>{&kfs[3], &kfs[4]}), "lFixedCameras");
  CHECK(kfs[2].mnBALocalForKF == 5 && kfs[6].mnBAFixedForKF == 5 && kfs[3].mnBAFixedForKF == 5 && pts[2].mnBALocalForKF == ~0ul, "marks");
  CHECK(L.kf_role == (std::vector<uint8_t>{1, 0, 2}) && L.cur_role == 1, "roles");
  CHECK(L.resident == (std::vector<KeyFrame*>{&kfs[1], &kfs[0], &kfs[3]}) && L.resident_frame == (std::vector<int>{0, 2, 4}), "resident");
  // observations in id order: point 1: kf2 (bad), kf3, cur; point 0: kf1, cur; point 3: kf1, kf4; point 4: kf0, kf3, kf6 (bad)
  const std::vector<int32_t> off = {0, 3, 5, 7, 10}, frame = {-2, 4, -1, 0, -1, 0, -2, 2, 4, 5}, kp = {0, 0, 0, 0, 2, 2, 0, 0, 1, 0};
  const std::vector<uint8_t> kf_bad = {1, 0, 0, 0, 0, 0, 0, 0, 0, 1}, stereo = {0, 1, 0, 0, 1, 1, 0, 0, 0, 0}, left = {0, 0, 0, 1};
  CHECK(L.obs.off == off && L.obs.frame == frame && L.obs.kp == kp && L.obs.kf_bad == kf_bad, "CSR lists");
  CHECK(L.obs.ref_obs == (std::vector<int32_t>{2, 0, 0, 0}) && L.obs.left == left && L.edge_stereo == stereo, "ref_obs / stereo");
  CHECK(L.edge_pt == (std::vector<int32_t>{0, 0, 0, 1, 1, 2, 2, 3, 3, 3}) && L.edge_kf[1] == &kfs[3] && L.edge_kf[6] == &kfs[4], "edges");

  // a result: erase entries 1 (stereo), 3 (mono), 4 (stereo), 8 (mono) -> mono first: 3, 8, then 1, 4
  SD_SLAM::Optimizer::LocalBaResult r(3, 4, 10);
  for (size_t e : {1u, 3u, 4u, 8u}) r.obs_erase[e] = 1;
  for (int f = 0; f < 3; f++) r.T_ref[(size_t)f * 16 + 12] = 100.0 + f;
  r.T_cur[12] = 55.0;
  for (int i = 0; i < 4; i++) r.Xw[(size_t)i * 3] = 10.0 + i;
  g_calls.clear();
  CHECK(SD_SLAM::Optimizer::ApplyLocalBa(cur, L, r), "something was erased");
  const std::vector<std::pair<int, int>> order = {{1, 0}, {3, 4}, {3, 1}, {5, 0}};
  CHECK(erased() == order, "erase order: all mono edges, then all stereo edges");
  CHECK(cur->mps[2] == nullptr && kfs[1].mps[0] == nullptr && kfs[3].mps[0] == nullptr && kfs[3].mps[1] == nullptr && cur->mps[0] == &pts[1], "matches");
  CHECK(pts[0].obs.empty() && pts[1].obs.size() == 2 && pts[4].obs.size() == 2, "observations");
  CHECK(cur->T.v[12] == 55.0 && kfs[1].T.v[12] == 100.0 && kfs[0].T.v[12] == 102.0 && cur->set_pose() + kfs[1].set_pose() + kfs[0].set_pose() == 3, "SetPose");
  CHECK(kfs[3].set_pose() == 0 && kfs[4].set_pose() == 0, "fixed cameras keep their pose objects");
  CHECK(pts[1].X.v[0] == 10.0 && pts[0].X.v[0] == 11.0 && pts[3].X.v[0] == 12.0 && pts[4].X.v[0] == 13.0 && pts[2].set_pos() == 0, "SetWorldPos");
  SD_SLAM::Optimizer::BuildBaObservations(cur, frameOf, L);   // what the refresh is given after the erasures
  CHECK(L.obs.off == (std::vector<int32_t>{0, 2, 2, 4, 6}) && L.obs.frame == (std::vector<int32_t>{-2, -1, 0, -2, 2, 5}), "lists after the erasures");
  SD_SLAM::Optimizer::LocalBaResult none(3, 4, 6);
  CHECK(!SD_SLAM::Optimizer::ApplyLocalBa(cur, L, none), "nothing erased");
}

#ifdef RUN_ON_GPU
static const int B = 6, NKF = 7;   // keyframes 0 .. 5 are frames 0 .. 5 of the ref extractor, keyframe 6 is the current one

struct Scene {
  std::vector<KeyFrame> kfs;
  std::vector<MapPoint> pts;
};

// Cameras on a line looking down +z, points 3.5 .. 6 m in front of them; wrong: every tenth point's first observation is 45 px off
static void make_scene(Scene& s, bool wrong) {
  s.kfs.assign(NKF, KeyFrame());
  s.pts.assign(60, MapPoint());
  const unsigned long ids[NKF] = {0, 11, 12, 13, 4, 5, 20};   // mnId 0: local and fixed; 4, 5: fixed cameras; 20: the current keyframe
  for (int c = 0; c < NKF; c++) {
    s.kfs[(size_t)c].mnId = ids[c];
    pose_on_the_line(s.kfs[(size_t)c], c);
  }
  for (int i = 0; i < 60; i++) {
    MapPoint& p = s.pts[(size_t)i];
    p.id = i;
    const double X[3] = {1.5 * uni(), uni(), 4.75 + 1.25 * uni()};
    bool first = true;
    for (int c = 0; c < NKF; c++) {
      if ((i + 2 * c) % 5 >= 3) continue;
      const KeyFrame& k = s.kfs[(size_t)c];
      double pc[3];
      for (int r = 0; r < 3; r++) pc[r] = k.T.v[r] * X[0] + k.T.v[4 + r] * X[1] + k.T.v[8 + r] * X[2] + k.T.v[12 + r];
      double u = FX * pc[0] / pc[2] + CX + 0.4 * uni(), v = FY * pc[1] / pc[2] + CY + 0.4 * uni();
      if (wrong && first && i % 10 == 3) u += 45.0, v -= 30.0;
      first = false;
      const int octave = (i + c) % 3;
      const float ur = (i + c) % 2 ? (float)(u - BF / pc[2] + 0.3 * uni()) : -1.f;
      observe(s.kfs[(size_t)c], p, (float)u, (float)v, octave, ur);
      if (!p.ref) p.ref = &s.kfs[(size_t)c];
    }
    for (int r = 0; r < 3; r++) p.X.v[r] = X[r] + 0.02 * uni();
    std::memset(p.desc, i, 32);
  }
  for (int c = 1; c <= 3; c++)   // the local keyframes start off their true poses
    for (int r = 0; r < 3; r++) s.kfs[(size_t)c].T.v[12 + r] += 0.004 * uni();
  for (int r = 0; r < 3; r++) s.kfs[6].T.v[12 + r] += 0.004 * uni();
  s.kfs[6].covisible = {&s.kfs[2], &s.kfs[1], &s.kfs[3], &s.kfs[0]};
}

static void run_case(SD_SLAM::ORBextractor& cur_x, SD_SLAM::ORBextractor& ref_x, SD_SLAM::TrackBatch& batch, bool wrong) {
  Scene s;
  make_scene(s, wrong);
  plant(ref_x, &s.kfs[0], B, "plant ref");
  plant(cur_x, &s.kfs[6], 1, "plant cur");
  KeyFrame* cur = &s.kfs[6];
  auto frameOf = [&](KeyFrame* k) { return (int)(k - &s.kfs[0]) < B ? (int)(k - &s.kfs[0]) : -1; };
  // the lists with straight loops: local keyframes in covisibility order, their matches by keypoint index, first seen first
  const int local[5] = {6, 2, 1, 3, 0};
  std::vector<MapPoint*> pl;
  for (int c : local)
    for (MapPoint* p : s.kfs[(size_t)c].mps)
      if (p && std::find(pl.begin(), pl.end(), p) == pl.end()) pl.push_back(p);
  CHECK(pl.size() == 60, "%zu local points", pl.size());
  std::vector<int32_t> off(1, 0), kf;
  std::vector<float> uv, ur, inv;
  std::vector<double> Xw;
  std::vector<std::pair<int, int>> edge;   // (mnId, point id)
  std::vector<uint8_t> stereo;
  for (MapPoint* p : pl) {
    for (const auto& ob : p->obs) {
      const KeyFrame* k = ob.first;
      kf.push_back((int32_t)(k - &s.kfs[0]));
      uv.push_back(k->keys[ob.second].x); uv.push_back(k->keys[ob.second].y);
      ur.push_back(k->mvuRight[ob.second]);
      inv.push_back(1.f / (float)(1 << (2 * k->keys[ob.second].octave)));
      edge.push_back({(int)k->mnId, p->id});
      stereo.push_back(!(k->mvuRight[ob.second] < 0));
    }
    off.push_back((int32_t)kf.size());
    for (int r = 0; r < 3; r++) Xw.push_back(p->X.v[r]);
  }
  std::vector<double> T((size_t)NKF * 16), To((size_t)NKF * 16), Xo(Xw.size());
  for (int c = 0; c < NKF; c++) std::memcpy(&T[(size_t)c * 16], s.kfs[(size_t)c].T.v, 128);
  const uint8_t roles[NKF] = {2, 1, 1, 1, 0, 0, 1};
  const float cam9[9] = {FX, FY, CX, CY, BF, 0, 640, 0, 480};
  std::vector<uint8_t> ps(pl.size()), er(kf.size());
  int32_t info[16];
  check(sd_debug_local_ba((int)pl.size(), off.data(), kf.data(), uv.data(), ur.data(), inv.data(), nullptr, nullptr, NKF, T.data(), roles,
                          Xw.data(), cam9, To.data(), Xo.data(), ps.data(), er.data(), info), "debug entry");
  CHECK(info[0] == SD_BA_OK && info[1] == 4 && info[2] == 3 && info[3] == 60 && (wrong ? info[13] >= 3 : info[13] == 0), "info: %d %d %d %d, %d erased",
        info[0], info[1], info[2], info[3], info[13]);
  std::vector<std::pair<int, int>> want_erased;
  for (int st = 0; st < 2; st++)
    for (size_t e = 0; e < er.size(); e++)
      if (er[e] && stereo[e] == st) want_erased.push_back(edge[e]);

  // (every call of the reference has a new keyframe id; the test calls again with the same one, so it takes the marks off)
  auto unmark = [&] {
    for (KeyFrame& k : s.kfs) k.mnBALocalForKF = k.mnBAFixedForKF = ~0ul;
    for (MapPoint& q : s.pts) q.mnBALocalForKF = ~0ul;
  };
  g_calls.clear();
  bool stop = true;
  CHECK(!SD_SLAM::Optimizer::LocalBundleAdjustment(batch, cur, &stop, frameOf, 1) && cur->set_pose() == 0 && pl[0]->set_pos() == 0, "pbStopFlag");
  stop = false;
  unmark();
  CHECK(SD_SLAM::Optimizer::LocalBundleAdjustment(batch, cur, &stop, frameOf, 1), "the call: %s", sd_last_error());
  CHECK(erased() == want_erased, "%zu erased, %zu expected, in the reference's order", erased().size(), want_erased.size());
  for (int c = 0; c < NKF; c++) {
    const bool is_local = c <= 3 || c == 6;
    CHECK(s.kfs[(size_t)c].set_pose() == (is_local ? 1 : 0), "SetPose calls of keyframe %d", c);
    CHECK(std::memcmp(s.kfs[(size_t)c].T.v, &To[(size_t)c * 16], 128) == 0, "pose of keyframe %d", c);
  }
  CHECK(std::memcmp(s.kfs[1].T.v, &T[16], 128) != 0 && std::memcmp(s.kfs[0].T.v, &T[0], 128) == 0, "local poses move, the fixed one does not");
  for (size_t i = 0; i < pl.size(); i++)
    CHECK(pl[i]->set_pos() == 1 && std::memcmp(pl[i]->X.v, &Xo[i * 3], 24) == 0, "position of local point %zu", i);
  // UpdateNormalAndDepth over the observations as they are now, at the optimised poses and positions
  for (size_t i = 0; i < pl.size(); i++) {
    const MapPoint& p = *pl[i];
    if (p.obs.empty() || !p.obs.count(p.ref)) {
      CHECK(p.set_normal() == 0, "point %d has no reference observation and was refreshed", p.id);
      continue;
    }
    const NormalAndDepth want = update_normal_and_depth(p);
    const double* normal = want.normal;
    const float max_dist = want.max_dist, min_dist = want.min_dist;
    CHECK(p.set_normal() == 1 && std::memcmp(p.normal.v, normal, 24) == 0, "normal of point %d: %.17g %.17g", p.id, p.normal.v[0], normal[0]);
    CHECK(p.max_dist == max_dist && p.min_dist == min_dist, "distances of point %d: %.9g %.9g", p.id, p.max_dist, max_dist);
  }
  // the device holds what the objects hold
  double Td[16];
  check(sd_track_debug_read(batch.handle(), 8, 2, Td, 128), "read Tref");
  CHECK(std::memcmp(Td, s.kfs[2].T.v, 128) == 0, "Tref of slot 2");
  check(sd_track_debug_read(batch.handle(), 9, 0, Td, 128), "read Tcur");
  CHECK(std::memcmp(Td, cur->T.v, 128) == 0, "Tcur of slot 0");
  if (!wrong) {   // a refusal: keyframe 5 is not resident any more -> false, nothing touched
    auto fewer = [&](KeyFrame* k) { return (int)(k - &s.kfs[0]) < B - 1 ? (int)(k - &s.kfs[0]) : -1; };
    const size_t before = erased().size();
    unmark();
    CHECK(!SD_SLAM::Optimizer::LocalBundleAdjustment(batch, cur, nullptr, fewer, 1), "a keyframe that is not resident");
    CHECK(erased().size() == before && cur->set_pose() == 1 && pl[0]->set_pos() == 1 && pl[0]->set_normal() <= 1, "a refusal touches nothing");
  }
}

static void gpu_part() {
  const int W = 640, H = 480;
  std::vector<uint8_t> img((size_t)B * W * H);
  for (size_t i = 0; i < img.size(); i++) img[i] = (uint8_t)((i * 2654435761u) >> 24);
  SD_SLAM::ORBextractor cur_x(300, 2.0f, 3, 20, W, H, B), ref_x(300, 2.0f, 3, 20, W, H, B);   // level sigma^2 = 4^level: exact floats
  const int cap = 512;
  std::vector<sd_keypoint> kps((size_t)B * cap);
  std::vector<uint8_t> desc((size_t)B * cap * 32);
  int32_t n_out[B];
  check(sd_orb_extract_batch(ref_x.handle(), img.data(), B, W, H, W, (size_t)W * H, kps.data(), desc.data(), cap, n_out), "extract ref");
  check(sd_orb_extract_batch(cur_x.handle(), img.data(), B, W, H, W, (size_t)W * H, kps.data(), desc.data(), cap, n_out), "extract cur");
  SD_SLAM::TrackBatch batch(cur_x, ref_x, 96, B, 8);
  check(sd_track_set_camera(batch.handle(), FX, FY, CX, CY, BF, 0, (float)W, 0, (float)H), "set_camera");
  run_case(cur_x, ref_x, batch, true);
  run_case(cur_x, ref_x, batch, false);
}
#endif

int main() {
  host_part();
#ifdef RUN_ON_GPU
  gpu_part();
#endif
  std::printf("facade_local_ba OK\n");
  return 0;
}
