// Optimizer::BundleAdjustment / GlobalBundleAdjustemnt of include/sdslam/sdslam.hpp on mock KeyFrame / MapPoint / Map classes shaped
// like the reference's (tests/test_global_ba_facade.py, linked against the library).  The host part checks the roles and the CSR
// lists (BuildGlobalBaLists) against lists typed in below.  The device part plants six keyframes, runs the method through both
// nLoopKF branches and compares what the objects were given, byte for byte, with sd_debug_global_ba on lists built by straight
// loops; the order of the SetPose / SetWorldPos / refresh calls with the reference's (:185-217); the normals and distances with a
// restatement of MapPoint::UpdateNormalAndDepth; and checks that a set stop flag and a refusal return false and touch nothing.
#if !defined(HOST_PART_ONLY) && !defined(RUN_ON_GPU)   // (the test's build defines nothing; -DHOST_PART_ONLY builds host_part()
#define RUN_ON_GPU                                     // alone and links nothing)
#endif
#include "mock_map.h"

using namespace mock;

static void host_part() {
  // keyframes by mnId: 0 (fixed by its id), 1, 2 (bad), 3 (not resident), 9 (not in vpKFs, id above maxKFid = 3).  Frames: 0 -> 2, 1 -> 0, 2 -> 1, 9 -> 3.
  std::vector<KeyFrame> kfs(5);
  const unsigned long ids[5] = {0, 1, 2, 3, 9};
  for (int i = 0; i < 5; i++) kfs[(size_t)i].mnId = ids[i];
  kfs[2].bad = true;
  auto frameOf = [&](KeyFrame* k) { return k->mnId == 0 ? 2 : k->mnId == 1 ? 0 : k->mnId == 2 ? 1 : k->mnId == 9 ? 3 : -1; };
  std::vector<MapPoint> pts(4);
  for (int i = 0; i < 4; i++) pts[(size_t)i].id = i;
  observe(kfs[0], pts[0], 1, 1, 0, -1.f);
  observe(kfs[1], pts[0], 2, 2, 0, 5.f);
  observe(kfs[2], pts[0], 3, 3, 0, -1.f);
  observe(kfs[1], pts[1], 4, 4, 0, -1.f);
  observe(kfs[1], pts[2], 5, 5, 0, -1.f);
  observe(kfs[3], pts[2], 6, 6, 0, -1.f);
  observe(kfs[4], pts[2], 7, 7, 0, -1.f);
  pts[1].bad = true;
  pts[0].ref = &kfs[1]; pts[2].ref = &kfs[0];   // point 2's reference does not observe it
  const std::vector<KeyFrame*> vpKFs = {&kfs[1], &kfs[0], &kfs[2], &kfs[3]};
  const std::vector<MapPoint*> vpMP = {&pts[0], &pts[1], nullptr, &pts[2], &pts[3]};
  SD_SLAM::Optimizer::GlobalBaLists<KeyFrame> L;
  SD_SLAM::Optimizer::BuildGlobalBaLists(vpKFs, vpMP, frameOf, L);
  CHECK(L.kf_role == (std::vector<uint8_t>{1, 0, 2}), "roles: a bad keyframe has none, mnId 0 is fixed");
  CHECK(L.resident == (std::vector<KeyFrame*>{&kfs[1], &kfs[0]}) && L.resident_frame == (std::vector<int>{0, 2}), "resident");
  CHECK(L.obs.off == (std::vector<int32_t>{0, 3, 3, 3, 6, 6}) && L.obs.point_bad == (std::vector<uint8_t>{0, 1, 1, 0, 0}), "offsets / point_bad");
  CHECK(L.obs.frame == (std::vector<int32_t>{2, 0, 1, 0, -2, 3}) && L.obs.kp == (std::vector<int32_t>{0, 0, 0, 2, 0, 0}), "frames / keypoints");
  CHECK(L.obs.kf_bad == (std::vector<uint8_t>{0, 0, 1, 0, 0, 0}) && L.ba_kf_bad == (std::vector<uint8_t>{0, 0, 1, 0, 0, 1}), "kf_bad: isBad(), and mnId > maxKFid for the run");
  CHECK(L.obs.ref_obs == (std::vector<int32_t>{1, 0, 0, 0, 0}) && L.obs.left == (std::vector<uint8_t>{0, 0, 0, 1, 0}), "ref_obs / left");
}

#ifdef RUN_ON_GPU
static const int B = 6, NKF = 8, NP = 60;   // keyframes 0 .. 5 are frames 0 .. 5 of the ref extractor; 6 is bad, 7 is newer than vpKFs

struct Scene {
  std::vector<KeyFrame> kfs;
  std::vector<MapPoint> pts;
  Map map;
};

// Cameras on a line looking down +z, points 3.5 .. 6 m in front of them
static void make_scene(Scene& s) {
  s.kfs.assign(NKF, KeyFrame());
  s.pts.assign(NP + 2, MapPoint());
  const unsigned long ids[NKF] = {0, 11, 12, 13, 4, 5, 7, 99};
  for (int c = 0; c < NKF; c++) {
    s.kfs[(size_t)c].mnId = ids[c];
    pose_on_the_line(s.kfs[(size_t)c], c);
  }
  s.kfs[6].bad = true;
  for (int i = 0; i < NP; i++) {
    MapPoint& p = s.pts[(size_t)i];
    p.id = i;
    const double X[3] = {1.5 * uni(), uni(), 4.75 + 1.25 * uni()};
    for (int c = 0; c < NKF; c++) {
      if ((i + 2 * c) % 5 >= 3 || (c >= 6 && i % 7)) continue;   // the bad and the newer keyframe see every seventh point
      const KeyFrame& k = s.kfs[(size_t)c];
      double pc[3];
      for (int r = 0; r < 3; r++) pc[r] = k.T.v[r] * X[0] + k.T.v[4 + r] * X[1] + k.T.v[8 + r] * X[2] + k.T.v[12 + r];
      const double u = FX * pc[0] / pc[2] + CX + 0.4 * uni(), v = FY * pc[1] / pc[2] + CY + 0.4 * uni();
      const float ur = (i + c) % 2 ? (float)(u - BF / pc[2] + 0.3 * uni()) : -1.f;
      observe(s.kfs[(size_t)c], p, (float)u, (float)v, (i + c) % 3, ur);
      if (!p.ref && c < 6) p.ref = &s.kfs[(size_t)c];
    }
    for (int r = 0; r < 3; r++) p.X.v[r] = X[r] + 0.02 * uni();
    std::memset(p.desc, i, 32);
  }
  s.pts[NP].id = NP; s.pts[NP].bad = true;          // a bad point with an observation
  observe(s.kfs[1], s.pts[NP], 100.f, 100.f, 0, -1.f);
  s.pts[NP + 1].id = NP + 1;                          // a point nobody observes: vbNotIncludedMP
  s.pts[5].ref = &s.kfs[7];                           // point 5's reference keyframe ...
  s.pts[5].obs.erase(&s.kfs[7]);                      // ... does not observe it: the position only
  for (int c = 1; c < 6; c++)                         // the free keyframes start off their true poses
    for (int r = 0; r < 3; r++) s.kfs[(size_t)c].T.v[12 + r] += 0.004 * uni();
  s.map.kfs = {&s.kfs[2], &s.kfs[0], &s.kfs[6], &s.kfs[1], &s.kfs[3], &s.kfs[4], &s.kfs[5]};
  for (int i = 0; i < NP + 2; i++) s.map.mps.push_back(&s.pts[(size_t)i]);
  s.map.mps.insert(s.map.mps.begin() + 3, nullptr);
}

struct Expected {
  std::vector<double> T, X;       // [B][16], [points of the map's list][3]
  std::vector<uint8_t> status;
};

// sd_debug_global_ba on lists built with straight loops over the map's lists
static Expected expected(const Scene& s, int n_iterations, int robust) {
  std::vector<int32_t> off(1, 0), kf;
  std::vector<float> uv, ur, inv;
  std::vector<uint8_t> kb, pb;
  std::vector<double> Xw;
  for (MapPoint* p : s.map.mps) {
    pb.push_back(!p || p->bad);
    if (p && !p->bad)
      for (const auto& ob : p->obs) {
        const KeyFrame* k = ob.first;
        const int c = (int)(k - &s.kfs[0]);
        kf.push_back(c < B ? c : 0);
        kb.push_back(c >= B);                        // keyframe 6 is bad, keyframe 7 has mnId > maxKFid
        uv.push_back(k->keys[ob.second].x); uv.push_back(k->keys[ob.second].y);
        ur.push_back(k->mvuRight[ob.second]);
        inv.push_back(1.f / (float)(1 << (2 * k->keys[ob.second].octave)));
      }
    off.push_back((int32_t)kf.size());
    for (int r = 0; r < 3; r++) Xw.push_back(p ? p->X.v[r] : 0.0);
  }
  Expected e;
  std::vector<double> T((size_t)B * 16);
  e.T.resize((size_t)B * 16); e.X.resize(Xw.size()); e.status.resize(s.map.mps.size());
  for (int c = 0; c < B; c++) std::memcpy(&T[(size_t)c * 16], s.kfs[(size_t)c].T.v, 128);
  const uint8_t roles[B] = {2, 1, 1, 1, 1, 1};
  const float cam9[9] = {FX, FY, CX, CY, BF, 0, 640, 0, 480};
  int32_t info[16];
  check(sd_debug_global_ba((int)s.map.mps.size(), off.data(), kf.data(), uv.data(), ur.data(), inv.data(), kb.data(), pb.data(), B, T.data(), roles,
                           Xw.data(), cam9, n_iterations, robust, e.T.data(), e.X.data(), e.status.data(), info), "debug entry");
  CHECK(info[0] == SD_BA_OK && info[1] == 5 && info[2] == 1 && info[3] == NP && info[6] >= 2, "info: %d %d %d %d %d", info[0], info[1], info[2], info[3], info[6]);
  return e;
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
  Scene s;
  make_scene(s);
  plant(ref_x, &s.kfs[0], B, "plant ref");
  auto frameOf = [&](KeyFrame* k) { return (int)(k - &s.kfs[0]) < B ? (int)(k - &s.kfs[0]) : -1; };
  const std::vector<MapPoint*>& mps = s.map.mps;
  double T0[16];
  std::memcpy(T0, s.kfs[2].T.v, 128);

  // ---- the stop flag: false, nothing touched
  bool stop = true;
  g_calls.clear();
  CHECK(!SD_SLAM::Optimizer::GlobalBundleAdjustemnt(batch, &s.map, 10, &stop, 0, true, frameOf, 1) && g_calls.empty(), "pbStopFlag");
  stop = false;

  // ---- nLoopKF != 0: nothing is written, the result is kept aside
  const Expected loop = expected(s, 10, 0);
  CHECK(SD_SLAM::Optimizer::BundleAdjustment(batch, s.map.kfs, mps, 10, &stop, 17ul, false, frameOf, 1), "the loop branch: %s", sd_last_error());
  CHECK(g_calls.empty(), "the loop branch calls no setter");
  for (int c = 0; c < NKF; c++) {
    const KeyFrame& k = s.kfs[(size_t)c];
    if (c < B) CHECK(k.mnBAGlobalForKF == 17 && std::memcmp(k.mTcwGBA.v, &loop.T[(size_t)c * 16], 128) == 0, "mTcwGBA of keyframe %d", c);
    else CHECK(k.mnBAGlobalForKF == 0, "keyframe %d is not of the problem", c);
  }
  CHECK(std::memcmp(s.kfs[2].mTcwGBA.v, T0, 128) != 0 && std::memcmp(s.kfs[0].mTcwGBA.v, s.kfs[0].T.v, 128) == 0, "free poses move, the fixed one does not");
  int included = 0;
  for (size_t i = 0; i < mps.size(); i++) {
    if (!mps[i]) continue;
    const bool in = loop.status[i] == SD_BA_POINT_OPTIMISED;
    included += in;
    CHECK(mps[i]->mnBAGlobalForKF == (in ? 17ul : 0ul), "mnBAGlobalForKF of entry %zu", i);
    if (in) CHECK(std::memcmp(mps[i]->mPosGBA.v, &loop.X[i * 3], 24) == 0, "mPosGBA of entry %zu", i);
  }
  CHECK(included == NP && !mps[3] && mps[NP + 1]->bad && loop.status[NP + 2] == SD_BA_POINT_SKIPPED, "%d points included", included);
  double Td[16];
  check(sd_track_debug_read(batch.handle(), 8, 2, Td, 128), "read Tref");
  CHECK(std::memcmp(Td, T0, 128) == 0, "write_back = 0 leaves Tref");

  // ---- nLoopKF == 0: SetPose on every keyframe, then per point SetWorldPos and the refresh
  const Expected init = expected(s, 10, 1);
  CHECK(SD_SLAM::Optimizer::GlobalBundleAdjustemnt(batch, &s.map, 10, &stop, 0, true, frameOf, 1), "the nLoopKF == 0 branch: %s", sd_last_error());
  std::vector<Call> want;
  for (KeyFrame* k : s.map.kfs)
    if (!k->bad) want.push_back({EV_POSE, (int)k->mnId});
  for (size_t i = 0; i < mps.size(); i++)
    if (mps[i] && init.status[i] == SD_BA_POINT_OPTIMISED) {
      want.push_back({EV_POS, mps[i]->id});
      // (point 5's reference keyframe does not observe it; keyframes 6 and 7 are not resident, and sd_track_refresh_points leaves a
      // point with such an observation to the caller, as it does after LocalBundleAdjustment)
      if (mps[i]->id != 5 && !mps[i]->obs.count(&s.kfs[6]) && !mps[i]->obs.count(&s.kfs[7])) want.push_back({EV_NORMAL, mps[i]->id});
    }
  CHECK(g_calls == want, "%zu setter calls, %zu expected, in the reference's order", g_calls.size(), want.size());
  for (int c = 0; c < B; c++) CHECK(std::memcmp(s.kfs[(size_t)c].T.v, &init.T[(size_t)c * 16], 128) == 0, "pose of keyframe %d", c);
  CHECK(std::memcmp(s.kfs[2].T.v, T0, 128) != 0, "free poses move");
  for (size_t i = 0; i < mps.size(); i++)
    if (mps[i] && init.status[i] == SD_BA_POINT_OPTIMISED) CHECK(std::memcmp(mps[i]->X.v, &init.X[i * 3], 24) == 0, "position of entry %zu", i);
  for (int i = 0; i < NP; i++) {   // UpdateNormalAndDepth over every observation, at the optimised poses and positions
    const MapPoint& p = s.pts[(size_t)i];
    if (i == 5 || i % 7 == 0) continue;   // (point 5 has no reference observation; the others' lists name keyframes that are not resident)
    const NormalAndDepth nd = update_normal_and_depth(p);
    const double* normal = nd.normal;
    const float max_dist = nd.max_dist, min_dist = nd.min_dist;
    CHECK(std::memcmp(p.normal.v, normal, 24) == 0, "normal of point %d: %.17g %.17g", p.id, p.normal.v[0], normal[0]);
    CHECK(p.max_dist == max_dist && p.min_dist == min_dist, "distances of point %d: %.9g %.9g", p.id, p.max_dist, max_dist);
  }
  check(sd_track_debug_read(batch.handle(), 8, 2, Td, 128), "read Tref");
  CHECK(std::memcmp(Td, s.kfs[2].T.v, 128) == 0, "the device holds what the objects hold");

  // ---- a refusal: keyframe 5 is not resident any more -> false, nothing touched
  auto fewer = [&](KeyFrame* k) { return (int)(k - &s.kfs[0]) < B - 1 ? (int)(k - &s.kfs[0]) : -1; };
  const size_t before = g_calls.size();
  CHECK(!SD_SLAM::Optimizer::GlobalBundleAdjustemnt(batch, &s.map, 10, nullptr, 0, true, fewer, 1), "a keyframe that is not resident");
  CHECK(g_calls.size() == before, "a refusal touches nothing");
  // ... and an observation of a keyframe that is neither in vpKFs nor newer than them: the vertex does not exist
  std::vector<KeyFrame*> without = s.map.kfs;
  without.erase(std::find(without.begin(), without.end(), &s.kfs[4]));
  CHECK(!SD_SLAM::Optimizer::BundleAdjustment(batch, without, mps, 10, nullptr, 23ul, false, frameOf, 1), "SD_BA_NO_VERTEX");
  CHECK(g_calls.size() == before && s.kfs[1].mnBAGlobalForKF == 17, "... touches nothing either");
}

#endif

int main() {
  host_part();
#ifdef RUN_ON_GPU
  gpu_part();
#endif
  std::printf("facade_global_ba OK\n");
  return 0;
}
