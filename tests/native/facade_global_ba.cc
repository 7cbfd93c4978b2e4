// Optimizer::BundleAdjustment / GlobalBundleAdjustemnt of include/sdslam/sdslam.hpp on mock KeyFrame / MapPoint / Map classes shaped
// like the reference's (tests/test_global_ba_facade.py, linked against the library).  The host part checks the roles and the CSR
// lists (BuildGlobalBaLists) against lists typed in below.  The device part plants six keyframes, runs the method through both
// nLoopKF branches and compares what the objects were given, byte for byte, with sd_debug_global_ba on lists built by straight
// loops; the order of the SetPose / SetWorldPos / refresh calls with the reference's (:185-217); the normals and distances with a
// restatement of MapPoint::UpdateNormalAndDepth; and checks that a set stop flag and a refusal return false and touch nothing.
#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <utility>
#include <vector>

#include "sdslam/sdslam.hpp"

#define CHECK(cond, ...)                 \
  do {                                   \
    if (!(cond)) {                       \
      std::printf("FAILED %s: ", #cond); \
      std::printf(__VA_ARGS__);          \
      std::printf("\n");                 \
      std::exit(1);                      \
    }                                    \
  } while (0)

struct Mat4 {
  double v[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};   // column-major
  const double* data() const { return v; }
  double* data() { return v; }
};
struct Vec3 {
  double v[3] = {0, 0, 0};
  double operator()(int k) const { return v[k]; }
  double* data() { return v; }
};
struct MapPoint;
enum { EV_POSE = 0, EV_POS = 1, EV_NORMAL = 2 };
static std::vector<std::pair<int, int>> g_calls;   // (what, keyframe mnId or point id), in call order

struct KeyFrame {
  unsigned long mnId = 0, mnBAGlobalForKF = 0;
  int N = 0;
  bool bad = false;
  std::vector<float> mvuRight;
  std::vector<sd_keypoint> keys;
  Mat4 T, mTcwGBA;
  bool isBad() const { return bad; }
  Mat4 GetPose() const { return T; }
  void SetPose(const double* t) { std::memcpy(T.v, t, 128); g_calls.push_back({EV_POSE, (int)mnId}); }
  int add_keypoint(float x, float y, int octave, float ur) {
    keys.push_back(sd_keypoint{x, y, 31.f, 0.f, 1.f, octave, -1});
    mvuRight.push_back(ur);
    return N++;
  }
};
struct ById {
  bool operator()(const KeyFrame* a, const KeyFrame* b) const { return a->mnId < b->mnId; }
};
struct MapPoint {
  int id = 0;
  unsigned long mnBAGlobalForKF = 0;
  bool bad = false;
  Vec3 X, normal, mPosGBA;
  float max_dist = 0.f, min_dist = 0.f;
  uint8_t desc[32] = {};
  std::map<KeyFrame*, size_t, ById> obs;   // (the reference keys by pointer; by id here, so that the order is the test's)
  KeyFrame* ref = nullptr;
  bool isBad() const { return bad; }
  Vec3 GetWorldPos() const { return X; }
  Vec3 GetNormal() const { return normal; }
  float GetMinDistanceInvariance() const { return 0.8f * min_dist; }
  float GetMaxDistanceInvariance() const { return 1.2f * max_dist; }
  float GetMaxDistance() const { return max_dist; }
  const uint8_t* GetDescriptor() const { return desc; }
  const std::map<KeyFrame*, size_t, ById>& GetObservations() const { return obs; }
  KeyFrame* GetReferenceKeyFrame() const { return ref; }
  void SetWorldPos(const double* x) { std::memcpy(X.v, x, 24); g_calls.push_back({EV_POS, id}); }
  void SetNormalVector(const double* n) { std::memcpy(normal.v, n, 24); g_calls.push_back({EV_NORMAL, id}); }
  void SetMaxDistance(float v) { max_dist = v; }
  void SetMinDistance(float v) { min_dist = v; }
};
struct Map {
  std::vector<KeyFrame*> kfs;
  std::vector<MapPoint*> mps;
  std::vector<KeyFrame*> GetAllKeyFrames() const { return kfs; }
  std::vector<MapPoint*> GetAllMapPoints() const { return mps; }
};

static void observe(KeyFrame& kf, MapPoint& p, float x, float y, int octave, float ur) {
  p.obs[&kf] = (size_t)kf.add_keypoint(x, y, octave, ur);
}

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

static void check(int rc, const char* what) { CHECK(rc == SD_OK, "%s: %s", what, sd_last_error()); }
static uint32_t g_seed = 2463534242u;
static double uni() {   // (-1, 1)
  g_seed ^= g_seed << 13; g_seed ^= g_seed >> 17; g_seed ^= g_seed << 5;
  return (double)(g_seed >> 8) / 8388608.0 - 1.0;
}

static const float FX = 458.654f, FY = 457.296f, CX = 367.215f, CY = 248.375f, BF = 47.9f;
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
    KeyFrame& k = s.kfs[(size_t)c];
    k.mnId = ids[c];
    const double ang = 0.03 * (c - 3), centre[3] = {0.3 * c - 0.9, 0.02 * c, -0.01 * c};
    const double cs = std::cos(ang), sn = std::sin(ang);
    const double R[3][3] = {{cs, 0, sn}, {0, 1, 0}, {-sn, 0, cs}};
    for (int r = 0; r < 3; r++) {
      for (int cc = 0; cc < 3; cc++) k.T.v[cc * 4 + r] = R[r][cc];
      k.T.v[12 + r] = -(R[r][0] * centre[0] + R[r][1] * centre[1] + R[r][2] * centre[2]);
    }
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

static void plant(SD_SLAM::ORBextractor& ref_x, Scene& s) {
  const int cap = 128;
  std::vector<sd_keypoint> kps((size_t)B * cap, sd_keypoint{0, 0, 0, 0, 0, 0, -1});
  std::vector<uint8_t> desc((size_t)B * cap * 32, 0);
  int32_t n[B];
  for (int f = 0; f < B; f++) {
    CHECK(s.kfs[(size_t)f].N <= cap, "keyframe %d has %d keypoints", f, s.kfs[(size_t)f].N);
    n[f] = s.kfs[(size_t)f].N;
    std::copy(s.kfs[(size_t)f].keys.begin(), s.kfs[(size_t)f].keys.end(), kps.begin() + (size_t)f * cap);
  }
  check(sd_debug_orb_set_keypoints(ref_x.handle(), 0, B, n, kps.data(), desc.data(), cap), "plant ref");
}

static void centre_of(const double* T, double* Ow) {   // Ow = -R^T t in the library's operation order
  for (int r = 0; r < 3; r++) Ow[r] = -((T[r * 4] * T[12] + T[r * 4 + 1] * T[13]) + T[r * 4 + 2] * T[14]);
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
  plant(ref_x, s);
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
  std::vector<std::pair<int, int>> want;
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
    double normal[3] = {0, 0, 0}, Ow[3], d[3];
    int n = 0;
    for (const auto& ob : p.obs) {
      centre_of(ob.first->T.v, Ow);
      for (int k = 0; k < 3; k++) d[k] = p.X.v[k] - Ow[k];
      const double len = std::sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
      for (int k = 0; k < 3; k++) normal[k] = normal[k] + d[k] / len;
      n++;
    }
    for (int k = 0; k < 3; k++) normal[k] = normal[k] / n;
    centre_of(p.ref->T.v, Ow);
    for (int k = 0; k < 3; k++) d[k] = p.X.v[k] - Ow[k];
    const float dist = (float)std::sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
    const float max_dist = dist * (float)(1 << p.ref->keys[p.obs.at(p.ref)].octave), min_dist = max_dist / 4.f;
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

int main() {
  host_part();
  gpu_part();
  std::printf("facade_global_ba OK\n");
  return 0;
}
