// What the facade tests of the map-side methods share (facade_local_ba.cc, facade_global_ba.cc, in part facade_refresh.cc): CHECK,
// KeyFrame / MapPoint / Map mocks shaped like the reference's with the members Optimizer::LocalBundleAdjustment and
// Optimizer::BundleAdjustment need, one ordered log of the setter and erase calls, a restatement of
// MapPoint::UpdateNormalAndDepth, and with RUN_ON_GPU the synthetic camera, the line of cameras and the keypoint planting.
// The mocks are in namespace mock: a test with classes of its own (facade_refresh.cc) takes the rest.
#pragma once
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

// Ow = -R^T t in the library's operation order (camera_centre); T column-major
inline void centre_of(const double* T, double* Ow) {
  for (int r = 0; r < 3; r++) Ow[r] = -((T[r * 4] * T[12] + T[r * 4 + 1] * T[13]) + T[r * 4 + 2] * T[14]);
}

// MapPoint::UpdateNormalAndDepth (src/MapPoint.cc:311-343) over p.obs in iteration order, for a point at X that p.ref observes;
// centre(keyframe, Ow) gives a camera centre, sf the extractor's scale factors.  (Compile with -ffp-contract=off.)
struct NormalAndDepth {
  double normal[3];
  float max_dist, min_dist;
};
template <class MapPointT, class Centre>
inline NormalAndDepth update_normal_and_depth(const MapPointT& p, const double* X, const float* sf, int nlevels, Centre centre) {
  NormalAndDepth out = {{0, 0, 0}, 0.f, 0.f};
  double Ow[3], d[3];
  int n = 0;
  for (const auto& ob : p.obs) {
    centre(ob.first, Ow);
    for (int k = 0; k < 3; k++) d[k] = X[k] - Ow[k];
    const double len = std::sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
    for (int k = 0; k < 3; k++) out.normal[k] = out.normal[k] + d[k] / len;
    n++;
  }
  for (int k = 0; k < 3; k++) out.normal[k] = out.normal[k] / n;
  centre(p.ref, Ow);
  for (int k = 0; k < 3; k++) d[k] = X[k] - Ow[k];
  const float dist = (float)std::sqrt((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
  out.max_dist = dist * sf[p.ref->keys[p.obs.at(p.ref)].octave];
  out.min_dist = out.max_dist / sf[nlevels - 1];
  return out;
}

namespace mock {

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

// Every call that changes a mock, in call order: (what, keyframe mnId or point id, for the two erasures the keyframe's mnId)
enum { EV_POSE = 0, EV_POS = 1, EV_NORMAL = 2, EV_ERASE_MATCH = 3, EV_ERASE_OBS = 4 };
struct Call {
  int what, id, kf = -1;
  bool operator==(const Call& o) const { return what == o.what && id == o.id && kf == o.kf; }
};
static std::vector<Call> g_calls;
inline int count_calls(int what, int id) {
  return (int)std::count_if(g_calls.begin(), g_calls.end(), [&](const Call& c) { return c.what == what && c.id == id; });
}
inline std::vector<std::pair<int, int>> erased() {   // EraseObservation: (keyframe mnId, point id), in call order
  std::vector<std::pair<int, int>> out;
  for (const Call& c : g_calls)
    if (c.what == EV_ERASE_OBS) out.push_back({c.kf, c.id});
  return out;
}

struct MapPoint;
struct KeyFrame {
  unsigned long mnId = 0, mnBALocalForKF = ~0ul, mnBAFixedForKF = ~0ul, mnBAGlobalForKF = 0;
  int N = 0;
  bool bad = false;
  std::vector<float> mvuRight;
  std::vector<sd_keypoint> keys;
  std::vector<KeyFrame*> covisible;
  std::vector<MapPoint*> mps;   // by keypoint index
  Mat4 T, mTcwGBA;
  bool isBad() const { return bad; }
  std::vector<KeyFrame*> GetVectorCovisibleKeyFrames() const { return covisible; }
  std::vector<MapPoint*> GetMapPointMatches() const { return mps; }
  Mat4 GetPose() const { return T; }
  void SetPose(const double* t) { std::memcpy(T.v, t, 128); g_calls.push_back({EV_POSE, (int)mnId}); }
  inline void EraseMapPointMatch(MapPoint* p);
  int add_keypoint(float x, float y, int octave, float ur) {
    keys.push_back(sd_keypoint{x, y, 31.f, 0.f, 1.f, octave, -1});
    mvuRight.push_back(ur);
    mps.push_back(nullptr);
    return N++;
  }
  int set_pose() const { return count_calls(EV_POSE, (int)mnId); }
};
struct ById {
  bool operator()(const KeyFrame* a, const KeyFrame* b) const { return a->mnId < b->mnId; }
};
struct MapPoint {
  int id = 0;
  unsigned long mnBALocalForKF = ~0ul, mnBAGlobalForKF = 0;
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
  void EraseObservation(KeyFrame* kf) {
    g_calls.push_back({EV_ERASE_OBS, id, (int)kf->mnId});
    obs.erase(kf);
  }
  void SetWorldPos(const double* x) { std::memcpy(X.v, x, 24); g_calls.push_back({EV_POS, id}); }
  void SetNormalVector(const double* n) { std::memcpy(normal.v, n, 24); g_calls.push_back({EV_NORMAL, id}); }
  void SetMaxDistance(float v) { max_dist = v; }
  void SetMinDistance(float v) { min_dist = v; }
  int set_pos() const { return count_calls(EV_POS, id); }
  int set_normal() const { return count_calls(EV_NORMAL, id); }
};
inline void KeyFrame::EraseMapPointMatch(MapPoint* p) {
  for (MapPoint*& m : mps)
    if (m == p) m = nullptr, g_calls.push_back({EV_ERASE_MATCH, p->id, (int)mnId});
}
struct Map {
  std::vector<KeyFrame*> kfs;
  std::vector<MapPoint*> mps;
  std::vector<KeyFrame*> GetAllKeyFrames() const { return kfs; }
  std::vector<MapPoint*> GetAllMapPoints() const { return mps; }
};

// A new keypoint of kf that is an observation of p, and p the keyframe's match there
inline void observe(KeyFrame& kf, MapPoint& p, float x, float y, int octave, float ur) {
  const int k = kf.add_keypoint(x, y, octave, ur);
  kf.mps[(size_t)k] = &p;
  p.obs[&kf] = (size_t)k;
}

// UpdateNormalAndDepth of p as it stands, for an extractor of scale factor 2 and three levels
inline NormalAndDepth update_normal_and_depth(const MapPoint& p) {
  static const float sf[3] = {1.f, 2.f, 4.f};
  return ::update_normal_and_depth(p, p.X.v, sf, 3, [](const KeyFrame* k, double* Ow) { centre_of(k->T.v, Ow); });
}

#ifdef RUN_ON_GPU
inline void check(int rc, const char* what) { CHECK(rc == SD_OK, "%s: %s", what, sd_last_error()); }
static uint32_t g_seed = 2463534242u;
inline double uni() {   // (-1, 1)
  g_seed ^= g_seed << 13; g_seed ^= g_seed >> 17; g_seed ^= g_seed << 5;
  return (double)(g_seed >> 8) / 8388608.0 - 1.0;
}

static const float FX = 458.654f, FY = 457.296f, CX = 367.215f, CY = 248.375f, BF = 47.9f;

// Camera c of a line of cameras looking down +z
inline void pose_on_the_line(KeyFrame& k, int c) {
  const double ang = 0.03 * (c - 3), centre[3] = {0.3 * c - 0.9, 0.02 * c, -0.01 * c};
  const double cs = std::cos(ang), sn = std::sin(ang);
  const double R[3][3] = {{cs, 0, sn}, {0, 1, 0}, {-sn, 0, cs}};
  for (int r = 0; r < 3; r++) {
    for (int cc = 0; cc < 3; cc++) k.T.v[cc * 4 + r] = R[r][cc];
    k.T.v[12 + r] = -(R[r][0] * centre[0] + R[r][1] * centre[1] + R[r][2] * centre[2]);
  }
}

// The keypoints of kfs[0 .. n) as frames 0 .. n - 1 of an extractor
inline void plant(SD_SLAM::ORBextractor& x, const KeyFrame* kfs, int n_frames, const char* what) {
  const int cap = 128;
  std::vector<sd_keypoint> kps((size_t)n_frames * cap, sd_keypoint{0, 0, 0, 0, 0, 0, -1});
  std::vector<uint8_t> desc((size_t)n_frames * cap * 32, 0);
  std::vector<int32_t> n((size_t)n_frames);
  for (int f = 0; f < n_frames; f++) {
    CHECK(kfs[f].N <= cap, "%s: keyframe %d has %d keypoints", what, f, kfs[f].N);
    n[(size_t)f] = kfs[f].N;
    std::copy(kfs[f].keys.begin(), kfs[f].keys.end(), kps.begin() + (size_t)f * cap);
  }
  check(sd_debug_orb_set_keypoints(x.handle(), 0, n_frames, n.data(), kps.data(), desc.data(), cap), what);
}
#endif

}   // namespace mock
