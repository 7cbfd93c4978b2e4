// LocalMapping::KeyFrameCulling and the erase_on_device path of Optimizer::LocalBundleAdjustment of include/sdslam/sdslam.hpp on
// reference-shaped KeyFrame / MapPoint classes that cascade as the reference's do (KeyFrame::SetBadFlag, src/KeyFrame.cc:430-446,
// the map-point part; MapPoint::EraseObservation, src/MapPoint.cc:110-134; MapPoint::SetBadFlag, :146-161).  What this test needs
// beyond tests/native/mock_map.h lives here: the classes below are the mock's with nObs, SetBadFlag and the cascade.
// Without RUN_ON_GPU (tests/test_cull_facade.py::test_facade_cull_host_side): the candidates and flags built from
// GetVectorCovisibleKeyFrames(), mnId and the not-erase predicate, the SetBadFlag calls and their order for a verdict array, and
// the scene of the device part under the straight restatement of :580-634 (it must cull, set to-be-erased and take points bad).
// With RUN_ON_GPU (::test_facade_cull_on_the_device): the method on planted keyframes against that restatement on a twin scene --
// the SetBadFlag order and the state of every object -- a device refusal and a covisible keyframe that is not resident, both
// returning false with nothing touched; then LocalBundleAdjustment with erase_on_device false and true on twin scenes with wrong
// observations, every object compared: poses, positions, observations, matches, reference keyframes, flags, normals, distances.
#include "mock_map.h"

namespace cm {

using mock::Mat4;
using mock::Vec3;

std::vector<int> g_set_bad;   // the mnId of every keyframe SetBadFlag was called on, in call order

struct MapPoint;
struct KeyFrame {
  unsigned long mnId = 0, mnBALocalForKF = ~0ul, mnBAFixedForKF = ~0ul;
  int N = 0;
  bool bad = false, mbNotErase = false, mbToBeErased = false;
  std::vector<float> mvuRight, mvDepth;
  std::vector<sd_keypoint> keys;
  std::vector<KeyFrame*> covisible;
  std::vector<MapPoint*> mps;   // by keypoint index
  Mat4 T;
  int n_set_pose = 0;
  bool isBad() const { return bad; }
  std::vector<KeyFrame*> GetVectorCovisibleKeyFrames() const { return covisible; }
  std::vector<MapPoint*> GetMapPointMatches() const { return mps; }
  Mat4 GetPose() const { return T; }
  void SetPose(const double* t) { std::memcpy(T.v, t, 128); n_set_pose++; }
  void EraseMapPointMatch(MapPoint* p) {
    for (MapPoint*& m : mps)
      if (m == p) m = nullptr;
  }
  void EraseMapPointMatch(size_t idx) { mps[idx] = nullptr; }
  int add_keypoint(float x, float y, int octave, float ur, float depth) {
    keys.push_back(sd_keypoint{x, y, 31.f, 0.f, 1.f, octave, -1});
    mvuRight.push_back(ur);
    mvDepth.push_back(depth);
    mps.push_back(nullptr);
    return N++;
  }
  inline void SetBadFlag();
};
struct ById {
  bool operator()(const KeyFrame* a, const KeyFrame* b) const { return a->mnId < b->mnId; }
};
struct MapPoint {
  int id = 0;
  unsigned long mnBALocalForKF = ~0ul;
  bool bad = false;
  int nObs = 0, n_set_pos = 0, n_set_normal = 0;
  Vec3 X, normal;
  float max_dist = 0.f, min_dist = 0.f;
  uint8_t desc[32] = {};
  std::map<KeyFrame*, size_t, ById> obs;   // (the reference keys by pointer; by id here, so that the order is the test's)
  KeyFrame* ref = nullptr;
  bool isBad() const { return bad; }
  int Observations() const { return nObs; }
  Vec3 GetWorldPos() const { return X; }
  Vec3 GetNormal() const { return normal; }
  float GetMinDistanceInvariance() const { return 0.8f * min_dist; }
  float GetMaxDistanceInvariance() const { return 1.2f * max_dist; }
  float GetMaxDistance() const { return max_dist; }
  const uint8_t* GetDescriptor() const { return desc; }
  const std::map<KeyFrame*, size_t, ById>& GetObservations() const { return obs; }
  KeyFrame* GetReferenceKeyFrame() const { return ref; }
  void EraseObservation(KeyFrame* kf) {   // src/MapPoint.cc:110-134
    bool bBad = false;
    if (obs.count(kf)) {
      const size_t idx = obs[kf];
      if (kf->mvuRight[idx] >= 0) nObs -= 2;
      else nObs--;
      obs.erase(kf);
      if (ref == kf) ref = obs.empty() ? nullptr : obs.begin()->first;
      if (nObs <= 2) bBad = true;
    }
    if (bBad) SetBadFlag();
  }
  void SetBadFlag() {   // :146-161
    bad = true;
    const auto was = obs;
    obs.clear();
    for (const auto& ob : was) ob.first->EraseMapPointMatch(ob.second);
  }
  void SetWorldPos(const double* x) { std::memcpy(X.v, x, 24); n_set_pos++; }
  void SetNormalVector(const double* n) { std::memcpy(normal.v, n, 24); n_set_normal++; }
  void SetMaxDistance(float v) { max_dist = v; }
  void SetMinDistance(float v) { min_dist = v; }
};
void KeyFrame::SetBadFlag() {   // src/KeyFrame.cc:430-446, the map-point part
  g_set_bad.push_back((int)mnId);
  if (mnId == 0) return;
  else if (mbNotErase) {
    mbToBeErased = true;
    return;
  }
  for (size_t i = 0; i < mps.size(); i++)
    if (mps[i]) mps[i]->EraseObservation(this);
  bad = true;
}

inline void observe(KeyFrame& kf, MapPoint& p, float x, float y, int octave, float ur, float depth) {
  const int k = kf.add_keypoint(x, y, octave, ur, depth);
  kf.mps[(size_t)k] = &p;
  p.obs[&kf] = (size_t)k;
  p.nObs += ur >= 0 ? 2 : 1;
  if (!p.ref) p.ref = &kf;
}

// LocalMapping::KeyFrameCulling, src/LocalMapping.cc:580-634, on the objects
inline void KeyFrameCulling(KeyFrame* mpCurrentKeyFrame, bool mbMonocular, float mThDepth) {
  for (KeyFrame* pKF : mpCurrentKeyFrame->GetVectorCovisibleKeyFrames()) {
    if (pKF->mnId == 0) continue;
    const std::vector<MapPoint*> vpMapPoints = pKF->GetMapPointMatches();
    const int thObs = 3;
    int nRedundantObservations = 0, nMPs = 0;
    for (size_t i = 0; i < vpMapPoints.size(); i++) {
      MapPoint* pMP = vpMapPoints[i];
      if (!pMP || pMP->isBad()) continue;
      if (!mbMonocular && (pKF->mvDepth[i] > mThDepth || pKF->mvDepth[i] < 0)) continue;
      nMPs++;
      if (pMP->Observations() > thObs) {
        const int scaleLevel = pKF->keys[i].octave;
        int nObs = 0;
        for (const auto& ob : pMP->GetObservations()) {
          if (ob.first == pKF) continue;
          if (ob.first->keys[ob.second].octave <= scaleLevel + 1) {
            nObs++;
            if (nObs >= thObs) break;
          }
        }
        if (nObs >= thObs) nRedundantObservations++;
      }
    }
    if (nRedundantObservations > 0.9 * nMPs) pKF->SetBadFlag();
  }
}

static const int B = 6, NKF = 7;   // keyframes 0 .. 5 are frames 0 .. 5 of the ref extractor, keyframe 6 is the current one
static const float FX = 458.654f, FY = 457.296f, CX = 367.215f, CY = 248.375f, BF = 47.9f;
static uint32_t g_seed = 2463534242u;
inline double uni() {   // (-1, 1)
  g_seed ^= g_seed << 13; g_seed ^= g_seed >> 17; g_seed ^= g_seed << 5;
  return (double)(g_seed >> 8) / 8388608.0 - 1.0;
}

struct Scene {
  std::vector<KeyFrame> kfs;
  std::vector<MapPoint> pts;
};

// Cameras on a line looking down +z (mock::pose_on_the_line's), 60 points 3.5 .. 6 m in front of them.  Always the same scene.
// dense (the culling scene): a point is seen by six of the seven cameras, points 0, 20 and 40 by cameras 2, 4 and 6 only (mono: nObs 3).
// Otherwise (the bundle-adjustment scene) by about four, and every tenth point's first observation is 45 px off; of those,
// points 3, 23 and 43 keep three mono observations, so that the erasure takes them to nObs 2.
static void make_scene(Scene& s, bool dense) {
  g_seed = 2463534242u;
  s.kfs.assign(NKF, KeyFrame());
  s.pts.assign(60, MapPoint());
  const unsigned long ids[NKF] = {0, 11, 12, 13, 4, 5, 20};   // mnId 0: the first keyframe; 20: the current keyframe
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
  for (int i = 0; i < 60; i++) {
    MapPoint& p = s.pts[(size_t)i];
    p.id = i;
    const double X[3] = {1.5 * uni(), uni(), 4.75 + 1.25 * uni()};
    const bool sparse = dense ? i % 20 == 0 : (i % 20 == 3);
    int seen = 0;
    for (int c = 0; c < NKF; c++) {
      if (dense ? (sparse ? (c != 2 && c != 4 && c != 6) : (i + c) % 7 == 0) : ((i + 2 * c) % 5 >= 3 || (sparse && seen == 3))) continue;
      const KeyFrame& k = s.kfs[(size_t)c];
      double pc[3];
      for (int r = 0; r < 3; r++) pc[r] = k.T.v[r] * X[0] + k.T.v[4 + r] * X[1] + k.T.v[8 + r] * X[2] + k.T.v[12 + r];
      double u = FX * pc[0] / pc[2] + CX + 0.4 * uni(), v = FY * pc[1] / pc[2] + CY + 0.4 * uni();
      if (!dense && seen == 0 && i % 10 == 3) u += 45.0, v -= 30.0;
      const int octave = dense ? (i + 2 * c) % 3 == 0 : (i + c) % 3;
      const float ur = !sparse && (i + c) % 2 ? (float)(u - BF / pc[2] + 0.3 * uni()) : -1.f;
      observe(s.kfs[(size_t)c], p, (float)u, (float)v, octave, ur, (float)pc[2]);
      seen++;
    }
    for (int r = 0; r < 3; r++) p.X.v[r] = X[r] + 0.02 * uni();
    std::memset(p.desc, i, 32);
  }
  for (int c : {1, 2, 3, 6})   // the local keyframes start off their true poses
    for (int r = 0; r < 3; r++) s.kfs[(size_t)c].T.v[12 + r] += 0.004 * uni();
  s.kfs[6].covisible = {&s.kfs[2], &s.kfs[1], &s.kfs[3], &s.kfs[0]};
  if (dense) {
    s.kfs[6].covisible = {&s.kfs[2], &s.kfs[1], &s.kfs[3], &s.kfs[0], &s.kfs[4], &s.kfs[5]};
    s.kfs[1].mbNotErase = true;
  }
}

// Everything a test compares of two scenes built alike: "" if equal, else what differs first
inline std::string differ(const Scene& a, const Scene& b, bool geometry) {
  char buf[128];
  for (int c = 0; c < NKF; c++) {
    const KeyFrame &x = a.kfs[(size_t)c], &y = b.kfs[(size_t)c];
    bool same = x.bad == y.bad && x.mbToBeErased == y.mbToBeErased && x.n_set_pose == y.n_set_pose && x.mps.size() == y.mps.size();
    for (size_t k = 0; same && k < x.mps.size(); k++) same = (x.mps[k] ? x.mps[k]->id : -1) == (y.mps[k] ? y.mps[k]->id : -1);
    if (geometry && same) same = std::memcmp(x.T.v, y.T.v, 128) == 0;
    if (!same) return std::snprintf(buf, sizeof buf, "keyframe %d", c), buf;
  }
  for (size_t i = 0; i < a.pts.size(); i++) {
    const MapPoint &x = a.pts[i], &y = b.pts[i];
    bool same = x.bad == y.bad && x.nObs == y.nObs && x.obs.size() == y.obs.size() && (x.ref ? (int)x.ref->mnId : -1) == (y.ref ? (int)y.ref->mnId : -1);
    auto it = y.obs.begin();
    for (auto jt = x.obs.begin(); same && jt != x.obs.end(); ++jt, ++it) same = jt->first->mnId == it->first->mnId && jt->second == it->second;
    if (geometry && same)
      same = std::memcmp(x.X.v, y.X.v, 24) == 0 && std::memcmp(x.normal.v, y.normal.v, 24) == 0 && x.max_dist == y.max_dist &&
             x.min_dist == y.min_dist && x.n_set_pos == y.n_set_pos && x.n_set_normal == y.n_set_normal;
    if (!same) return std::snprintf(buf, sizeof buf, "point %zu (bad %d %d, nObs %d %d, normals set %d %d)", i, x.bad, y.bad, x.nObs, y.nObs, x.n_set_normal, y.n_set_normal), buf;
  }
  return "";
}

}  // namespace cm

using cm::KeyFrame;
using cm::MapPoint;
using SD_SLAM::LocalMapping;

static void host_part() {
  // five covisible keyframes in an order that is not the frames'; frame 2 is the first keyframe, frame 4 must not be erased
  KeyFrame cur, kf[5];
  const int order[5] = {3, 0, 4, 2, 1};
  for (int f = 0; f < 5; f++) kf[f].mnId = f == 2 ? 0 : 10 + f;
  kf[4].mbNotErase = true;
  cur.mnId = 99;
  for (int k : order) cur.covisible.push_back(&kf[k]);
  auto frame_of = [&](KeyFrame* k) { return k >= kf && k < kf + 5 ? (int)(k - kf) : -1; };
  auto not_erase = [](KeyFrame* k) { return k->mbNotErase; };
  const auto c = LocalMapping::BuildCullCandidates(cur.GetVectorCovisibleKeyFrames(), frame_of, not_erase);
  CHECK(c.resident && c.frame == (std::vector<int32_t>{3, 0, 4, 2, 1}), "candidates in covisibility order");
  CHECK(c.flags == (std::vector<uint8_t>{0, 0, 2, 1, 0}), "flags: bit 0 mnId == 0, bit 1 mbNotErase");
  // points: p0 seen by frames 3, 0, 1 (mono): culling 3 takes it to nObs 2, it goes bad and leaves 0 and 1 as well;
  // p1 seen by 3 (stereo), 0, 1: nObs 4 -> 2, bad; p2 seen by 0, 1, 2, 4: culling 0 leaves nObs 3 and moves its reference keyframe
  MapPoint p[3];
  for (int i = 0; i < 3; i++) p[i].id = i;
  cm::observe(kf[3], p[0], 0, 0, 0, -1.f, 1.f); cm::observe(kf[0], p[0], 0, 0, 0, -1.f, 1.f); cm::observe(kf[1], p[0], 0, 0, 0, -1.f, 1.f);
  cm::observe(kf[3], p[1], 0, 0, 0, 5.f, 1.f); cm::observe(kf[0], p[1], 0, 0, 0, -1.f, 1.f); cm::observe(kf[1], p[1], 0, 0, 0, -1.f, 1.f);
  cm::observe(kf[0], p[2], 0, 0, 0, -1.f, 1.f); cm::observe(kf[1], p[2], 0, 0, 0, -1.f, 1.f); cm::observe(kf[2], p[2], 0, 0, 0, -1.f, 1.f);
  cm::observe(kf[4], p[2], 0, 0, 0, -1.f, 1.f);
  CHECK(p[2].ref == &kf[0] && p[1].nObs == 4, "the scene");
  const std::vector<uint8_t> verdict = {SD_CULL_CULLED, SD_CULL_CULLED, SD_CULL_TO_BE_ERASED, SD_CULL_SKIPPED_ID0, SD_CULL_KEPT};
  cm::g_set_bad.clear();
  const int n = LocalMapping::ApplyCullVerdicts(cur.GetVectorCovisibleKeyFrames(), verdict);
  CHECK(n == 3 && cm::g_set_bad == (std::vector<int>{13, 10, 14}), "SetBadFlag on the culled and to-be-erased keyframes, in candidate order");
  CHECK(kf[3].bad && kf[0].bad && !kf[4].bad && kf[4].mbToBeErased && !kf[1].bad && !kf[2].bad, "the objects' own SetBadFlag ran");
  CHECK(p[0].bad && p[0].obs.empty() && p[0].nObs == 2, "p0 went bad at nObs 2");
  CHECK(p[1].bad && p[1].nObs == 2, "p1: the stereo observation weighs 2");
  CHECK(!p[2].bad && p[2].nObs == 3 && p[2].ref == &kf[2] && p[2].obs.size() == 3, "p2 keeps three observations, mpRefKF moved to the first");
  CHECK(kf[1].mps[0] == nullptr && kf[1].mps[1] == nullptr && kf[1].mps[2] == &p[2], "the bad points' matches are gone");
  KeyFrame away;
  cur.covisible.push_back(&away);
  const auto c2 = LocalMapping::BuildCullCandidates(cur.GetVectorCovisibleKeyFrames(), frame_of, not_erase);
  CHECK(!c2.resident, "a covisible keyframe that is not resident");
  // the scene of the device part under the restatement: it has to be worth running
  cm::Scene s;
  cm::make_scene(s, true);
  cm::g_set_bad.clear();
  cm::KeyFrameCulling(&s.kfs[6], false, 40.f);
  int n_bad_kf = 0, n_bad_pt = 0, n_tbe = 0;
  for (const KeyFrame& k : s.kfs) n_bad_kf += k.bad, n_tbe += k.mbToBeErased;
  for (const MapPoint& q : s.pts) n_bad_pt += q.bad;
  std::printf("culling scene: %zu SetBadFlag calls, %d keyframes bad, %d to be erased, %d points bad\n", cm::g_set_bad.size(), n_bad_kf, n_tbe, n_bad_pt);
  CHECK(n_bad_kf >= 1 && n_bad_kf <= 3 && n_tbe == 1 && n_bad_pt >= 1, "the culling scene culls, keeps, sets to-be-erased and takes points bad");
}

#ifdef RUN_ON_GPU
static void check(int rc, const char* what) { CHECK(rc == SD_OK, "%s: %s", what, sd_last_error()); }

// The keypoints of kfs[0 .. n) as frames 0 .. n - 1 of an extractor
static void plant(SD_SLAM::ORBextractor& x, const KeyFrame* kfs, int n_frames, const char* what) {
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

// What the caller of KeyFrameCulling leaves resident: keypoints, mvuRight and mvDepth rows, the observation lists of every point
template <class FrameOf>
static void make_resident(SD_SLAM::ORBextractor& cur_x, SD_SLAM::ORBextractor& ref_x, SD_SLAM::TrackBatch& batch, cm::Scene& s, FrameOf frameOf) {
  plant(ref_x, &s.kfs[0], cm::B, "plant ref");
  plant(cur_x, &s.kfs[6], 1, "plant cur");
  for (int f = 0; f < cm::B; f++) {
    check(sd_track_set_uright_ref(batch.handle(), f, 1, s.kfs[(size_t)f].mvuRight.data(), s.kfs[(size_t)f].N), "uright_ref");
    check(sd_track_set_tri_depth(batch.handle(), 1, f, 1, s.kfs[(size_t)f].mvDepth.data(), s.kfs[(size_t)f].N), "tri_depth");
  }
  batch.SetURight(0, s.kfs[6].mvuRight.data(), s.kfs[6].N);
  std::vector<MapPoint*> all;
  for (MapPoint& p : s.pts) all.push_back(&p);
  SD_SLAM::ORBmatcher::ObservationLists L;
  SD_SLAM::ORBmatcher::WalkObservations(&s.kfs[6], all, true, frameOf, L, [](size_t, KeyFrame*, size_t) {});
  check(sd_track_set_observations(batch.handle(), (int)all.size(), L.off.data(), L.frame.data(), L.kp.data(), L.kf_bad.data(), L.ref_obs.data(),
                                  L.point_bad.data()), "set_observations");
}

static void cull_on_the_device(SD_SLAM::ORBextractor& cur_x, SD_SLAM::ORBextractor& ref_x, SD_SLAM::TrackBatch& batch) {
  cm::Scene want, got;
  cm::make_scene(want, true);
  cm::make_scene(got, true);
  cm::g_set_bad.clear();
  cm::KeyFrameCulling(&want.kfs[6], false, 40.f);
  const std::vector<int> want_calls = cm::g_set_bad;
  auto frameOf = [&](KeyFrame* k) { return (int)(k - &got.kfs[0]) < cm::B ? (int)(k - &got.kfs[0]) : -1; };
  // a covisible keyframe that is not resident: false, nothing touched, before anything else
  cm::g_set_bad.clear();
  auto fewer = [&](KeyFrame* k) { return (int)(k - &got.kfs[0]) < cm::B - 1 ? (int)(k - &got.kfs[0]) : -1; };
  make_resident(cur_x, ref_x, batch, got, frameOf);
  CHECK(!LocalMapping::KeyFrameCulling(batch, &got.kfs[6], false, 40.f, fewer) && cm::g_set_bad.empty(), "a covisible keyframe that is not resident");
  // a device refusal: keyframe 5 is no candidate, but the lists name it as not resident
  make_resident(cur_x, ref_x, batch, got, fewer);
  const std::vector<KeyFrame*> covisible = got.kfs[6].covisible;
  got.kfs[6].covisible.pop_back();
  CHECK(!LocalMapping::KeyFrameCulling(batch, &got.kfs[6], false, 40.f, fewer) && cm::g_set_bad.empty(), "a refusal touches nothing");
  int32_t info[8];
  check(sd_track_get_culled(batch.handle(), nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, info, 0, 0, 0), "get_culled");
  CHECK(info[0] == SD_CULL_NOT_RESIDENT, "status %d", info[0]);
  got.kfs[6].covisible = covisible;
  cm::Scene untouched;
  cm::make_scene(untouched, true);
  CHECK(cm::differ(got, untouched, true).empty(), "the refusals left the objects as they were");
  // the call
  make_resident(cur_x, ref_x, batch, got, frameOf);
  CHECK(LocalMapping::KeyFrameCulling(batch, &got.kfs[6], false, 40.f, frameOf), "the call: %s", sd_last_error());
  CHECK(cm::g_set_bad == want_calls && want_calls.size() >= 2, "%zu SetBadFlag calls, %zu expected, in candidate order", cm::g_set_bad.size(), want_calls.size());
  const std::string d = cm::differ(got, want, true);
  CHECK(d.empty(), "the objects after the device's verdicts and after the restatement differ: %s", d.c_str());
  // the device's own cascade is the objects': nObs, flags and reference keyframes point by point
  std::vector<uint8_t> pbad(60), dead(600);
  std::vector<int32_t> nobs(60), ref(60);
  check(sd_track_get_culled(batch.handle(), nullptr, nullptr, dead.data(), pbad.data(), ref.data(), nobs.data(), info, 0, 60, 600), "get_culled");
  for (size_t i = 0; i < 60; i++) {
    const MapPoint& p = got.pts[i];
    CHECK((bool)pbad[i] == p.bad && nobs[i] == p.nObs, "point %zu: device bad %d nObs %d, object bad %d nObs %d", i, pbad[i], nobs[i], p.bad, p.nObs);
  }
  // monocular: the depth gate is off (with every depth far beyond the threshold nothing counts, and nothing is culled)
  cm::make_scene(got, true);
  make_resident(cur_x, ref_x, batch, got, frameOf);
  cm::g_set_bad.clear();
  CHECK(LocalMapping::KeyFrameCulling(batch, &got.kfs[6], false, 1.f, frameOf) && cm::g_set_bad.empty(), "thDepth below every depth: nMPs = 0");
  CHECK(LocalMapping::KeyFrameCulling(batch, &got.kfs[6], true, 1.f, frameOf) && cm::g_set_bad == want_calls, "monocular ignores thDepth");
}

static void ba_both_ways(SD_SLAM::ORBextractor& cur_x, SD_SLAM::ORBextractor& ref_x, SD_SLAM::TrackBatch& batch) {
  cm::Scene s[2];
  int n_bad[2] = {0, 0}, n_erased[2] = {0, 0};
  for (int way = 0; way < 2; way++) {
    cm::make_scene(s[way], false);
    cm::Scene before;
    cm::make_scene(before, false);
    plant(ref_x, &s[way].kfs[0], cm::B, "plant ref");
    plant(cur_x, &s[way].kfs[6], 1, "plant cur");
    cm::Scene& sc = s[way];
    auto frameOf = [&](KeyFrame* k) { return (int)(k - &sc.kfs[0]) < cm::B ? (int)(k - &sc.kfs[0]) : -1; };
    bool stop = false;
    CHECK(SD_SLAM::Optimizer::LocalBundleAdjustment(batch, &sc.kfs[6], &stop, frameOf, 1, way == 1), "the call: %s", sd_last_error());
    for (size_t i = 0; i < 60; i++) n_bad[way] += sc.pts[i].bad, n_erased[way] += (int)(before.pts[i].obs.size() - sc.pts[i].obs.size());
    if (way == 1) {   // the resident lists are the objects' observations
      std::vector<int32_t> off(61), map(600);
      std::vector<uint8_t> pbad(60);
      int32_t info[8];
      check(sd_track_get_erased(batch.handle(), off.data(), nullptr, pbad.data(), nullptr, nullptr, info, 60, 0), "get_erased");
      SD_SLAM::Optimizer::LocalBaLists<KeyFrame, MapPoint> L;
      for (KeyFrame& k : sc.kfs) k.mnBALocalForKF = k.mnBAFixedForKF = ~0ul;
      for (MapPoint& q : sc.pts) q.mnBALocalForKF = ~0ul;
      cm::Scene twin;
      cm::make_scene(twin, false);
      SD_SLAM::Optimizer::LocalBaLists<KeyFrame, MapPoint> L0;
      SD_SLAM::Optimizer::BuildLocalBaLists(&twin.kfs[6], [&](KeyFrame* k) { return (int)(k - &twin.kfs[0]) < cm::B ? (int)(k - &twin.kfs[0]) : -1; }, L0);
      CHECK(L0.points.size() == 60, "%zu local points", L0.points.size());
      for (size_t i = 0; i < 60; i++) {   // list i of the device is local point i of the walk
        const MapPoint& p = sc.pts[(size_t)L0.points[i]->id];
        CHECK((size_t)(off[i + 1] - off[i]) == p.obs.size() && (bool)pbad[i] == p.bad, "list %zu: %d entries on the device, %zu on the object", i,
              off[i + 1] - off[i], p.obs.size());
      }
      CHECK(info[1] == n_erased[1] && info[2] == n_bad[1], "device erased %d / bad %d, objects %d / %d", info[1], info[2], n_erased[1], n_bad[1]);
    }
  }
  std::printf("local BA both ways: %d entries erased, %d points bad\n", n_erased[0], n_bad[0]);
  CHECK(n_erased[0] >= 3 && n_bad[0] >= 1, "the scene erases and takes a point bad");
  const std::string d = cm::differ(s[0], s[1], true);
  CHECK(d.empty(), "erase_on_device ends in another object state than the walk and upload: %s", d.c_str());
  int refreshed = 0;
  for (const MapPoint& p : s[1].pts) refreshed += p.n_set_normal;
  CHECK(refreshed >= 50, "%d points refreshed", refreshed);
}

static void gpu_part() {
  const int W = 640, H = 480, B = cm::B;
  std::vector<uint8_t> img((size_t)B * W * H);
  for (size_t i = 0; i < img.size(); i++) img[i] = (uint8_t)((i * 2654435761u) >> 24);
  SD_SLAM::ORBextractor cur_x(300, 2.0f, 3, 20, W, H, B), ref_x(300, 2.0f, 3, 20, W, H, B);
  const int cap = 512;
  std::vector<sd_keypoint> kps((size_t)B * cap);
  std::vector<uint8_t> desc((size_t)B * cap * 32);
  int32_t n_out[cm::B];
  check(sd_orb_extract_batch(ref_x.handle(), img.data(), B, W, H, W, (size_t)W * H, kps.data(), desc.data(), cap, n_out), "extract ref");
  check(sd_orb_extract_batch(cur_x.handle(), img.data(), B, W, H, W, (size_t)W * H, kps.data(), desc.data(), cap, n_out), "extract cur");
  SD_SLAM::TrackBatch batch(cur_x, ref_x, 96, B, 8);
  check(sd_track_set_camera(batch.handle(), cm::FX, cm::FY, cm::CX, cm::CY, cm::BF, 0, (float)W, 0, (float)H), "set_camera");
  cull_on_the_device(cur_x, ref_x, batch);
  ba_both_ways(cur_x, ref_x, batch);
}
#else
// The device paths compile against the header in the host build too
bool instantiate(SD_SLAM::TrackBatch& batch, KeyFrame* kf, bool* stop) {
  auto frameOf = [](KeyFrame* k) { return (int)k->mnId; };
  return LocalMapping::KeyFrameCulling(batch, kf, false, 40.f, frameOf) &&
         LocalMapping::KeyFrameCulling(batch, kf, true, 40.f, frameOf, [](KeyFrame*) { return false; }) &&
         SD_SLAM::Optimizer::LocalBundleAdjustment(batch, kf, stop, frameOf, 0, true);
}
#endif

int main() {
  host_part();
#ifdef RUN_ON_GPU
  gpu_part();
#endif
  std::printf("facade_cull OK\n");
  return 0;
}
