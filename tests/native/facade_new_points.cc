// The C++ facade's ORBmatcher::CreateNewMapPoints against stand-in KeyFrame / MapPoint classes with the reference's member
// names.  No GPU work: the template is instantiated (compiles and links against the library), and the in-order walk that turns
// the device's rows into objects (WalkNewPoints) runs on rows written here.  Prints "facade new points ok".
#include <sdslam/sdslam.hpp>

#include <array>
#include <cstdio>
#include <cstring>
#include <list>
#include <vector>

struct KeyFrame;
struct MapPoint {
  int id = -1;
  double pos[3] = {}, normal[3] = {};
  float max_distance = 0.f, min_distance = 0.f;
  uint8_t desc[32] = {};
  KeyFrame* ref = nullptr;
  std::vector<std::pair<KeyFrame*, size_t> > obs;
  void AddObservation(KeyFrame* kf, size_t idx) { obs.push_back(std::make_pair(kf, idx)); }
  void SetDescriptor(const uint8_t* d) { std::memcpy(desc, d, 32); }
  void SetNormalVector(const double* n) { std::memcpy(normal, n, sizeof(normal)); }
  void SetMaxDistance(float d) { max_distance = d; }
  void SetMinDistance(float d) { min_distance = d; }
};
struct Pose {
  std::array<double, 16> m;
  const double* data() const { return m.data(); }
};
struct KeyFrame {
  int N = 0;
  std::vector<MapPoint*> mvpMapPoints;
  std::vector<float> mvuRight, mvDepth;
  Pose Tcw{};
  std::vector<MapPoint*> GetMapPointMatches() { return mvpMapPoints; }
  Pose GetPose() { return Tcw; }
  float ComputeSceneMedianDepth(int) { return 2.f; }
  void AddMapPoint(MapPoint* p, size_t idx) { mvpMapPoints[idx] = p; }
  explicit KeyFrame(int n) : N(n), mvpMapPoints(n, nullptr), mvuRight(n, -1.f), mvDepth(n, -1.f) {}
};

#define EXPECT(cond)                                            \
  do {                                                          \
    if (!(cond)) {                                              \
      std::printf("line %d: %s is false\n", __LINE__, #cond);   \
      return 1;                                                 \
    }                                                           \
  } while (0)

int main() {
  using namespace SD_SLAM;
  std::vector<MapPoint*> made;
  auto make_point = [&](const double* Xw, KeyFrame* pRefKF, int32_t id) {
    MapPoint* p = new MapPoint();
    p->id = id;
    std::memcpy(p->pos, Xw, sizeof(p->pos));
    p->ref = pRefKF;
    made.push_back(p);
    return p;
  };
  std::list<MapPoint*> recent;
  int (ORBmatcher::*create)(TrackBatch&, KeyFrame*, const std::vector<KeyFrame*>&, bool, int32_t, decltype(make_point), std::list<MapPoint*>&,
                            int) = &ORBmatcher::CreateNewMapPoints<KeyFrame, decltype(make_point), std::list<MapPoint*> >;
  if (!create) return 1;

  // three rows as sd_track_get_new_points returns them: (slot, idx1) order, ids counting on
  KeyFrame kf1(8), n0(8), n1(8);
  std::vector<KeyFrame*> neigh = {&n0, &n1};
  ORBmatcher::NewPointRows r;
  r.kp1 = {2, 5, 3};
  r.slot = {0, 0, 1};
  r.idx2 = {7, 1, 4};
  r.id = {40, 41, 42};
  for (int p = 0; p < 3; p++) {
    for (int k = 0; k < 3; k++) {
      r.Xw.push_back(p + 0.25 * k);
      r.normal.push_back(-p - 0.5 * k);
    }
    r.max_dist.push_back(10.f + p);
    r.min_dist.push_back(1.f + p);
    for (int k = 0; k < 32; k++) r.desc.push_back((uint8_t)(p * 32 + k));
  }
  const int nnew = ORBmatcher::WalkNewPoints(r, &kf1, neigh, make_point, recent);
  EXPECT(nnew == 3 && made.size() == 3 && recent.size() == 3);
  int p = 0;
  for (MapPoint* mp : recent) {                       // mlpRecentAddedMapPoints keeps the creation order
    KeyFrame* kf2 = neigh[(size_t)r.slot[p]];
    EXPECT(mp == made[(size_t)p] && mp->id == r.id[p] && mp->ref == &kf1);
    EXPECT(mp->pos[0] == p && mp->pos[2] == p + 0.5 && mp->normal[1] == -p - 0.5);
    EXPECT(mp->max_distance == 10.f + p && mp->min_distance == 1.f + p);
    EXPECT(mp->desc[0] == p * 32 && mp->desc[31] == p * 32 + 31);
    EXPECT(mp->obs.size() == 2 && mp->obs[0].first == &kf1 && mp->obs[0].second == (size_t)r.kp1[p]);   // KF1 first, as :404-405
    EXPECT(mp->obs[1].first == kf2 && mp->obs[1].second == (size_t)r.idx2[p]);
    EXPECT(kf1.mvpMapPoints[(size_t)r.kp1[p]] == mp && kf2->mvpMapPoints[(size_t)r.idx2[p]] == mp);
    p++;
  }
  int held = 0;
  for (KeyFrame* kf : {&kf1, &n0, &n1})
    for (MapPoint* mp : kf->mvpMapPoints) held += mp != nullptr;
  EXPECT(held == 6);                                  // nothing else was touched
  ORBmatcher::NewPointRows none;
  EXPECT(ORBmatcher::WalkNewPoints(none, &kf1, neigh, make_point, recent) == 0 && recent.size() == 3);
  for (MapPoint* mp : made) delete mp;
  std::printf("facade new points ok\n");
  return 0;
}
