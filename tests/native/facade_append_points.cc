// The C++ facade's ORBmatcher::CreateNewMapPoints overload that appends the new points to a local row on the device, against
// stand-in KeyFrame / MapPoint classes with the reference's member names.  No GPU work: the template is instantiated (compiles
// and links against the library), and the in-order walk that turns the device's four integers per point into objects
// (WalkAppendedPoints) runs on rows written here.  Prints "facade append points ok".
#include <sdslam/sdslam.hpp>

#include <array>
#include <cstdio>
#include <list>
#include <vector>

struct KeyFrame;
struct MapPoint {
  int id = -1, row_pos = -1;
  KeyFrame* ref = nullptr;
  std::vector<std::pair<KeyFrame*, size_t> > obs;
  void AddObservation(KeyFrame* kf, size_t idx) { obs.push_back(std::make_pair(kf, idx)); }
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
  auto make_point = [&](KeyFrame* pRefKF, int32_t id, int32_t pos) {
    MapPoint* p = new MapPoint();
    p->id = id;
    p->row_pos = pos;
    p->ref = pRefKF;
    made.push_back(p);
    return p;
  };
  std::list<MapPoint*> recent;
  int (ORBmatcher::*create)(TrackBatch&, KeyFrame*, const std::vector<KeyFrame*>&, bool, int32_t, decltype(make_point), std::list<MapPoint*>&,
                            int, int, int, std::vector<int32_t>&) =
      &ORBmatcher::CreateNewMapPoints<KeyFrame, decltype(make_point), std::list<MapPoint*> >;
  if (!create) return 1;

  // four points as sd_track_get_new_points numbers them, of which the row took the first three behind its 5 points
  KeyFrame kf1(8), n0(8), n1(8);
  std::vector<KeyFrame*> neigh = {&n0, &n1};
  ORBmatcher::NewPointRows r;
  r.kp1 = {2, 5, 3, 6};
  r.slot = {0, 0, 1, 1};
  r.idx2 = {7, 1, 4, 0};
  r.id = {40, 41, 42, 43};
  std::vector<int32_t> pos;
  const int nnew = ORBmatcher::WalkAppendedPoints(r, 5, 3, &kf1, neigh, make_point, recent, pos);
  EXPECT(nnew == 3 && made.size() == 3 && recent.size() == 3);
  EXPECT(pos == (std::vector<int32_t>{5, 6, 7}));
  int p = 0;
  for (MapPoint* mp : recent) {                       // mlpRecentAddedMapPoints keeps the creation order
    KeyFrame* kf2 = neigh[(size_t)r.slot[p]];
    EXPECT(mp == made[(size_t)p] && mp->id == r.id[p] && mp->ref == &kf1 && mp->row_pos == 5 + p);
    EXPECT(mp->obs.size() == 2 && mp->obs[0].first == &kf1 && mp->obs[0].second == (size_t)r.kp1[p]);   // KF1 first, as :404-405
    EXPECT(mp->obs[1].first == kf2 && mp->obs[1].second == (size_t)r.idx2[p]);
    EXPECT(kf1.mvpMapPoints[(size_t)r.kp1[p]] == mp && kf2->mvpMapPoints[(size_t)r.idx2[p]] == mp);
    p++;
  }
  EXPECT(kf1.mvpMapPoints[6] == nullptr && n1.mvpMapPoints[0] == nullptr);   // the dropped point: no object, no AddMapPoint
  int held = 0;
  for (KeyFrame* kf : {&kf1, &n0, &n1})
    for (MapPoint* mp : kf->mvpMapPoints) held += mp != nullptr;
  EXPECT(held == 6);
  // nothing appended (a full row, or no points): no object; a negative count is no count
  ORBmatcher::NewPointRows none;
  EXPECT(ORBmatcher::WalkAppendedPoints(none, 5, 0, &kf1, neigh, make_point, recent, pos) == 0 && recent.size() == 3 && pos.size() == 3);
  EXPECT(ORBmatcher::WalkAppendedPoints(r, 9, 0, &kf1, neigh, make_point, recent, pos) == 0 && made.size() == 3);
  EXPECT(ORBmatcher::WalkAppendedPoints(r, 9, -1, &kf1, neigh, make_point, recent, pos) == 0 && made.size() == 3);
  for (MapPoint* mp : made) delete mp;
  std::printf("facade append points ok\n");
  return 0;
}
