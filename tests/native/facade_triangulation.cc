// The C++ facade's ORBmatcher::SearchForTriangulation overloads against a stand-in KeyFrame with the reference's member
// names: compiles, links and prints "facade triangulation ok" (no GPU work).
#include <sdslam/sdslam.hpp>

#include <array>
#include <cstdio>
#include <vector>

struct MapPoint {};
struct Pose {
  std::array<double, 16> m;
  const double* data() const { return m.data(); }
};
struct KeyFrame {
  int N = 0;
  std::vector<MapPoint*> mvpMapPoints;
  std::vector<float> mvuRight;
  Pose Tcw;
  std::vector<MapPoint*> GetMapPointMatches() { return mvpMapPoints; }
  Pose GetPose() { return Tcw; }
};
struct Matrix3d {
  double v[9];
  double operator()(int r, int c) const { return v[r * 3 + c]; }
};
typedef std::vector<std::pair<size_t, size_t> > Pairs;

int main() {
  using namespace SD_SLAM;
  int (ORBmatcher::*one)(TrackBatch&, KeyFrame*, KeyFrame*, const Matrix3d&, Pairs&, int) = &ORBmatcher::SearchForTriangulation<KeyFrame, Matrix3d>;
  void (ORBmatcher::*many)(TrackBatch&, KeyFrame*, const std::vector<KeyFrame*>&, std::vector<Pairs>&, int) =
      &ORBmatcher::SearchForTriangulation<KeyFrame>;
  auto res = &ORBmatcher::TriangulationResult;
  if (!one || !many || !res) return 1;
  std::printf("facade triangulation ok\n");
  return 0;
}
