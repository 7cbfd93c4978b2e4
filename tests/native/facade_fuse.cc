// The C++ facade's ORBmatcher::Fuse overloads against stand-in KeyFrame / MapPoint classes with the reference's member names;
// MapPoint::Replace / AddObservation follow src/MapPoint.cc.
//   facade_fuse            link check: prints "facade fuse ok" (no GPU work)
//   facade_fuse IN OUT     builds the toy map in IN, extracts its keyframes' images on the GPU, runs Fuse (mode 0: the vector
//                          overload over all target keyframes; 1: the Sim3 overload on keyframe 0) and writes nFused,
//                          vpReplacePoint and the map's state to OUT (layout: tests/test_fuse_facade.py)
#include <sdslam/sdslam.hpp>

#include <algorithm>
#include <array>
#include <cstdio>
#include <set>
#include <vector>

struct KeyFrame;
struct Vec3 {
  double v[3];
  double operator()(int i) const { return v[i]; }
};
struct MapPoint {
  int id = -1;
  Vec3 pos{}, normal{};
  float min_distance = 0.f, max_distance = 0.f, mf_max_distance = 1.f;
  uint8_t desc[32] = {};
  bool bad = false;
  MapPoint* replaced = nullptr;
  std::vector<std::pair<KeyFrame*, size_t> > obs;
  bool isBad() { return bad; }
  bool IsInKeyFrame(KeyFrame* kf) {
    for (auto& o : obs)
      if (o.first == kf) return true;
    return false;
  }
  int Observations() { return (int)obs.size(); }
  void AddObservation(KeyFrame* kf, size_t idx) {
    if (!IsInKeyFrame(kf)) obs.push_back(std::make_pair(kf, idx));
  }
  inline void Replace(MapPoint* other);
  Vec3 GetWorldPos() { return pos; }
  Vec3 GetNormal() { return normal; }
  float GetMinDistanceInvariance() { return min_distance; }
  float GetMaxDistanceInvariance() { return max_distance; }
  float GetMaxDistance() { return mf_max_distance; }
  const uint8_t* GetDescriptor() { return desc; }
};
struct Pose {
  std::array<double, 16> m;
  const double* data() const { return m.data(); }
};
struct KeyFrame {
  int id = -1, N = 0;
  std::vector<MapPoint*> mvpMapPoints;
  std::vector<float> mvuRight;
  Pose Tcw{};
  Pose GetPose() { return Tcw; }
  MapPoint* GetMapPoint(size_t idx) { return mvpMapPoints[idx]; }
  void AddMapPoint(MapPoint* p, size_t idx) { mvpMapPoints[idx] = p; }
  std::set<MapPoint*> GetMapPoints() {
    std::set<MapPoint*> s;
    for (MapPoint* p : mvpMapPoints)
      if (p && !p->isBad()) s.insert(p);
    return s;
  }
};
// src/MapPoint.cc, MapPoint::Replace: this point goes bad, its observations move to `other` or are erased where it is there already
inline void MapPoint::Replace(MapPoint* other) {
  if (other == this) return;
  std::vector<std::pair<KeyFrame*, size_t> > old;
  old.swap(obs);
  bad = true;
  replaced = other;
  for (auto& o : old) {
    if (!other->IsInKeyFrame(o.first)) {
      o.first->mvpMapPoints[o.second] = other;
      other->AddObservation(o.first, o.second);
    } else {
      o.first->mvpMapPoints[o.second] = nullptr;
    }
  }
}
struct Matrix4d {
  double v[16];
  double operator()(int r, int c) const { return v[r * 4 + c]; }
};

template <typename T>
static bool rd(FILE* f, std::vector<T>& v, size_t n) {
  v.resize(n);
  return n == 0 || fread(v.data(), sizeof(T), n, f) == n;
}
static void wr(FILE* f, const std::vector<int32_t>& v) { fwrite(v.data(), 4, v.size(), f); }

int main(int argc, char** argv) {
  using namespace SD_SLAM;
  typedef std::vector<MapPoint*> Points;
  if (argc < 3) {
    int (ORBmatcher::*one)(TrackBatch&, KeyFrame*, const Points&, float) = &ORBmatcher::Fuse<KeyFrame, MapPoint>;
    void (ORBmatcher::*many)(TrackBatch&, const std::vector<KeyFrame*>&, const Points&, float, std::vector<int>&) =
        &ORBmatcher::Fuse<KeyFrame, MapPoint>;
    int (ORBmatcher::*sim3)(TrackBatch&, KeyFrame*, const Matrix4d&, const Points&, float, Points&) = &ORBmatcher::Fuse<KeyFrame, Matrix4d, MapPoint>;
    int (TrackBatch::*mp)() const = &TrackBatch::max_points;
    if (!one || !many || !sim3 || !mp) return 1;
    if (sd_track_fuse(nullptr, 1, 0, -1, 3.f, 0) != SD_ERR_INVALID_ARG || sd_track_get_fuse(nullptr, 0, 1, nullptr, nullptr, 0, nullptr) != SD_ERR_INVALID_ARG)
      return 2;
    std::printf("facade fuse ok\n");
    return 0;
  }
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  std::vector<int32_t> hdr, kf_sizes, ob;   // hdr: W, H, B, n_pts, M, points in all, keyframes in all, observations, mode, nfeatures
  std::vector<float> cam, th, uright, mn, mx, mf;
  std::vector<double> scw, poses, Xw, nrm;
  std::vector<uint8_t> images, exists, desc;
  if (!rd(f, hdr, 10)) return 3;
  const int W = hdr[0], H = hdr[1], B = hdr[2], n_pts = hdr[3], M = hdr[4], n_all = hdr[5], n_kfs = hdr[6], n_obs = hdr[7], mode = hdr[8], NF = hdr[9];
  bool ok = rd(f, cam, 5) && rd(f, th, 1) && rd(f, scw, 16) && rd(f, images, (size_t)B * W * H) && rd(f, poses, (size_t)B * 16) &&
            rd(f, uright, (size_t)B * NF) && rd(f, exists, n_pts) && rd(f, Xw, (size_t)n_pts * 3) && rd(f, nrm, (size_t)n_pts * 3) &&
            rd(f, mn, n_pts) && rd(f, mx, n_pts) && rd(f, mf, n_pts) && rd(f, desc, (size_t)n_pts * 32) && rd(f, kf_sizes, n_kfs) &&
            rd(f, ob, (size_t)n_obs * 4);
  std::fclose(f);
  if (!ok) return 4;

  ORBextractor cur(NF, 1.2f, 8, 20, W, H, B), ref(NF, 1.2f, 8, 20, W, H, B);
  TrackBatch batch(cur, ref, M, B, 8);
  batch.SetCamera(cam[0], cam[1], cam[2], cam[3], cam[4], 0.f, (float)W, 0.f, (float)H);
  std::vector<KeyPoint> kps((size_t)B * NF);
  std::vector<uint8_t> dsc((size_t)B * NF * 32);
  std::vector<int32_t> nkp(B);
  check(sd_orb_extract_batch(ref.handle(), images.data(), B, W, H, W, (size_t)W * H, kps.data(), dsc.data(), NF, nkp.data()));

  std::vector<MapPoint> all(n_all);
  std::vector<KeyFrame> kfs(n_kfs);
  for (int i = 0; i < n_all; i++) all[i].id = i;
  for (int i = 0; i < n_pts; i++) {
    MapPoint& p = all[i];
    for (int k = 0; k < 3; k++) {
      p.pos.v[k] = Xw[(size_t)i * 3 + k];
      p.normal.v[k] = nrm[(size_t)i * 3 + k];
    }
    p.min_distance = mn[i];
    p.max_distance = mx[i];
    p.mf_max_distance = mf[i];
    std::copy(desc.begin() + (size_t)i * 32, desc.begin() + (size_t)(i + 1) * 32, p.desc);
  }
  for (int k = 0; k < n_kfs; k++) {
    KeyFrame& kf = kfs[k];
    kf.id = k;
    kf.N = k < B ? nkp[k] : kf_sizes[k];
    if (k < B && kf.N != kf_sizes[k]) return 6;   // the map was built for the keypoints this extraction gives
    kf.mvpMapPoints.assign(kf.N, nullptr);
    if (k < B) {
      kf.mvuRight.assign(uright.begin() + (size_t)k * NF, uright.begin() + (size_t)k * NF + kf.N);
      std::copy(poses.begin() + (size_t)k * 16, poses.begin() + (size_t)(k + 1) * 16, kf.Tcw.m.begin());
    }
  }
  for (int o = 0; o < n_obs; o++) {   // point, keyframe, index, whether the keyframe lists the point there
    MapPoint* p = &all[ob[(size_t)o * 4]];
    KeyFrame* kf = &kfs[ob[(size_t)o * 4 + 1]];
    p->AddObservation(kf, ob[(size_t)o * 4 + 2]);
    if (ob[(size_t)o * 4 + 3]) kf->mvpMapPoints[ob[(size_t)o * 4 + 2]] = p;
  }
  Points list(n_pts, nullptr), replace(n_pts, nullptr);
  for (int i = 0; i < n_pts; i++)
    if (exists[i]) list[i] = &all[i];

  ORBmatcher matcher;
  std::vector<int> nFused;
  const int n_targets = mode ? 1 : B;
  if (mode) {
    Matrix4d S;
    std::copy(scw.begin(), scw.end(), S.v);
    nFused.assign(1, matcher.Fuse(batch, &kfs[0], S, list, th[0], replace));
  } else {
    std::vector<KeyFrame*> targets;
    for (int k = 0; k < B; k++) targets.push_back(&kfs[k]);
    matcher.Fuse(batch, targets, list, th[0], nFused);
  }

  FILE* o = std::fopen(argv[2], "wb");
  if (!o) return 5;
  std::vector<int32_t> out(nFused.begin(), nFused.end());
  for (int i = 0; i < n_pts; i++) out.push_back(replace[i] ? replace[i]->id : -1);
  for (int k = 0; k < n_targets; k++) {
    out.push_back(kfs[k].N);
    for (MapPoint* p : kfs[k].mvpMapPoints) out.push_back(p ? p->id : -1);
  }
  for (MapPoint& p : all) {
    std::vector<std::pair<int, int> > so;
    for (auto& ob2 : p.obs) so.push_back(std::make_pair(ob2.first->id, (int)ob2.second));
    std::sort(so.begin(), so.end());
    out.push_back(p.bad ? 1 : 0);
    out.push_back(p.replaced ? p.replaced->id : -1);
    out.push_back((int32_t)so.size());
    for (auto& s : so) {
      out.push_back(s.first);
      out.push_back(s.second);
    }
  }
  wr(o, out);
  std::fclose(o);
  std::printf("facade fuse ran mode %d on %d keyframes\n", mode, n_targets);
  return 0;
}
