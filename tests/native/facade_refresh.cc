// ORBmatcher::RefreshMapPoints of include/sdslam/sdslam.hpp on toy MapPoint / KeyFrame classes.
// Without RUN_ON_GPU (tests/test_refresh_cpu.py, built with AddressSanitizer + UBSan, links nothing): the host part -- the walk
// over the observation maps that builds the CSR lists (BuildObservationLists) and the walk that applies the results
// (ApplyRefreshed) -- against lists and results typed in below.
// With RUN_ON_GPU (tests/test_refresh_facade.py, linked against the library): the whole method on two small extractions, against
// a straight C++ restatement of src/MapPoint.cc:225-343 over the same observation order (compiled with -ffp-contract=off).
#include "mock_map.h"   // CHECK and the UpdateNormalAndDepth restatement; the classes are this file's (they record the descriptor too)

struct KeyFrame {
  int id = 0;
  bool bad = false;
  double Ow[3] = {0, 0, 0};
  std::vector<sd_keypoint> keys;
  std::vector<uint8_t> desc;
  bool isBad() const { return bad; }
};
struct ById {
  bool operator()(const KeyFrame* a, const KeyFrame* b) const { return a->id < b->id; }
};
struct MapPoint {
  bool bad = false;
  double X[3] = {0, 0, 0};
  std::map<KeyFrame*, size_t, ById> obs;   // (the reference keys by pointer; by id here, so that the order is the test's)
  KeyFrame* ref = nullptr;
  uint8_t desc[32] = {};
  double normal[3] = {0, 0, 0};
  float max_dist = -1, min_dist = -1;
  int set_desc = 0, set_normal = 0, set_max = 0, set_min = 0;
  bool isBad() const { return bad; }
  const std::map<KeyFrame*, size_t, ById>& GetObservations() const { return obs; }
  KeyFrame* GetReferenceKeyFrame() const { return ref; }
  void SetDescriptor(const uint8_t* d) { std::memcpy(desc, d, 32); set_desc++; }
  void SetNormalVector(const double* n) { std::memcpy(normal, n, 24); set_normal++; }
  void SetMaxDistance(float v) { max_dist = v; set_max++; }
  void SetMinDistance(float v) { min_dist = v; set_min++; }
};

static void host_part() {
  std::vector<KeyFrame> kfs(6);
  for (int i = 0; i < 6; i++) kfs[i].id = i;
  kfs[3].bad = true;
  KeyFrame* cur = &kfs[5];
  // keyframes 0..2 are frames 0..2 of the ref extractor, 3 is frame 7, 4 is not resident
  auto frameOf = [&](KeyFrame* k) { return k->id <= 2 ? k->id : (k->id == 3 ? 7 : -1); };
  std::vector<MapPoint> pts(7);
  pts[0].obs = {{&kfs[2], 20}, {&kfs[0], 10}, {cur, 50}};   pts[0].ref = &kfs[2];   // iteration order: 0, 2, 5
  pts[1].obs = {{&kfs[3], 33}, {&kfs[1], 11}};              pts[1].ref = &kfs[3];   // a bad keyframe, which is the reference too
  pts[2].bad = true;                                        pts[2].obs = {{&kfs[0], 1}};   pts[2].ref = &kfs[0];
  pts[3].ref = &kfs[0];                                                              // no observations
  pts[4].obs = {{&kfs[4], 44}, {&kfs[0], 4}};               pts[4].ref = &kfs[0];   // a keyframe that is not resident
  pts[5].obs = {{&kfs[1], 5}};                              pts[5].ref = &kfs[2];   // the reference keyframe does not observe it
  pts[6].obs = {{cur, 6}};                                  pts[6].ref = cur;
  std::vector<MapPoint*> vp;
  for (MapPoint& p : pts) vp.push_back(&p);
  vp.insert(vp.begin() + 3, nullptr);   // a hole in the list: indices 0 1 2 - 3 4 5 6
  SD_SLAM::ORBmatcher::ObservationLists L;
  SD_SLAM::ORBmatcher::BuildObservationLists(cur, vp, frameOf, L);
  const std::vector<int32_t> off = {0, 3, 5, 5, 5, 5, 7, 8, 9}, frame = {0, 2, -1, 1, 7, 0, -2, -2, -1}, kp = {10, 20, 50, 11, 33, 4, 44, 5, 6};
  const std::vector<int32_t> ref_obs = {1, 1, 0, 0, 0, 0, 0, 0};
  const std::vector<uint8_t> kf_bad = {0, 0, 0, 0, 1, 0, 0, 0, 0}, point_bad = {0, 0, 1, 1, 0, 0, 0, 0}, left = {0, 0, 0, 0, 0, 0, 1, 0};
  CHECK(L.off == off && L.frame == frame && L.kp == kp, "lists");
  CHECK(L.ref_obs == ref_obs && L.kf_bad == kf_bad && L.point_bad == point_bad && L.left == left, "flags");

  SD_SLAM::ORBmatcher::RefreshedRows r(vp.size());
  for (size_t i = 0; i < vp.size(); i++) {
    std::memset(&r.desc[i * 32], (int)(i + 1), 32);
    for (int k = 0; k < 3; k++) r.normal[i * 3 + k] = (double)i + 0.25 * k;
    r.max_dist[i] = 10.f + (float)i;
    r.min_dist[i] = 1.f + (float)i;
  }
  r.status = {SD_REFRESH_DESC | SD_REFRESH_NORMAL, SD_REFRESH_NORMAL, SD_REFRESH_SKIPPED, SD_REFRESH_SKIPPED, SD_REFRESH_SKIPPED,
              SD_REFRESH_NOT_RESIDENT, SD_REFRESH_NOT_RESIDENT, SD_REFRESH_TOO_MANY};
  const std::vector<MapPoint*> back = SD_SLAM::ORBmatcher::ApplyRefreshed(L, r, vp);
  CHECK(back.size() == 3 && back[0] == &pts[4] && back[1] == &pts[5] && back[2] == &pts[6], "the points left to the caller");
  CHECK(pts[0].set_desc == 1 && pts[0].set_normal == 1 && pts[0].set_max == 1 && pts[0].set_min == 1 && pts[0].desc[31] == 1 &&
            pts[0].normal[2] == 0.5 && pts[0].max_dist == 10.f && pts[0].min_dist == 1.f, "point 0");
  CHECK(pts[1].set_desc == 0 && pts[1].set_normal == 1 && pts[1].normal[1] == 1.25 && pts[1].max_dist == 11.f, "all keyframes bad: no descriptor");
  for (int i = 2; i < 7; i++) CHECK(pts[i].set_desc + pts[i].set_normal + pts[i].set_max + pts[i].set_min == 0, "point %d was touched", i);
  r.status[0] = SD_REFRESH_BAD_INDEX;
  bool threw = false;
  try {
    SD_SLAM::ORBmatcher::ApplyRefreshed(L, r, vp);
  } catch (const SD_SLAM::Error&) {
    threw = true;
  }
  CHECK(threw, "a bad keypoint index is an error");
  // an empty list, and a list of holes
  std::vector<MapPoint*> none, holes(3, nullptr);
  SD_SLAM::ORBmatcher::BuildObservationLists(cur, none, frameOf, L);
  CHECK(L.off.size() == 1 && L.frame.size() == 1 && L.ref_obs.empty(), "empty list");
  SD_SLAM::ORBmatcher::BuildObservationLists(cur, holes, frameOf, L);
  CHECK(L.off == std::vector<int32_t>(4, 0) && L.point_bad == std::vector<uint8_t>(3, 1), "holes");
}

#ifdef RUN_ON_GPU
static int popcount256(const uint8_t* a, const uint8_t* b) {
  int d = 0;
  for (int i = 0; i < 32; i++) d += __builtin_popcount((unsigned)(a[i] ^ b[i]));
  return d;
}
static void check(int rc, const char* what) { CHECK(rc == SD_OK, "%s: %s", what, sd_last_error()); }

// src/MapPoint.cc:225-343 on the toy classes, over GetObservations() in iteration order
static void reference_refresh(MapPoint& p, const float* sf, int nlevels, MapPoint& out) {
  out = p;
  if (p.bad || p.obs.empty()) return;
  std::vector<const uint8_t*> v;
  for (const auto& ob : p.obs)
    if (!ob.first->isBad()) v.push_back(&ob.first->desc[ob.second * 32]);
  if (!v.empty()) {
    const size_t N = v.size();
    int best_median = 1 << 30;
    size_t best = 0;
    for (size_t i = 0; i < N; i++) {
      std::vector<int> d(N);
      for (size_t j = 0; j < N; j++) d[j] = popcount256(v[i], v[j]);
      std::sort(d.begin(), d.end());
      const int median = d[(size_t)(0.5 * (N - 1))];
      if (median < best_median) best_median = median, best = i;
    }
    std::memcpy(out.desc, v[best], 32);
  }
  const NormalAndDepth nd = update_normal_and_depth(p, p.X, sf, nlevels, [](const KeyFrame* k, double* Ow) { std::memcpy(Ow, k->Ow, 24); });
  std::memcpy(out.normal, nd.normal, 24);
  out.max_dist = nd.max_dist;
  out.min_dist = nd.min_dist;
}

static void gpu_part() {
  const int W = 320, H = 240, B = 3, NL = 8, M = 64;
  std::vector<uint8_t> img((size_t)B * W * H);
  uint32_t s = 12345;
  for (int f = 0; f < B; f++)   // blocks of random brightness: corners everywhere
    for (int y = 0; y < H; y++)
      for (int x = 0; x < W; x++) {
        const uint32_t cell = (uint32_t)(f * 7919 + (y / 6) * 131 + (x / 6));
        s = cell * 2654435761u;
        img[((size_t)f * H + y) * W + x] = (uint8_t)(s >> 24);
      }
  SD_SLAM::ORBextractor cur_x(300, 1.2f, NL, 20, W, H, B), ref_x(300, 1.2f, NL, 20, W, H, B);
  sd_orb *cur = cur_x.handle(), *ref = ref_x.handle();
  const int cap = 400;
  std::vector<KeyFrame> kfs(B + 2);   // 0..2: frames of ref; 3: the current keyframe (frame 0 of cur); 4: not resident
  std::vector<sd_keypoint> kps((size_t)B * cap);
  std::vector<uint8_t> desc((size_t)B * cap * 32);
  int n_out[B];
  check(sd_orb_extract_batch(ref, img.data(), B, W, H, W, (size_t)W * H, kps.data(), desc.data(), cap, n_out), "extract ref");
  for (int f = 0; f < B; f++) {
    CHECK(n_out[f] >= 40, "frame %d: %d keypoints", f, n_out[f]);
    kfs[f].keys.assign(kps.begin() + (size_t)f * cap, kps.begin() + (size_t)f * cap + n_out[f]);
    kfs[f].desc.assign(desc.begin() + (size_t)f * cap * 32, desc.begin() + ((size_t)f * cap + n_out[f]) * 32);
  }
  check(sd_orb_extract_batch(cur, img.data() + (size_t)W * H, 1, W, H, W, (size_t)W * H, kps.data(), desc.data(), cap, n_out), "extract cur");
  kfs[3].keys.assign(kps.begin(), kps.begin() + n_out[0]);
  kfs[3].desc.assign(desc.begin(), desc.begin() + (size_t)n_out[0] * 32);
  kfs[4].keys.assign(1, sd_keypoint{0, 0, 0, 0, 0, 0, -1});
  kfs[4].desc.assign(32, 0);
  for (int i = 0; i < B + 2; i++) kfs[i].id = i;
  kfs[1].bad = true;
  // poses: small rotations about y and translations; Ow = -R^T t in the library's operation order
  std::vector<double> Tref((size_t)B * 16, 0.0), Tcur((size_t)B * 16, 0.0);
  auto pose = [](double* T, double a, double tx, double ty, double tz, double* Ow) {
    const double c = std::cos(a), sn = std::sin(a);
    const double R[3][3] = {{c, 0, sn}, {0, 1, 0}, {-sn, 0, c}}, t[3] = {tx, ty, tz};
    for (int r = 0; r < 3; r++) {
      for (int cc = 0; cc < 3; cc++) T[cc * 4 + r] = R[r][cc];
      T[12 + r] = t[r];
    }
    T[15] = 1;
    for (int r = 0; r < 3; r++) Ow[r] = -((T[r * 4] * t[0] + T[r * 4 + 1] * t[1]) + T[r * 4 + 2] * t[2]);
  };
  for (int f = 0; f < B; f++) pose(&Tref[(size_t)f * 16], 0.1 * f, 0.3 * f, -0.1 * f, 0.05 * f, kfs[f].Ow);
  for (int f = 0; f < B; f++) pose(&Tcur[(size_t)f * 16], -0.07, 0.11, 0.2, -0.3, kfs[3].Ow);
  SD_SLAM::TrackBatch batch(cur_x, ref_x, M, B, 8);
  sd_track* trk = batch.handle();
  check(sd_track_set_camera(trk, 300, 300, 160, 120, 0, 0, (float)W, 0, (float)H), "set_camera");
  check(sd_track_set_poses(trk, 0, B, Tref.data(), Tcur.data()), "set_poses");
  // the points: every one sees a few keyframes; one has a keyframe that is not resident, one is bad, one has none
  const int n_pts = 20;
  std::vector<MapPoint> pts(n_pts);
  for (int i = 0; i < n_pts; i++) {
    MapPoint& p = pts[i];
    p.X[0] = -1.0 + 0.1 * i; p.X[1] = 0.3 - 0.05 * i; p.X[2] = 4.0 + 0.2 * i;
    for (int k = 0; k < B + 1; k++)
      if ((i + k) % 4 != 3) p.obs[&kfs[k]] = (size_t)((i * 3 + k * 5) % 40);
    p.ref = p.obs.begin()->first;
    if (i % 3 == 1) p.ref = p.obs.rbegin()->first;
    std::memset(p.desc, 0xEE, 32);
  }
  pts[4].obs[&kfs[4]] = 0;
  pts[7].bad = true;
  pts[9].obs.clear();
  std::vector<MapPoint*> vp;
  for (MapPoint& p : pts) vp.push_back(&p);
  // the row as a Fuse call would have uploaded it
  std::vector<int32_t> n_local(1, n_pts), obs(M, 0);
  std::vector<uint8_t> cand(M, 1), d0(M * 32, 0xEE);
  std::vector<double> Xw(M * 3, 0.0), nrm(M * 3, -7.0);
  std::vector<float> dmin(M, -1.f), dmax(M, -2.f), mfmax(M, -3.f);
  for (int i = 0; i < n_pts; i++) std::memcpy(&Xw[i * 3], pts[i].X, 24);
  check(sd_track_set_local(trk, 0, 1, n_local.data(), cand.data(), Xw.data(), nrm.data(), dmin.data(), dmax.data(), mfmax.data(), d0.data(),
                           obs.data(), nullptr), "set_local");
  float sf[NL];
  sf[0] = 1.f;
  for (int l = 1; l < NL; l++) sf[l] = sf[l - 1] * 1.2f;
  std::vector<MapPoint> want(n_pts);
  for (int i = 0; i < n_pts; i++) reference_refresh(pts[i], sf, NL, want[i]);
  SD_SLAM::ORBmatcher matcher(0.6f, false);
  auto frameOf = [&](KeyFrame* k) { return k->id < B ? k->id : -1; };
  const std::vector<MapPoint*> back = matcher.RefreshMapPoints(batch, &kfs[3], vp, frameOf, 0);
  CHECK(back.size() == 1 && back[0] == &pts[4], "%zu points left to the caller", back.size());
  int with_desc = 0;
  for (int i = 0; i < n_pts; i++) {
    const MapPoint &g = pts[i], &w = (i == 4 ? pts[i] : want[i]);
    CHECK(std::memcmp(g.desc, w.desc, 32) == 0, "descriptor of point %d", i);
    CHECK(std::memcmp(g.normal, w.normal, 24) == 0 && std::memcmp(&g.max_dist, &w.max_dist, 4) == 0 &&
              std::memcmp(&g.min_dist, &w.min_dist, 4) == 0, "normal / depth of point %d: %.17g %.17g | %.9g %.9g", i, g.normal[0], w.normal[0],
          g.max_dist, w.max_dist);
    with_desc += g.set_desc;
  }
  CHECK(with_desc >= 15, "%d descriptors set", with_desc);
  // the row holds the refreshed fields: read it back
  std::vector<uint8_t> rd((size_t)M * 32);
  std::vector<float> rmax(M), rmf(M);
  check(sd_track_debug_read(trk, 3, 0, rd.data(), rd.size()), "debug_read desc");
  check(sd_track_debug_read(trk, 6, 0, rmax.data(), (size_t)M * 4), "debug_read max");
  check(sd_track_debug_read(trk, 7, 0, rmf.data(), (size_t)M * 4), "debug_read mfmax");
  for (int i = 0; i < n_pts; i++) {
    const bool written = i != 4 && i != 7 && i != 9;
    CHECK(std::memcmp(&rd[(size_t)i * 32], pts[i].desc, 32) == 0, "row descriptor %d", i);
    CHECK(written ? (rmf[i] == pts[i].max_dist && rmax[i] == 1.2f * pts[i].max_dist) : (rmf[i] == -3.f && rmax[i] == -2.f), "row distances %d", i);
  }
}
#endif

int main() {
  host_part();
#ifdef RUN_ON_GPU
  gpu_part();
#endif
  std::printf("facade_refresh OK\n");
  return 0;
}
