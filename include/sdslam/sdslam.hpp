// sdslam.hpp -- header-only C++ facade over the C ABI (sdslam_hip.h) that re-exposes the
// reference's class and method names for the tracking hot path, over POD types that are
// layout-compatible with what the reference's callers hold:
//   SD_SLAM::KeyPoint   == cv::KeyPoint (28 bytes)
//   descriptors         == N x 32 uint8 row-major (cv::Mat CV_8U)
//   poses               == 16 doubles column-major (Eigen::Matrix4d::data())
// A reference translation unit (Frame.cc / Tracking.cc style) keeps its call sites; see
// INTEGRATION.md for the type-alias header that maps cv::Mat / Eigen arguments onto these.
//
//   ORBextractor   reference src/ORBextractor.h:38-70
//   ORBmatcher     reference src/ORBmatcher.h:40-65  (DescriptorDistance, SearchByProjection(Frame,Frame), SearchByPoints,
//                                                      SearchForTriangulation, Fuse)
//   ImageAlign     reference src/ImageAlign.h:32-44  (ComputePose, GetError)
//   PnPsolver      reference src/PnPsolver.h:67-76   (SetRansacParameters, iterate)
// ImageAlign / ORBmatcher / PnPsolver operate on a TrackBatch (frames resident on the GPU).
#pragma once
#include <cstdint>
#include <cstring>
#include <stdexcept>
#include <string>
#include <utility>
#include <vector>

#include "../sdslam_hip.h"

namespace SD_SLAM {

typedef sd_keypoint KeyPoint;
static_assert(sizeof(KeyPoint) == 28, "cv::KeyPoint layout");

struct Error : std::runtime_error {
  int code;
  Error(int c, const std::string& m) : std::runtime_error(m), code(c) {}
};
inline void check(int rc) {
  if (rc != SD_OK) throw Error(rc, sd_last_error());
}

// Image pyramid level as handed back by ORBextractor::operator() (host copy on demand).
struct Mat8 {
  int cols = 0, rows = 0;
  std::vector<uint8_t> data;
  const uint8_t* ptr(int y) const { return data.data() + (size_t)y * cols; }
};

class ORBextractor {
 public:
  enum { HARRIS_SCORE = 0, FAST_SCORE = 1 };

  ORBextractor(int nfeatures, float scaleFactor, int nlevels, int thFAST, int max_w = 1280, int max_h = 960, int max_batch = 1,
               int device = 0)
      : nlevels_(nlevels), scaleFactor_(scaleFactor), cap_(nfeatures) {
    check(sd_orb_create(nfeatures, scaleFactor, nlevels, thFAST, max_w, max_h, max_batch, device, &h_));
  }
  ~ORBextractor() { sd_orb_destroy(h_); }
  ORBextractor(const ORBextractor&) = delete;
  ORBextractor& operator=(const ORBextractor&) = delete;

  // operator()(image, mask, keypoints, descriptors, imagePyramid); mask is ignored like in the
  // reference.  `image` is an 8-bit single-channel buffer (cv::Mat::data / step).
  void operator()(const uint8_t* image, int cols, int rows, int step, std::vector<KeyPoint>& keypoints,
                  std::vector<uint8_t>& descriptors, std::vector<Mat8>* imagePyramid = nullptr) {
    keypoints.resize(cap_);
    descriptors.resize((size_t)cap_ * 32);
    int n = 0;
    check(sd_orb_extract(h_, image, cols, rows, step, keypoints.data(), descriptors.data(), cap_, &n));
    keypoints.resize(n);
    descriptors.resize((size_t)n * 32);
    if (imagePyramid && cols > 0 && rows > 0) {
      imagePyramid->resize(nlevels_);
      for (int l = 0; l < nlevels_; l++) {
        Mat8& m = (*imagePyramid)[l];
        check(sd_orb_level_info(h_, l, &m.cols, &m.rows));
        m.data.resize((size_t)m.cols * m.rows);
        check(sd_orb_level_copy(h_, 0, l, 0, m.data.data(), m.cols));
      }
    }
  }

  int GetLevels() { return nlevels_; }
  float GetScaleFactor() { return scaleFactor_; }
  std::vector<float> GetScaleFactors() { return table(0); }
  std::vector<float> GetInverseScaleFactors() { return table(1); }
  std::vector<float> GetScaleSigmaSquares() { return table(2); }
  std::vector<float> GetInverseScaleSigmaSquares() { return table(3); }

  // Frame::UndistortKeyPoints (src/Frame.cc:335-366): K as Converter::toCvMat(K) (CV_32F), DistCoef {k1,k2,p1,p2,k3}.
  // After this, matching / PnP read mvKeysUn; UndistortedKeyPoints() returns them for the frames of the last call.
  void SetDistortion(float fx, float fy, float cx, float cy, float k1, float k2 = 0, float p1 = 0, float p2 = 0, float k3 = 0) {
    check(sd_orb_set_distortion(h_, fx, fy, cx, cy, k1, k2, p1, p2, k3));
  }
  void UndistortedKeyPoints(int frame, std::vector<KeyPoint>& mvKeysUn, int n) {
    std::vector<KeyPoint> all(cap_);
    check(sd_orb_download_undistorted(h_, frame, 1, all.data(), cap_));
    mvKeysUn.assign(all.begin(), all.begin() + (n < cap_ ? n : cap_));
  }

  sd_orb* handle() { return h_; }

 private:
  std::vector<float> table(int which) {
    std::vector<float> t[4];
    for (auto& v : t) v.resize(nlevels_);
    check(sd_orb_scale_tables(h_, t[0].data(), t[1].data(), t[2].data(), t[3].data()));
    return t[which];
  }
  sd_orb* h_ = nullptr;
  int nlevels_;
  float scaleFactor_;
  int cap_;
};

// Flattened view of what TrackWithMotionModel reads from LastFrame (src/Tracking.cc:654-718):
// one entry per last-frame keypoint.
struct LastFrameView {
  std::vector<uint8_t> valid;    // mvpMapPoints[i] != NULL && !mvbOutlier[i]
  std::vector<double> Xw;        // 3 per entry: pMP->GetWorldPos()
  std::vector<uint8_t> desc;     // 32 per entry: pMP->GetDescriptor()
  std::vector<int32_t> octave;   // mvKeys[i].octave
  std::vector<float> angle;      // mvKeysUn[i].angle
  std::vector<int32_t> obs;      // pMP->Observations()
  int size() const { return (int)valid.size(); }
};

// One batch of (current frame, last frame) pairs resident on the GPU.
class TrackBatch {
 public:
  TrackBatch(ORBextractor& cur, ORBextractor& ref, int max_points, int max_batch, int pnp_max_iterations = 300)
      : max_points_(max_points), cur_(&cur), ref_(&ref) {
    check(sd_track_create(cur.handle(), ref.handle(), max_points, max_batch, pnp_max_iterations, &h_));
  }
  ~TrackBatch() { sd_track_destroy(h_); }
  TrackBatch(const TrackBatch&) = delete;
  TrackBatch& operator=(const TrackBatch&) = delete;

  // Frame statics (src/Frame.cc:158-174)
  void SetCamera(float fx, float fy, float cx, float cy, float bf, float minX, float maxX, float minY, float maxY) {
    check(sd_track_set_camera(h_, fx, fy, cx, cy, bf, minX, maxX, minY, maxY));
  }
  void SetLastFrame(int frame, const LastFrameView& v) {
    LastFrameView p = v;   // pad to capacity
    const int n = v.size();
    p.valid.resize(max_points_); p.Xw.resize((size_t)max_points_ * 3); p.desc.resize((size_t)max_points_ * 32);
    p.octave.resize(max_points_); p.angle.resize(max_points_); p.obs.resize(max_points_);
    check(sd_track_set_last(h_, frame, 1, &n, p.valid.data(), p.Xw.data(), p.desc.data(), p.octave.data(), p.angle.data(),
                            p.obs.data()));
  }
  // LastFrame.GetPose(), CurrentFrame.GetPose() (prior); 16 doubles column-major each
  void SetPoses(int frame, const double* Tlast, const double* Tcur_prior) { check(sd_track_set_poses(h_, frame, 1, Tlast, Tcur_prior)); }
  // one current frame (frame `cur_frame` of the cur extractor) against the keyframes held in the batch slots; -1 = off
  void SetCurrentBroadcast(int cur_frame) { check(sd_track_set_current_broadcast(h_, cur_frame)); }
  // Frame::ComputeStereoFromRGBD (src/Frame.cc:399-417) on the current frames: depth = CV_32F images, one per frame
  void ComputeStereoFromRGBD(int n_frames, const float* imDepth, int cols, int rows, int step_elems, size_t frame_step_elems) {
    check(sd_track_stereo_from_depth(h_, n_frames, imDepth, cols, rows, step_elems, frame_step_elems));
  }
  // the same on depth maps already in device memory (dtype SD_DEPTH_F32 / SD_DEPTH_U16), converted as Tracking::GrabImageRGBD
  // does with depthMapFactor = Config::DepthMapFactor(); queued without a host wait (ordering: sdslam_hip.h)
  void ComputeStereoFromRGBD(int n_frames, const void* d_imDepth, int dtype, int cols, int rows, int step_elems, size_t frame_step_elems,
                             float depthMapFactor) {
    check(sd_track_stereo_from_depth_device(h_, n_frames, d_imDepth, dtype, cols, rows, step_elems, frame_step_elems, depthMapFactor));
  }
  // TrackLocalMap: local map points of one frame (src/Tracking.cc:898-939), flattened in mvpLocalMapPoints order
  struct LocalMapView {
    std::vector<uint8_t> cand;                 // reaches isInFrustum: !isBad() && mnLastFrameSeen != frame id
    std::vector<double> Xw, normal;            // GetWorldPos(), GetNormal()  (3 per point)
    std::vector<float> min_dist, max_dist;     // GetMinDistanceInvariance(), GetMaxDistanceInvariance()
    std::vector<float> mf_max_dist;            // mfMaxDistance (MapPoint::PredictScale)
    std::vector<uint8_t> desc;                 // GetDescriptor(), 32 per point
    std::vector<int32_t> obs;                  // Observations()
  };
  void SetLocalMap(int frame, const LocalMapView& v, const uint8_t* kp_claimed /* kp_cap flags or nullptr */) {
    LocalMapView p = v;
    const int n = (int)v.cand.size();
    p.cand.resize(max_points_); p.Xw.resize((size_t)max_points_ * 3); p.normal.resize((size_t)max_points_ * 3);
    p.min_dist.resize(max_points_); p.max_dist.resize(max_points_); p.mf_max_dist.resize(max_points_);
    p.desc.resize((size_t)max_points_ * 32); p.obs.resize(max_points_);
    check(sd_track_set_local(h_, frame, 1, &n, p.cand.data(), p.Xw.data(), p.normal.data(), p.min_dist.data(), p.max_dist.data(),
                             p.mf_max_dist.data(), p.desc.data(), p.obs.data(), kp_claimed));
  }
  // stereo frames: mvuRight computed by the caller (-1 = no match)
  void SetURight(int frame, const float* mvuRight, int n) { check(sd_track_set_uright(h_, frame, 1, mvuRight, n)); }

  // Sequential tracking: mLastFrame = Frame(mCurrentFrame) on the device (src/Tracking.cc:250-292).  Per frame:
  //   CurrentExtractor() extracts -> SetPrior | PredictMotion -> Tracking::TrackWithMotionModel -> Tracking::TrackLocalMap ->
  //   [UpdateMotion] -> AdvanceLastFrame.
  // ids: the caller's MapPoint identities (which 0: the last frame's points, 1: the local map's; -1 = none).  With both set,
  // TrackLocalMap skips the local points TrackWithMotionModel saw (mnLastFrameSeen, :703, :900-918).
  void SetMapIds(int frame, int which, const int32_t* ids, int n) { check(sd_track_set_map_ids(h_, frame, 1, which, ids, n)); }
  // source 1: after TrackLocalMap; 0: after TrackWithMotionModel; 2: after StereoInitialization.  The extractors swap roles afterwards.
  void AdvanceLastFrame(int n_frames, int source = 1) { check(sd_track_advance(h_, n_frames, source)); }
  // CurrentFrame pose prior, 16 doubles column-major per frame: T (relative = false) or T * LastFrame.GetPose()
  // (ConstantVelocity::GetPose, relative = true)
  void SetPrior(int frame0, int n_frames, const double* T_cm, bool relative) {
    check(sd_track_set_prior(h_, frame0, n_frames, T_cm, relative ? 1 : 0));
  }
  // The motion model on the device (EKF + ConstantVelocity per slot, src/sensors/EKF.cc, ConstantVelocity.cc), all queued:
  // PredictMotion = motion_model_->Predict(mLastFrame.GetPose()) (src/Tracking.cc:661) as the prior of slots < n_frames, dt the
  // time since the last update (the reference's timer_); UpdateMotion = :243-247 with the Restart() of :221 / :226 for the
  // slots the call named by source (0 TrackWithMotionModel, 1 TrackLocalMap, -1 every slot) did not track, before
  // AdvanceLastFrame; RestartMotion = motion_model_->Restart().  A slot that is not started gets the last pose as prior;
  // running TrackReferenceKeyFrame or Relocalization on such slots stays with the caller.  Which Sensor the three run is
  // SetSensorModel's choice, as Tracking chooses at construction (src/Tracking.cc:134-138): SD_SENSOR_CONSTANT_VELOCITY (the
  // default) or SD_SENSOR_IMU, the 16-state filter of System::MONOCULAR_IMU (src/sensors/IMU.cc), whose prior is the filter's
  // own absolute pose and whose UpdateMotion reads the measurements of SetMeasurements.
  void PredictMotion(int n_frames, double dt) { check(sd_track_motion_predict(h_, n_frames, dt)); }
  void UpdateMotion(int n_frames, int source = 1) { check(sd_track_motion_update(h_, n_frames, source)); }
  void RestartMotion(int frame0, int n_frames) { check(sd_track_motion_restart(h_, frame0, n_frames)); }
  // the filter of slot `frame`: X (v, w), the diagonal of P, it_time and Exp(X) of the last prediction (16 doubles
  // column-major); any pointer may be null.  Returns EKF::Started().  Synchronises.
  bool MotionState(int frame, double X[6], double Pdiag[6] = nullptr, double* it_time = nullptr, double E_cm[16] = nullptr) {
    int32_t started = 0;
    check(sd_track_get_motion(h_, frame, 1, X, Pdiag, &started, it_time, E_cm, nullptr));
    return started != 0;
  }
  // the Sensor of the motion model; every slot's filter of the chosen model restarts
  void SetSensorModel(int model) { check(sd_track_set_sensor_model(h_, model)); }
  // Tracking::SetMeasurements for slots frame0 .. frame0 + n - 1: [n][6] doubles (gyro xyz, accelerometer xyz), queued; they
  // persist until replaced.  SD_SENSOR_IMU only.
  void SetMeasurements(int frame0, int n, const double* wa6) { check(sd_track_set_measurements(h_, frame0, n, wa6)); }
  // the IMU filter of slot `frame`: X (x, q as w x y z, v, w, a), the dense P row-major, gravity_ and it_time; any pointer
  // may be null.  Returns EKF::Started().  Synchronises.
  bool ImuState(int frame, double X[16], double P[256] = nullptr, double gravity[3] = nullptr, double* it_time = nullptr) {
    int32_t started = 0;
    check(sd_track_get_imu(h_, frame, 1, X, P, gravity, &started, it_time, nullptr, nullptr));
    return started != 0;
  }
  // the last frame of slot `frame` (what AdvanceLastFrame or SetLastFrame left); ids may be null
  void GetLastFrame(int frame, LastFrameView& v, std::vector<int32_t>* ids = nullptr) {
    const size_t M = max_points_;
    int32_t n = 0;
    v.valid.resize(M); v.Xw.resize(M * 3); v.desc.resize(M * 32); v.octave.resize(M); v.angle.resize(M); v.obs.resize(M);
    if (ids) ids->resize(M);
    check(sd_track_get_last(h_, frame, 1, &n, v.valid.data(), v.Xw.data(), v.desc.data(), v.octave.data(), v.angle.data(), v.obs.data(),
                            ids ? ids->data() : nullptr));
    v.valid.resize(n); v.Xw.resize((size_t)n * 3); v.desc.resize((size_t)n * 32); v.octave.resize(n); v.angle.resize(n); v.obs.resize(n);
    if (ids) ids->resize(n);
  }
  // Tracking::NeedNewKeyFrame's RGB-D counts (src/Tracking.cc:776-789), queued: keypoints with 0 < mvDepth < thDepth (mThDepth)
  // whose map point AdvanceLastFrame(n_frames, source) would keep, and the others; CloseTrackedPointsResult reads them
  void CloseTrackedPoints(int n_frames, int source, float thDepth) { check(sd_track_close_points(h_, n_frames, source, thDepth)); }
  void CloseTrackedPointsResult(int frame, int& nTrackedClose, int& nNonTrackedClose) {
    int32_t out2[2];
    check(sd_track_get_close_points(h_, frame, 1, out2));
    nTrackedClose = out2[0];
    nNonTrackedClose = out2[1];
  }
  // RGB-D map points on the device (src/Tracking.cc:302-349, :753-896).  Frame 0: extract, ComputeStereoFromRGBD,
  // StereoInitialization, AdvanceLastFrame(n, 2).  Later frames: ... Tracking::TrackLocalMap -> CloseTrackedPoints(n, 1, thDepth)
  // -> Tracking::NeedNewKeyFrame -> Tracking::CreateNewKeyFrame(use_flags) -> AdvanceLastFrame(n, 1).
  // Tracking::StereoInitialization (:302-349), queued: slots with more than min_keypoints keypoints get the identity pose and
  // one map point per keypoint with depth, ids from SetNextMapPointId in keypoint order
  void StereoInitialization(int n_frames, int min_keypoints = 500) { check(sd_track_stereo_init(h_, n_frames, min_keypoints)); }
  // MapPoint::nNextId of the slots' maps
  void SetNextMapPointId(int frame0, int n_frames, const int32_t* next_id) { check(sd_track_set_next_map_id(h_, frame0, n_frames, next_id)); }
  // NeedNewKeyFrame's caller state, 8 ints per slot {KeyFramesInMap(), mpReferenceKF->TrackedMapPoints(nMinObs), mnLastKeyFrameId,
  // mnLastRelocFrameId, flags (1 AcceptKeyFrames(), 2 isStopped() || stopRequested(), 4 KeyframesInQueue() < 3, 8 usePattern), 0, 0,
  // 0}; SD_KF_KEEP leaves an entry as the device has it
  void SetKeyFrameState(int frame0, int n_frames, const int32_t* state8) { check(sd_track_set_keyframe_state(h_, frame0, n_frames, state8)); }
  // the decision bytes: bit 0 insert a keyframe, bit 1 wanted but the mapper is busy (call InterruptBA)
  void SetKeyFrameFlags(int frame0, int n_frames, const uint8_t* flags) { check(sd_track_set_keyframe_flags(h_, frame0, n_frames, flags)); }
  uint8_t KeyFrameFlags(int frame) {
    uint8_t f = 0;
    check(sd_track_get_keyframe_flags(h_, frame, 1, &f));
    return f;
  }
  // the map points the last StereoInitialization / Tracking::CreateNewKeyFrame made in slot `frame`, in creation order (what
  // the caller mirrors into its Map; KeyFrame construction and InsertKeyFrame stay with it).  Synchronises.
  struct CreatedMapPoints {
    int mode = 0;                   // 0 nothing created on the slot, 1 keyframe, 2 initialisation
    int processed = 0, candidates = 0;
    std::vector<int32_t> keypoint;  // index into the frame's keypoints
    std::vector<int32_t> id;
    std::vector<double> Xw;         // 3 per point
  };
  CreatedMapPoints CreatedPoints(int frame) {
    const int cap = 2048;           // the tracker's keypoint limit
    CreatedMapPoints c;
    int32_t i4[4];
    c.keypoint.resize(cap); c.id.resize(cap); c.Xw.resize((size_t)cap * 3);
    check(sd_track_get_created(h_, frame, 1, i4, c.keypoint.data(), c.Xw.data(), c.id.data(), cap));
    c.mode = i4[0]; c.processed = i4[2]; c.candidates = i4[3];
    c.keypoint.resize(i4[1]); c.id.resize(i4[1]); c.Xw.resize((size_t)i4[1] * 3);
    return c;
  }
  // the extractor whose frames are tracked next (the two swap roles at every AdvanceLastFrame)
  ORBextractor& CurrentExtractor() {
    sd_orb* c = nullptr;
    check(sd_track_get_extractors(h_, &c, nullptr));
    return c == cur_->handle() ? *cur_ : *ref_;
  }
  sd_track* handle() { return h_; }
  int max_points() const { return max_points_; }

 private:
  sd_track* h_ = nullptr;
  int max_points_;
  ORBextractor* cur_;
  ORBextractor* ref_;
};

class ImageAlign {
 public:
  ImageAlign() {}
  // bool ComputePose(Frame &CurrentFrame, const Frame &LastFrame) for every pair of the batch;
  // per-frame results through Result().
  void ComputePose(TrackBatch& batch, int n_frames, bool keyframe = false, bool fast = false) {
    check(sd_track_align(batch.handle(), n_frames, keyframe ? (fast ? 2 : 1) : 0));
  }
  void ComputePoseKF(TrackBatch& batch, int n_frames) { check(sd_track_align(batch.handle(), n_frames, 3)); }
  // returns the bool of ComputePose; Tcw = pose set by CurrentFrame.SetPose; error = GetError()
  bool Result(TrackBatch& batch, int frame, double Tcw[16], double* error = nullptr) {
    int32_t ok = 0;
    check(sd_track_get_align(batch.handle(), frame, 1, Tcw, error, &ok, nullptr, nullptr));
    return ok != 0;
  }
};

class ORBmatcher {
 public:
  static const int TH_LOW = 50, TH_HIGH = 100, HISTO_LENGTH = 30;
  ORBmatcher(float nnratio = 0.6f, bool checkOri = true) : mfNNratio(nnratio), mbCheckOrientation(checkOri) {}
  static int DescriptorDistance(const uint8_t* a, const uint8_t* b) { return sd_hamming(a, b); }
  // int SearchByProjection(Frame &CurrentFrame, const Frame &LastFrame, const float th, const bool bMono)
  void SearchByProjection(TrackBatch& batch, int n_frames, float th, bool bMono) {
    check(sd_track_match(batch.handle(), n_frames, th, bMono ? 1 : 0, mbCheckOrientation ? 1 : 0));
  }
  // CurrentFrame.mvpMapPoints as indices into LastFrame (-1 = NULL); returns nmatches
  // SearchByProjection(Frame&, const vector<MapPoint*>&, th): isInFrustum (viewing cosine limit 0.5) + the local-map search
  void SearchLocalPoints(TrackBatch& batch, int n_frames, float th) {
    check(sd_track_match_local(batch.handle(), n_frames, th, mfNNratio, 0.5f));
  }
  int LocalResult(TrackBatch& batch, int frame, std::vector<int32_t>& local_match, int kp_cap) {
    local_match.resize(kp_cap);
    int32_t n = 0;
    check(sd_track_get_local(batch.handle(), frame, 1, local_match.data(), kp_cap, &n, nullptr, nullptr, nullptr, nullptr));
    return n;
  }
  // int SearchByPoints(KeyFrame* currentKF, KeyFrame* pKF, vector<MapPoint*>& matches) (src/ORBmatcher.h:56, brute-force
  // Hamming; LoopClosing::ComputeSim3): has_mp_* = GetMapPointMatches()[i] != NULL && !isBad(), n flags per keyframe
  void SearchByPoints(TrackBatch& batch, int n_frames, const uint8_t* has_mp_cur, const uint8_t* has_mp_ref, int n) {
    check(sd_track_set_point_flags(batch.handle(), 0, n_frames, has_mp_cur, has_mp_ref, n));
    check(sd_track_search_by_points(batch.handle(), n_frames, mfNNratio, mbCheckOrientation ? 1 : 0));
  }
  int PointsResult(TrackBatch& batch, int frame, std::vector<int32_t>& matches12, int kp_cap) {
    matches12.resize(kp_cap);
    int32_t n = 0;
    check(sd_track_get_point_matches(batch.handle(), frame, 1, matches12.data(), kp_cap, &n));
    return n;
  }
  int Result(TrackBatch& batch, int frame, std::vector<int32_t>& mvpMapPoints, int kp_cap) {
    mvpMapPoints.resize(kp_cap);
    int32_t n = 0;
    check(sd_track_get_matches(batch.handle(), frame, 1, mvpMapPoints.data(), kp_cap, &n));
    return n;
  }
  // int SearchForTriangulation(KeyFrame* pKF1, KeyFrame* pKF2, const Eigen::Matrix3d& F12, vector<pair<size_t, size_t>>&)
  //                                            src/ORBmatcher.h:65, src/ORBmatcher.cc:359-475, LocalMapping::CreateNewMapPoints
  // Frame 0 of the batch's cur extractor holds pKF1's image, frame 0 of its ref extractor pKF2's.  KeyFrameT needs N,
  // GetMapPointMatches(), mvuRight and GetPose(); F12 is anything indexable as F12(r, c).  kp_cap: the keypoint capacity.
  template <class KeyFrameT, class Matrix3T>
  int SearchForTriangulation(TrackBatch& batch, KeyFrameT* pKF1, KeyFrameT* pKF2, const Matrix3T& F12,
                             std::vector<std::pair<size_t, size_t> >& vMatchedPairs, int kp_cap) {
    UploadTriangulationSlot(batch, 0, pKF1, pKF2, kp_cap);
    double F[9];
    for (int r = 0; r < 3; r++)
      for (int c = 0; c < 3; c++) F[r * 3 + c] = F12(r, c);
    check(sd_track_set_f12(batch.handle(), 0, 1, F));
    check(sd_track_search_for_triangulation(batch.handle(), 1, 1, mbCheckOrientation ? 1 : 0));
    return TriangulationResult(batch, 0, vMatchedPairs, kp_cap);
  }
  // The loop of CreateNewMapPoints over the neighbours in one call: pKF1 (frame 0 of the cur extractor, broadcast) against
  // vpNeighKFs[i] (frame i of the ref extractor), F12 = LocalMapping::ComputeF12 on the device.  vMatchedPairs[i] is what the
  // reference returns for neighbour i on pKF1's map points as they are NOW; with orientation checking off, dropping the pairs
  // whose idx1 an earlier neighbour turned into a point gives the reference's sequential result (sdslam_hip.h).
  template <class KeyFrameT>
  void SearchForTriangulation(TrackBatch& batch, KeyFrameT* pKF1, const std::vector<KeyFrameT*>& vpNeighKFs,
                              std::vector<std::vector<std::pair<size_t, size_t> > >& vMatchedPairs, int kp_cap) {
    const int n = (int)vpNeighKFs.size();
    vMatchedPairs.assign(n, {});
    if (n == 0) return;
    for (int i = 0; i < n; i++) UploadTriangulationSlot(batch, i, pKF1, vpNeighKFs[i], kp_cap);
    batch.SetCurrentBroadcast(0);
    const int rc = sd_track_search_for_triangulation(batch.handle(), n, 0, mbCheckOrientation ? 1 : 0);
    if (rc == SD_OK)
      for (int i = 0; i < n; i++) TriangulationResult(batch, i, vMatchedPairs[i], kp_cap);
    batch.SetCurrentBroadcast(-1);
    check(rc);
  }
  // The rows of sd_track_get_new_points, in (neighbour, idx1) order
  struct NewPointRows {
    std::vector<int32_t> kp1, slot, idx2, id;
    std::vector<double> Xw, normal;        // [n][3]
    std::vector<float> max_dist, min_dist;
    std::vector<uint8_t> desc;             // [n][32]
    size_t size() const { return kp1.size(); }
  };
  // void LocalMapping::CreateNewMapPoints()                                                  src/LocalMapping.cc:187-420
  // pKF1 = mpCurrentKeyFrame (frame 0 of the cur extractor, broadcast), vpNeighKFs = GetBestCovisibilityKeyFrames(nn) (frame i
  // of the ref extractor).  The device searches every neighbour, triangulates every match with the reference's tests and
  // numbers the new points in the reference's creation order (sd_track_triangulate); the caller's objects are made here, in
  // that order (WalkNewPoints).  nNextId = MapPoint::nNextId; make_point(Xw[3], pKF1, id) is `new MapPoint(x3D, pKF1, mpMap)`
  // (+ mpMap->AddMapPoint, which stays the caller's); recent = mlpRecentAddedMapPoints.  Returns nnew.  The matcher must have
  // been made with checkOri = false, as the reference's `ORBmatcher matcher(0.6, false)` is.  CheckNewKeyFrames' early return
  // between neighbours is not taken: all neighbours are done in one call.
  // KeyFrameT needs, besides what SearchForTriangulation needs, mvDepth, ComputeSceneMedianDepth(q) and AddMapPoint(pMP, idx);
  // MapPointT needs AddObservation(pKF, idx), SetDescriptor(const uint8_t*), SetNormalVector(const double*),
  // SetMaxDistance(float) and SetMinDistance(float): what ComputeDistinctiveDescriptors and UpdateNormalAndDepth would compute
  // (for two observations; RefreshMapPoints below runs both functions for any list).
  template <class KeyFrameT, class MakePoint, class RecentList>
  int CreateNewMapPoints(TrackBatch& batch, KeyFrameT* pKF1, const std::vector<KeyFrameT*>& vpNeighKFs, bool monocular, int32_t nNextId,
                         MakePoint make_point, RecentList& recent, int kp_cap) {
    const int n = (int)vpNeighKFs.size();
    if (n == 0) return 0;
    UploadNewPointSlots(batch, pKF1, vpNeighKFs, monocular, nNextId, kp_cap);
    batch.SetCurrentBroadcast(0);
    int rc = sd_track_search_for_triangulation(batch.handle(), n, 0, 0);
    if (rc == SD_OK) rc = sd_track_triangulate(batch.handle(), n, monocular ? 1 : 0);
    NewPointRows rows;
    if (rc == SD_OK) rc = DownloadNewPoints(batch, rows);
    batch.SetCurrentBroadcast(-1);
    check(rc);
    return WalkNewPoints(rows, pKF1, vpNeighKFs, make_point, recent);
  }
  // The same with the new points appended to local row point_row ON THE DEVICE (sd_track_append_new_points, mark_flags = 1), behind
  // the points the row holds: the row is then what the first loop of SearchInNeighbors hands to Fuse (sd_track_fuse with this
  // point_row), with cand of rows < n_cand_rows = the Fuse targets, the neighbours in the first ref frames.  Only kp1, slot, idx2
  // and id of every point come back; position, normal, distances and descriptor stay on the device (sd_track_get_local_points
  // reads them when the caller wants them, RefreshMapPoints rewrites them).  make_point(pKF1, id, pos) makes the caller's object of
  // the point at position pos of the row; the objects are made in creation order and vnRowPos[i] is the position of the i-th --
  // what Fuse's walk indexes best_idx with.  Points that did not fit into the row were dropped on the device (neither appended nor
  // flagged): no object is made for them.  Returns nnew = the number appended.
  template <class KeyFrameT, class MakePoint, class RecentList>
  int CreateNewMapPoints(TrackBatch& batch, KeyFrameT* pKF1, const std::vector<KeyFrameT*>& vpNeighKFs, bool monocular, int32_t nNextId,
                         MakePoint make_point, RecentList& recent, int kp_cap, int point_row, int n_cand_rows,
                         std::vector<int32_t>& vnRowPos) {
    vnRowPos.clear();
    const int n = (int)vpNeighKFs.size();
    if (n == 0) return 0;
    UploadNewPointSlots(batch, pKF1, vpNeighKFs, monocular, nNextId, kp_cap);
    batch.SetCurrentBroadcast(0);
    int rc = sd_track_search_for_triangulation(batch.handle(), n, 0, 0);
    if (rc == SD_OK) rc = sd_track_triangulate(batch.handle(), n, monocular ? 1 : 0);
    if (rc == SD_OK) rc = sd_track_append_new_points(batch.handle(), point_row, n_cand_rows, 1);
    NewPointRows rows;
    int32_t base = 0, appended = 0;
    if (rc == SD_OK) rc = DownloadNewPointIndices(batch, rows);
    if (rc == SD_OK) rc = sd_track_get_appended(batch.handle(), point_row, 1, &base, &appended, nullptr);
    batch.SetCurrentBroadcast(-1);
    check(rc);
    return WalkAppendedPoints(rows, base, appended, pKF1, vpNeighKFs, make_point, recent, vnRowPos);
  }
  // What both overloads upload: mvDepth of both sides, every slot's flags, mvuRight and poses, the median depths, nNextId
  template <class KeyFrameT>
  void UploadNewPointSlots(TrackBatch& batch, KeyFrameT* pKF1, const std::vector<KeyFrameT*>& vpNeighKFs, bool monocular, int32_t nNextId,
                           int kp_cap) {
    const int n = (int)vpNeighKFs.size();
    std::vector<float> z(kp_cap, -1.f), median(n, -1.f);
    for (int i = 0; i < pKF1->N && i < kp_cap; i++) z[i] = pKF1->mvDepth[i];
    check(sd_track_set_tri_depth(batch.handle(), 0, 0, 1, z.data(), kp_cap));
    for (int k = 0; k < n; k++) {
      KeyFrameT* pKF2 = vpNeighKFs[k];
      UploadTriangulationSlot(batch, k, pKF1, pKF2, kp_cap);
      std::fill(z.begin(), z.end(), -1.f);
      for (int i = 0; i < pKF2->N && i < kp_cap; i++) z[i] = pKF2->mvDepth[i];
      check(sd_track_set_tri_depth(batch.handle(), 1, k, 1, z.data(), kp_cap));
      if (monocular) median[k] = pKF2->ComputeSceneMedianDepth(2);
    }
    check(sd_track_set_tri_median_depth(batch.handle(), 0, n, median.data()));
    check(sd_track_set_next_map_id(batch.handle(), 0, 1, &nNextId));
  }
  // kp1, slot, idx2 and id of sd_track_get_new_points, nothing else: the other arrays of `r` stay empty
  int DownloadNewPointIndices(TrackBatch& batch, NewPointRows& r) {
    int32_t info[4] = {0, 0, 0, 0};
    int rc = sd_track_get_new_points(batch.handle(), info, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0);
    if (rc != SD_OK) return rc;
    const size_t n = (size_t)info[0];
    r.kp1.resize(n); r.slot.resize(n); r.idx2.resize(n); r.id.resize(n);
    if (n == 0) return SD_OK;
    return sd_track_get_new_points(batch.handle(), info, r.kp1.data(), r.slot.data(), r.idx2.data(), r.id.data(), nullptr, nullptr, nullptr,
                                   nullptr, nullptr, (int)n);
  }
  // :401-417 for the first `appended` rows, in order, without the fields: the point at row position base + p, its two observations,
  // both keyframes' AddMapPoint, mlpRecentAddedMapPoints.  Host code only.
  template <class KeyFrameT, class MakePoint, class RecentList>
  static int WalkAppendedPoints(const NewPointRows& r, int32_t base, int32_t appended, KeyFrameT* pKF1,
                                const std::vector<KeyFrameT*>& vpNeighKFs, MakePoint make_point, RecentList& recent,
                                std::vector<int32_t>& vnRowPos) {
    int nnew = 0;
    for (size_t p = 0; p < r.size() && p < (size_t)(appended > 0 ? appended : 0); p++) {
      KeyFrameT* pKF2 = vpNeighKFs[(size_t)r.slot[p]];
      auto* pMP = make_point(pKF1, r.id[p], base + (int32_t)p);
      pMP->AddObservation(pKF1, (size_t)r.kp1[p]);
      pMP->AddObservation(pKF2, (size_t)r.idx2[p]);
      pKF1->AddMapPoint(pMP, (size_t)r.kp1[p]);
      pKF2->AddMapPoint(pMP, (size_t)r.idx2[p]);
      recent.push_back(pMP);
      vnRowPos.push_back(base + (int32_t)p);
      nnew++;
    }
    return nnew;
  }
  int DownloadNewPoints(TrackBatch& batch, NewPointRows& r) {
    int32_t info[4] = {0, 0, 0, 0};
    int rc = sd_track_get_new_points(batch.handle(), info, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, 0);
    if (rc != SD_OK) return rc;
    const size_t n = (size_t)info[0];
    r.kp1.resize(n); r.slot.resize(n); r.idx2.resize(n); r.id.resize(n);
    r.Xw.resize(n * 3); r.normal.resize(n * 3); r.max_dist.resize(n); r.min_dist.resize(n); r.desc.resize(n * 32);
    if (n == 0) return SD_OK;
    return sd_track_get_new_points(batch.handle(), info, r.kp1.data(), r.slot.data(), r.idx2.data(), r.id.data(), r.Xw.data(),
                                   r.normal.data(), r.max_dist.data(), r.min_dist.data(), r.desc.data(), (int)n);
  }
  // :401-417 for every row, in order: the point, its two observations, both keyframes' AddMapPoint, descriptor, normal and
  // distances from the device's fields, mlpRecentAddedMapPoints.  Host code only.
  template <class KeyFrameT, class MakePoint, class RecentList>
  static int WalkNewPoints(const NewPointRows& r, KeyFrameT* pKF1, const std::vector<KeyFrameT*>& vpNeighKFs, MakePoint make_point,
                           RecentList& recent) {
    int nnew = 0;
    for (size_t p = 0; p < r.size(); p++) {
      KeyFrameT* pKF2 = vpNeighKFs[(size_t)r.slot[p]];
      auto* pMP = make_point(&r.Xw[p * 3], pKF1, r.id[p]);
      pMP->AddObservation(pKF1, (size_t)r.kp1[p]);
      pMP->AddObservation(pKF2, (size_t)r.idx2[p]);
      pKF1->AddMapPoint(pMP, (size_t)r.kp1[p]);
      pKF2->AddMapPoint(pMP, (size_t)r.idx2[p]);
      pMP->SetDescriptor(&r.desc[p * 32]);
      pMP->SetNormalVector(&r.normal[p * 3]);
      pMP->SetMaxDistance(r.max_dist[p]);
      pMP->SetMinDistance(r.min_dist[p]);
      recent.push_back(pMP);
      nnew++;
    }
    return nnew;
  }
  int TriangulationResult(TrackBatch& batch, int frame, std::vector<std::pair<size_t, size_t> >& vMatchedPairs, int kp_cap) {
    std::vector<int32_t> m12(kp_cap);
    int32_t n = 0;
    check(sd_track_get_triangulation_matches(batch.handle(), frame, 1, m12.data(), kp_cap, &n, nullptr, nullptr));
    vMatchedPairs.clear();
    vMatchedPairs.reserve(n);
    for (int i = 0; i < kp_cap; i++)
      if (m12[i] >= 0) vMatchedPairs.push_back(std::make_pair((size_t)i, (size_t)m12[i]));
    return n;
  }
  // Slot `slot` of a SearchForTriangulation call: "holds a map point" flags (bad points count, :385-403), mvuRight and poses.
  // pKF1's mvuRight goes to row 0 of the cur extractor's frames, the row every slot reads under the broadcast.
  template <class KeyFrameT>
  void UploadTriangulationSlot(TrackBatch& batch, int slot, KeyFrameT* pKF1, KeyFrameT* pKF2, int kp_cap) {
    const auto vpMapPoints1 = pKF1->GetMapPointMatches();
    const auto vpMapPoints2 = pKF2->GetMapPointMatches();
    std::vector<uint8_t> has1(kp_cap, 0), has2(kp_cap, 0);
    std::vector<float> ur1(kp_cap, -1.f), ur2(kp_cap, -1.f);
    for (int i = 0; i < pKF1->N && i < kp_cap; i++) {
      has1[i] = vpMapPoints1[i] != nullptr;
      ur1[i] = pKF1->mvuRight[i];
    }
    for (int i = 0; i < pKF2->N && i < kp_cap; i++) {
      has2[i] = vpMapPoints2[i] != nullptr;
      ur2[i] = pKF2->mvuRight[i];
    }
    check(sd_track_set_point_flags(batch.handle(), slot, 1, has1.data(), has2.data(), kp_cap));
    if (slot == 0) check(sd_track_set_uright(batch.handle(), 0, 1, ur1.data(), kp_cap));
    check(sd_track_set_uright_ref(batch.handle(), slot, 1, ur2.data(), kp_cap));
    const auto T1 = pKF1->GetPose();
    const auto T2 = pKF2->GetPose();
    batch.SetPoses(slot, T2.data(), T1.data());
  }

  // int Fuse(KeyFrame* pKF, const vector<MapPoint*>& vpMapPoints, const float th = 3.0)     src/ORBmatcher.cc:477-615
  // Frame i of the batch's ref extractor holds vpTargetKFs[i]'s image (i = 0 for the single-keyframe overloads).  The device
  // searches (sd_track_fuse), the caller's objects are fused here.  KeyFrameT needs N, mvuRight, GetPose(), GetMapPoint(idx),
  // AddMapPoint(pMP, idx) (and GetMapPoints() for the Sim3 overload); MapPointT needs isBad(), IsInKeyFrame(pKF), Observations(),
  // Replace(pMP), AddObservation(pKF, idx), GetWorldPos() / GetNormal() indexable as v(i), GetMinDistanceInvariance(),
  // GetMaxDistanceInvariance(), GetMaxDistance() (= mfMaxDistance, which PredictScale reads) and GetDescriptor() -> 32 bytes.
  template <class KeyFrameT, class MapPointT>
  int Fuse(TrackBatch& batch, KeyFrameT* pKF, const std::vector<MapPointT*>& vpMapPoints, float th = 3.0f) {
    std::vector<int> nFused;
    Fuse(batch, std::vector<KeyFrameT*>(1, pKF), vpMapPoints, th, nFused);
    return nFused[0];
  }
  // The first loop of LocalMapping::SearchInNeighbors (src/LocalMapping.cc:456-461) in one device call: vpMapPoints against every
  // target keyframe (shared point row, kf_side 1), then the keyframes in order and, inside each, the points in order.
  template <class KeyFrameT, class MapPointT>
  void Fuse(TrackBatch& batch, const std::vector<KeyFrameT*>& vpTargetKFs, const std::vector<MapPointT*>& vpMapPoints, float th,
            std::vector<int>& nFused) {
    const int n = (int)vpTargetKFs.size(), M = batch.max_points();
    nFused.assign(n, 0);
    if (n == 0) return;
    for (int k = 0; k < n; k++) {
      KeyFrameT* pKF = vpTargetKFs[k];
      UploadFusePoints(batch, k, vpMapPoints, k == 0, [&](MapPointT* pMP) { return pMP->IsInKeyFrame(pKF); });
      UploadFuseKeyFrame(batch, k, pKF);
    }
    check(sd_track_fuse(batch.handle(), n, 1, 0, th, 0));
    std::vector<int32_t> best((size_t)n * M);
    check(sd_track_get_fuse(batch.handle(), 0, n, best.data(), nullptr, M, nullptr));
    // Equal to the sequential loop: best_idx depends on nothing the walk changes, and for a point that is not bad isBad() and
    // IsInKeyFrame() only ever go from false to true during the walk, so the uploaded cand is a superset of the live test.
    for (int k = 0; k < n; k++) {
      KeyFrameT* pKF = vpTargetKFs[k];
      for (size_t i = 0; i < vpMapPoints.size() && i < (size_t)M; i++) {
        MapPointT* pMP = vpMapPoints[i];
        if (!pMP || pMP->isBad() || pMP->IsInKeyFrame(pKF)) continue;
        const int bestIdx = best[(size_t)k * M + i];
        if (bestIdx < 0) continue;
        MapPointT* pMPinKF = pKF->GetMapPoint(bestIdx);   // :597-611
        if (pMPinKF) {
          if (!pMPinKF->isBad()) {
            if (pMPinKF->Observations() > pMP->Observations()) pMP->Replace(pMPinKF);
            else pMPinKF->Replace(pMP);
          }
        } else {
          pMP->AddObservation(pKF, bestIdx);
          pKF->AddMapPoint(pMP, bestIdx);
        }
        nFused[k]++;
      }
    }
  }
  // int Fuse(KeyFrame* pKF, const Eigen::Matrix4d& Scw, const vector<MapPoint*>& vpPoints, float th, vector<MapPoint*>& vpReplacePoint)
  //                                                                     src/ORBmatcher.cc:617-732, LoopClosing::SearchAndFuse
  // Scw is anything indexable as Scw(r, c); vpReplacePoint has vpPoints.size() entries, as in the reference.
  template <class KeyFrameT, class Matrix4T, class MapPointT>
  int Fuse(TrackBatch& batch, KeyFrameT* pKF, const Matrix4T& Scw, const std::vector<MapPointT*>& vpPoints, float th,
           std::vector<MapPointT*>& vpReplacePoint) {
    const int M = batch.max_points();
    const auto spAlreadyFound = pKF->GetMapPoints();
    UploadFusePoints(batch, 0, vpPoints, true, [&](MapPointT* pMP) { return spAlreadyFound.count(pMP) != 0; });
    UploadFuseKeyFrame(batch, 0, pKF);
    double S[16];
    for (int r = 0; r < 4; r++)
      for (int c = 0; c < 4; c++) S[c * 4 + r] = Scw(r, c);
    check(sd_track_set_fuse_scw(batch.handle(), 0, 1, S));
    check(sd_track_fuse(batch.handle(), 1, 1, -1, th, 1));
    std::vector<int32_t> best(M);
    check(sd_track_get_fuse(batch.handle(), 0, 1, best.data(), nullptr, M, nullptr));
    int nFused = 0;
    for (size_t i = 0; i < vpPoints.size() && i < (size_t)M; i++) {   // :718-728; nothing here makes a point bad or adds to the set
      MapPointT* pMP = vpPoints[i];
      if (!pMP || pMP->isBad() || spAlreadyFound.count(pMP) || best[i] < 0) continue;
      MapPointT* pMPinKF = pKF->GetMapPoint(best[i]);
      if (pMPinKF) {
        if (!pMPinKF->isBad()) vpReplacePoint[i] = pMPinKF;
      } else {
        pMP->AddObservation(pKF, best[i]);
        pKF->AddMapPoint(pMP, best[i]);
      }
      nFused++;
    }
    return nFused;
  }
  // Point row `slot` of a Fuse call: cand = pMP && !isBad() && !in_kf(pMP); the other fields only where `full` (the shared row).
  template <class MapPointT, class InKF>
  void UploadFusePoints(TrackBatch& batch, int slot, const std::vector<MapPointT*>& pts, bool full, InKF in_kf) {
    const size_t M = batch.max_points();
    if (pts.size() > M) throw Error(SD_ERR_CAPACITY, "Fuse: more points than the batch's max_points (split the list)");
    const int32_t n = (int32_t)pts.size();
    std::vector<uint8_t> cand(M, 0), desc(M * 32, 0);
    std::vector<double> Xw(M * 3, 0.0), normal(M * 3, 0.0);
    std::vector<float> dmin(M, 0.f), dmax(M, 0.f), mfmax(M, 0.f);
    std::vector<int32_t> obs(M, 0);
    for (size_t i = 0; i < pts.size(); i++) {
      MapPointT* p = pts[i];
      if (!p) continue;
      cand[i] = !p->isBad() && !in_kf(p);
      if (!full) continue;
      const auto X = p->GetWorldPos();
      const auto Nn = p->GetNormal();
      for (int k = 0; k < 3; k++) {
        Xw[i * 3 + k] = X(k);
        normal[i * 3 + k] = Nn(k);
      }
      dmin[i] = p->GetMinDistanceInvariance();
      dmax[i] = p->GetMaxDistanceInvariance();
      mfmax[i] = p->GetMaxDistance();
      std::memcpy(&desc[i * 32], p->GetDescriptor(), 32);
    }
    check(sd_track_set_local(batch.handle(), slot, 1, &n, cand.data(), Xw.data(), normal.data(), dmin.data(), dmax.data(), mfmax.data(),
                             desc.data(), obs.data(), nullptr));
  }
  // Keyframe of slot `slot` (frame `slot` of the ref extractor): mvuRight and the pose, as Tref
  template <class KeyFrameT>
  void UploadFuseKeyFrame(TrackBatch& batch, int slot, KeyFrameT* pKF) {
    if (pKF->N > 0) check(sd_track_set_uright_ref(batch.handle(), slot, 1, pKF->mvuRight.data(), pKF->N));
    const auto T = pKF->GetPose();
    batch.SetPoses(slot, T.data(), T.data());
  }

  // pMP->ComputeDistinctiveDescriptors(); pMP->UpdateNormalAndDepth(); for every point of a list
  //                                   src/MapPoint.cc:225-343; callers src/LocalMapping.cc:478-488, :140-147, src/LoopClosing.cc:457-484
  // The loop that ends SearchInNeighbors, on the device (sd_track_refresh_points, write_local = 1).  vpMapPoints are the points of
  // local row `point_row` as the last Fuse call (or sd_track_set_local) uploaded them, entry i = vpMapPoints[i]; pKF is the current
  // keyframe (the broadcast frame of the cur extractor, or its frame 0; pose Tcur of slot 0); frameOf(KeyFrameT*) returns the
  // frame of the ref extractor that holds a keyframe's image (its pose is Tref of that slot), or a negative number when the
  // keyframe is not resident.  Each point's GetObservations() is walked in ITS iteration order, which defines the tie-break of
  // the descriptor and the order of the normal's sum.  Points the device refreshed get SetDescriptor / SetNormalVector /
  // SetMaxDistance / SetMinDistance (the parts their status names) and the row holds the same values: the next Fuse or
  // TrackLocalMap search needs no upload.  Returns the points left to the caller's own two calls: those with a keyframe that is
  // not resident, with more than SD_REFRESH_MAX_OBS observations, or whose reference keyframe is not among the observations.
  // KeyFrameT needs isBad(); MapPointT needs isBad(), GetObservations() (pairs of KeyFrameT* and keypoint index),
  // GetReferenceKeyFrame() and the four setters.
  template <class KeyFrameT, class MapPointT, class FrameOf>
  std::vector<MapPointT*> RefreshMapPoints(TrackBatch& batch, KeyFrameT* pKF, const std::vector<MapPointT*>& vpMapPoints, FrameOf frameOf,
                                           int point_row = 0) {
    if (vpMapPoints.size() > (size_t)batch.max_points())
      throw Error(SD_ERR_CAPACITY, "RefreshMapPoints: more points than the batch's max_points (split the list)");
    ObservationLists L;
    BuildObservationLists(pKF, vpMapPoints, frameOf, L);
    const int n = (int)vpMapPoints.size();
    if (n == 0) return {};
    SetObservations(batch.handle(), n, L);
    check(sd_track_refresh_points(batch.handle(), point_row, 1));
    RefreshedRows r(n);
    check(sd_track_get_refreshed(batch.handle(), r.status.data(), nullptr, nullptr, r.desc.data(), r.normal.data(), r.max_dist.data(),
                                 r.min_dist.data(), n));
    return ApplyRefreshed(L, r, vpMapPoints);   // (the lists and the results, not the batch: host code, tests/native/facade_refresh.cc)
  }
  // The CSR lists of sd_track_set_observations.  left[i]: the point goes back to the caller whatever the device says.
  struct ObservationLists {
    std::vector<int32_t> off, frame, kp, ref_obs;
    std::vector<uint8_t> kf_bad, point_bad, left;
  };
  struct RefreshedRows {
    std::vector<uint8_t> status, desc;
    std::vector<double> normal;
    std::vector<float> max_dist, min_dist;
    explicit RefreshedRows(size_t n) : status(n, 0), desc(n * 32, 0), normal(n * 3, 0.0), max_dist(n, 0.f), min_dist(n, 0.f) {}
  };
  // Host code only: every point's GetObservations() in ITS iteration order into the CSR lists; the one walk behind the refresh and
  // both bundle adjustments.  pKF (may be null) is frame -1, a keyframe frameOf() does not know -2.  ask_bad: a NULL or bad point is
  // sent as a bad one, without its observations; otherwise every point is taken as it stands (it must not be NULL).  left[i]: the
  // reference keyframe is not among the observations (the reference would read observations[pRefKF] of a keyframe that is not
  // there).  edge(i, pKFi, keypoint index) is called for every entry, in order.
  template <class KeyFrameT, class MapPointT, class FrameOf, class Edge>
  static void WalkObservations(KeyFrameT* pKF, const std::vector<MapPointT*>& vpMapPoints, bool ask_bad, FrameOf frameOf, ObservationLists& L,
                               Edge edge) {
    const size_t n = vpMapPoints.size();
    L.off.assign(1, 0);
    L.frame.clear(); L.kp.clear(); L.kf_bad.clear();
    L.ref_obs.assign(n, 0);
    L.point_bad.assign(n, 0);
    L.left.assign(n, 0);
    for (size_t i = 0; i < n; i++) {
      MapPointT* pMP = vpMapPoints[i];
      if (ask_bad && (!pMP || pMP->isBad())) {
        L.point_bad[i] = 1;
        L.off.push_back((int32_t)L.frame.size());
        continue;
      }
      const auto& observations = pMP->GetObservations();
      const KeyFrameT* pRefKF = pMP->GetReferenceKeyFrame();
      int32_t pos = 0, ref_pos = -1;
      for (const auto& ob : observations) {
        KeyFrameT* pKFi = ob.first;
        const int f = pKFi == pKF ? -1 : (int)frameOf(pKFi);
        L.frame.push_back(pKFi == pKF ? -1 : (f < 0 ? -2 : f));
        L.kp.push_back((int32_t)ob.second);
        L.kf_bad.push_back(pKFi->isBad() ? 1 : 0);
        edge(i, pKFi, ob.second);
        if (pKFi == pRefKF) ref_pos = pos;
        pos++;
      }
      if (pos > 0 && ref_pos < 0) L.left[i] = 1;
      L.ref_obs[i] = ref_pos < 0 ? 0 : ref_pos;
      L.off.push_back((int32_t)L.frame.size());
    }
    // (data() of an empty vector may be NULL: no entry is sent as one entry of zeros; SetObservations sees to the lists per point)
    if (L.frame.empty()) L.frame.push_back(0), L.kp.push_back(0), L.kf_bad.push_back(0);
  }
  // Host code only: the lists of RefreshMapPoints.  A NULL point is sent as a bad one (both functions skip it).
  template <class KeyFrameT, class MapPointT, class FrameOf>
  static void BuildObservationLists(KeyFrameT* pKF, const std::vector<MapPointT*>& vpMapPoints, FrameOf frameOf, ObservationLists& L) {
    WalkObservations(pKF, vpMapPoints, true, frameOf, L, [](size_t, KeyFrameT*, size_t) {});
    for (size_t i = 0; i < vpMapPoints.size(); i++)
      if (L.left[i]) L.frame[(size_t)L.off[i]] = -2;   // the device leaves the point, and its row, alone
  }
  // Host code only: the setters for what the status names; returns the points that stay with the caller
  template <class MapPointT>
  static std::vector<MapPointT*> ApplyRefreshed(const ObservationLists& L, const RefreshedRows& r, const std::vector<MapPointT*>& vpMapPoints) {
    std::vector<MapPointT*> left;
    for (size_t i = 0; i < vpMapPoints.size(); i++) {
      MapPointT* pMP = vpMapPoints[i];
      if (!pMP || L.point_bad[i]) continue;
      const int st = r.status[i];
      if (L.left[i] || (st & (SD_REFRESH_NOT_RESIDENT | SD_REFRESH_TOO_MANY))) {
        left.push_back(pMP);
        continue;
      }
      if (st & SD_REFRESH_BAD_INDEX) throw Error(SD_ERR_INVALID_ARG, "RefreshMapPoints: an observation's keypoint index is outside its keyframe");
      if (st & SD_REFRESH_DESC) pMP->SetDescriptor(&r.desc[i * 32]);
      if (st & SD_REFRESH_NORMAL) SetNormalAndDepth(pMP, r, i);
    }
    return left;
  }

 protected:
  friend class Optimizer;   // (the bundle adjustments upload the same lists and apply the same refresh)
  // The one sd_track_set_observations call from the lists; kf_bad: another per-entry flag list than L.kf_bad
  static void SetObservations(sd_track* h, int n, const ObservationLists& L, const std::vector<uint8_t>* kf_bad = nullptr) {
    static const int32_t no_ref = 0;   // n == 0: data() of an empty vector may be NULL
    static const uint8_t not_bad = 0;
    check(sd_track_set_observations(h, n, L.off.data(), L.frame.data(), L.kp.data(), (kf_bad ? *kf_bad : L.kf_bad).data(),
                                    n ? L.ref_obs.data() : &no_ref, n ? L.point_bad.data() : &not_bad));
  }
  // What UpdateNormalAndDepth writes, from row i of the refresh's results
  template <class MapPointT>
  static void SetNormalAndDepth(MapPointT* pMP, const RefreshedRows& r, size_t i) {
    pMP->SetNormalVector(&r.normal[i * 3]);
    pMP->SetMaxDistance(r.max_dist[i]);
    pMP->SetMinDistance(r.min_dist[i]);
  }
  float mfNNratio;
  bool mbCheckOrientation;
};

// Optimizer::PoseOptimization (src/Optimizer.h: static int PoseOptimization(Frame*)), batched.
class Optimizer {
 public:
  // source 0: map points of ORBmatcher::SearchByProjection(batch, ...); 1: of SearchLocalPoints
  static void PoseOptimization(TrackBatch& batch, int n_frames, int source = 0) { check(sd_track_pose_opt(batch.handle(), n_frames, source)); }
  // returns nInitialCorrespondences - nBad; Tcw = 16 doubles column-major; mvbOutlier resized to kp_cap
  static int Result(TrackBatch& batch, int frame, double Tcw[16], std::vector<uint8_t>& mvbOutlier, int kp_cap) {
    mvbOutlier.resize(kp_cap);
    int32_t info[8];
    check(sd_track_get_pose_opt(batch.handle(), frame, 1, Tcw, mvbOutlier.data(), kp_cap, info));
    return info[5];
  }

  // void Optimizer::LocalBundleAdjustment(KeyFrame* pKF, bool* pbStopFlag, Map* pMap)          src/Optimizer.cc:417-714
  // on the device (sd_track_local_ba with write_back = 1).  pKF is the current keyframe (frame 0 of the cur extractor, or the
  // broadcast frame; Tcur of slot 0); frameOf(KeyFrameT*) returns the frame of the ref extractor that holds a keyframe, or a
  // negative number when it is not resident.  The three lists are built as :418-460 builds them (the marks mnBALocalForKF /
  // mnBAFixedForKF are written as there); the points go into local row `point_row` in lLocalMapPoints order, the poses and
  // mvuRight rows of every resident keyframe of the problem into its slot (Tcur of those slots is overwritten with the same
  // pose, as by ORBmatcher::Fuse), roles and observations behind them.  Then, in the reference's order: EraseMapPointMatch /
  // EraseObservation for the erase flags (all mono edges, then all stereo edges, each in edge order), SetPose on every local
  // keyframe, SetWorldPos on every local point, and the refresh that is UpdateNormalAndDepth (SetNormalVector / SetMaxDistance /
  // SetMinDistance; the observations are uploaded again only when something was erased).  *pbStopFlag is read once, where the
  // reference reads it before optimize() (:604); inside the run it is not modelled.  Returns false, with no object touched, when
  // the flag is set or the device refuses the problem (a local point seen by a keyframe that is not resident, more than
  // SD_BA_MAX_FREE_KF local keyframes, a keypoint index outside its frame); the marks and the uploads have happened by then.
  // KeyFrameT needs mnId, mnBALocalForKF, mnBAFixedForKF, N, mvuRight, isBad(), GetVectorCovisibleKeyFrames(),
  // GetMapPointMatches(), GetPose() (16 doubles column-major behind .data()), SetPose(const double*), EraseMapPointMatch(pMP).
  // MapPointT needs what ORBmatcher::Fuse's point upload needs, and mnBALocalForKF, GetObservations(), GetReferenceKeyFrame(),
  // EraseObservation(pKF), SetWorldPos(const double*) and the three setters of the refresh.
  // erase_on_device: when something was erased, sd_track_erase_observations(SD_ERASE_LOCAL_BA) kills the same entries on the
  // resident lists before the refresh, instead of the second walk and upload; the objects' EraseObservation must then cascade as
  // the reference's does (nObs <= 2: SetBadFlag, mpRefKF to the first observation), which is what the device does to the lists.
  template <class KeyFrameT, class FrameOf>
  static bool LocalBundleAdjustment(TrackBatch& batch, KeyFrameT* pKF, bool* pbStopFlag, FrameOf frameOf, int point_row = 0,
                                    bool erase_on_device = false) {
    using MapPointT = typename std::remove_pointer<typename std::decay<decltype(pKF->GetMapPointMatches())>::type::value_type>::type;
    LocalBaLists<KeyFrameT, MapPointT> L;
    BuildLocalBaLists(pKF, frameOf, L);
    if (pbStopFlag && *pbStopFlag) return false;
    if (L.points.size() > (size_t)batch.max_points())
      throw Error(SD_ERR_CAPACITY, "LocalBundleAdjustment: more local points than the batch's max_points");
    sd_track* h = batch.handle();
    ORBmatcher matcher(0.6f, false);
    matcher.UploadFusePoints(batch, point_row, L.points, true, [](MapPointT*) { return false; });
    const auto Tc = pKF->GetPose();
    check(sd_track_set_poses(h, 0, 1, Tc.data(), Tc.data()));
    if (pKF->N > 0) batch.SetURight(0, pKF->mvuRight.data(), pKF->N);
    for (size_t k = 0; k < L.resident.size(); k++)   // (Tcur of slot 0 is the current keyframe's pose, not the resident keyframe's)
      UploadBaKeyFrame(h, L.resident_frame[k], L.resident[k], L.resident_frame[k] == 0 ? Tc.data() : nullptr);
    const int n = (int)L.points.size(), n_ref = (int)L.kf_role.size();
    check(sd_track_set_ba_keyframes(h, n_ref, L.kf_role.data(), L.cur_role));
    ORBmatcher::SetObservations(h, n, L.obs);
    check(sd_track_local_ba(h, point_row, 1));
    LocalBaResult r((size_t)n_ref, (size_t)n, L.edge_kf.size());
    check(sd_track_get_local_ba(h, r.T_ref.data(), r.T_cur, r.Xw.data(), r.point_status.data(), r.obs_erase.data(), r.info, n, (int)L.edge_kf.size()));
    if (r.info[0] != SD_BA_OK) return false;
    const bool erased = ApplyLocalBa(pKF, L, r);
    if (n == 0) return true;
    if (erased && erase_on_device) {
      check(sd_track_erase_observations(h, SD_ERASE_LOCAL_BA));
    } else if (erased) {   // the lists the refresh reads are the points' observations as they are now
      BuildBaObservations(pKF, frameOf, L);
      ORBmatcher::SetObservations(h, n, L.obs);
    }
    check(sd_track_refresh_points(h, point_row, 1));
    ORBmatcher::RefreshedRows rr((size_t)n);
    check(sd_track_get_refreshed(h, rr.status.data(), nullptr, nullptr, nullptr, rr.normal.data(), rr.max_dist.data(), rr.min_dist.data(), n));
    for (size_t i = 0; i < (size_t)n; i++)   // pMP->UpdateNormalAndDepth() (:712); a point whose reference keyframe does not observe it stays as it is
      if ((rr.status[i] & SD_REFRESH_NORMAL) && !L.obs.left[i]) ORBmatcher::SetNormalAndDepth(L.points[i], rr, i);
    return true;
  }
  // A resident keyframe of either bundle adjustment into its slot: the pose (Tcur: what the slot's current-frame pose is given when
  // it is not the keyframe's own), then its mvuRight row.  (ORBmatcher::UploadFuseKeyFrame sends the same two in the other order.)
  template <class KeyFrameT>
  static void UploadBaKeyFrame(sd_track* h, int slot, KeyFrameT* kf, const double* Tcur = nullptr) {
    const auto T = kf->GetPose();
    check(sd_track_set_poses(h, slot, 1, T.data(), Tcur ? Tcur : T.data()));
    if (kf->N > 0) check(sd_track_set_uright_ref(h, slot, 1, kf->mvuRight.data(), kf->N));
  }
  // void Optimizer::BundleAdjustment(vpKFs, vpMP, nIterations, pbStopFlag, nLoopKF, bRobust)          src/Optimizer.cc:53-219
  // on the device (sd_track_global_ba).  Every keyframe is a frame of the ref extractor: frameOf(KeyFrameT*) returns it, or a
  // negative number when the keyframe is not resident (its observations then refuse the call, as in LocalBundleAdjustment); the
  // current-keyframe slot is not used (it is given role 2 and no observation).  Entry i of local row `point_row` is vpMP[i]; a
  // NULL or bad point is sent as a bad one.  Roles: a keyframe of vpKFs that is not bad is 1, with mnId == 0 it is 2; a bad one has
  // none and its observations carry obs_kf_bad; so do the observations of a keyframe with mnId > maxKFid (:109).  An observation
  // of any other keyframe outside vpKFs is the edge to a missing vertex the reference would dereference: SD_BA_NO_VERTEX.
  // *pbStopFlag is read once, before anything is uploaded; inside the run it is not modelled.  With nLoopKF == 0 the run writes
  // back, and then, in the reference's order (:185-217): SetPose on every keyframe of vpKFs that is not bad, and for every point
  // that was included SetWorldPos followed by the refresh's values that are UpdateNormalAndDepth (a point whose reference keyframe
  // does not observe it, or with an observation of a keyframe that is not resident, gets the position only).  Otherwise nothing is written back and mTcwGBA / mnBAGlobalForKF of the
  // keyframes and mPosGBA / mnBAGlobalForKF of the included points are set from the getter (16 and 3 doubles behind .data()).
  // Returns false, with no object touched, when the flag is set or the device refuses the problem.
  // KeyFrameT needs mnId, N, mvuRight, isBad(), GetPose(), SetPose(const double*), mTcwGBA, mnBAGlobalForKF; MapPointT what
  // ORBmatcher::Fuse's point upload needs, GetObservations(), GetReferenceKeyFrame(), SetWorldPos(const double*), the three setters
  // of the refresh, mPosGBA, mnBAGlobalForKF.
  template <class KeyFrameT, class MapPointT, class FrameOf>
  static bool BundleAdjustment(TrackBatch& batch, const std::vector<KeyFrameT*>& vpKFs, const std::vector<MapPointT*>& vpMP, int nIterations,
                               bool* pbStopFlag, const unsigned long nLoopKF, const bool bRobust, FrameOf frameOf, int point_row = 0) {
    if (pbStopFlag && *pbStopFlag) return false;
    if (vpMP.size() > (size_t)batch.max_points()) throw Error(SD_ERR_CAPACITY, "BundleAdjustment: more points than the batch's max_points");
    GlobalBaLists<KeyFrameT> L;
    BuildGlobalBaLists(vpKFs, vpMP, frameOf, L);
    sd_track* h = batch.handle();
    ORBmatcher matcher(0.6f, false);
    matcher.UploadFusePoints(batch, point_row, vpMP, true, [](MapPointT*) { return false; });
    for (size_t k = 0; k < L.resident.size(); k++) UploadBaKeyFrame(h, L.resident_frame[k], L.resident[k]);
    const int n = (int)vpMP.size(), n_ref = (int)L.kf_role.size();
    check(sd_track_set_ba_keyframes(h, n_ref, L.kf_role.data(), 2));
    ORBmatcher::SetObservations(h, n, L.obs, &L.ba_kf_bad);
    check(sd_track_global_ba(h, point_row, nIterations, bRobust ? 1 : 0, nLoopKF == 0 ? 1 : 0));
    std::vector<double> T_ref((size_t)n_ref * 16 + 16, 0.0), Xw((size_t)n * 3 + 3, 0.0);
    std::vector<uint8_t> point_status((size_t)n + 1, 0);
    double T_cur[16];
    int32_t info[16];
    check(sd_track_get_global_ba(h, T_ref.data(), T_cur, Xw.data(), point_status.data(), info, n));
    if (info[0] != SD_BA_OK) return false;
    if (nLoopKF != 0) {
      for (size_t k = 0; k < L.resident.size(); k++) {
        std::memcpy(L.resident[k]->mTcwGBA.data(), &T_ref[(size_t)L.resident_frame[k] * 16], 128);
        L.resident[k]->mnBAGlobalForKF = nLoopKF;
      }
      for (int i = 0; i < n; i++)
        if (point_status[(size_t)i] == SD_BA_POINT_OPTIMISED) {   // !vbNotIncludedMP[i]
          std::memcpy(vpMP[(size_t)i]->mPosGBA.data(), &Xw[(size_t)i * 3], 24);
          vpMP[(size_t)i]->mnBAGlobalForKF = nLoopKF;
        }
      return true;
    }
    ORBmatcher::RefreshedRows rr((size_t)n);
    if (n > 0) {   // UpdateNormalAndDepth reads every observation: the lists with isBad() alone, on the poses and positions written back
      if (L.ba_kf_bad != L.obs.kf_bad) ORBmatcher::SetObservations(h, n, L.obs);
      check(sd_track_refresh_points(h, point_row, 1));
      check(sd_track_get_refreshed(h, rr.status.data(), nullptr, nullptr, nullptr, rr.normal.data(), rr.max_dist.data(), rr.min_dist.data(), n));
    }
    for (size_t k = 0; k < L.resident.size(); k++) L.resident[k]->SetPose(&T_ref[(size_t)L.resident_frame[k] * 16]);
    for (size_t i = 0; i < (size_t)n; i++) {
      if (point_status[i] != SD_BA_POINT_OPTIMISED) continue;
      vpMP[i]->SetWorldPos(&Xw[i * 3]);
      if ((rr.status[i] & SD_REFRESH_NORMAL) && !L.obs.left[i]) ORBmatcher::SetNormalAndDepth(vpMP[i], rr, i);
    }
    return true;
  }
  // void Optimizer::GlobalBundleAdjustemnt(Map* pMap, int nIterations = 5, bool* pbStopFlag = NULL, nLoopKF = 0, bRobust = true)   :46-50
  // (frameOf follows the reference's parameters, so their defaults cannot be kept: every argument is given)
  template <class MapT, class FrameOf>
  static bool GlobalBundleAdjustemnt(TrackBatch& batch, MapT* pMap, int nIterations, bool* pbStopFlag, const unsigned long nLoopKF,
                                     const bool bRobust, FrameOf frameOf, int point_row = 0) {
    return BundleAdjustment(batch, pMap->GetAllKeyFrames(), pMap->GetAllMapPoints(), nIterations, pbStopFlag, nLoopKF, bRobust, frameOf, point_row);
  }
  template <class KeyFrameT>
  struct GlobalBaLists {
    std::vector<KeyFrameT*> resident;            // the keyframes of vpKFs that are not bad and are frames of the ref extractor, in vpKFs order ...
    std::vector<int> resident_frame;             // ... and their frames
    std::vector<uint8_t> kf_role;                // sd_track_set_ba_keyframes
    ORBmatcher::ObservationLists obs;            // kf_bad: isBad() (what the refresh is given); left[i]: the reference keyframe is not an observation
    std::vector<uint8_t> ba_kf_bad;              // ... || mnId > maxKFid (what the bundle adjustment is given)
  };
  // Host code only: the roles (:74-85) and the CSR lists (:102-110)
  template <class KeyFrameT, class MapPointT, class FrameOf>
  static void BuildGlobalBaLists(const std::vector<KeyFrameT*>& vpKFs, const std::vector<MapPointT*>& vpMP, FrameOf frameOf, GlobalBaLists<KeyFrameT>& L) {
    unsigned long maxKFid = 0;
    L.resident.clear(); L.resident_frame.clear(); L.kf_role.clear();
    for (KeyFrameT* kf : vpKFs) {
      if (kf->isBad()) continue;
      if (kf->mnId > maxKFid) maxKFid = kf->mnId;
      const int f = (int)frameOf(kf);
      if (f < 0) continue;
      L.resident.push_back(kf);
      L.resident_frame.push_back(f);
      if (L.kf_role.size() <= (size_t)f) L.kf_role.resize((size_t)f + 1, 0);
      L.kf_role[(size_t)f] = kf->mnId == 0 ? 2 : 1;
    }
    L.ba_kf_bad.clear();
    ORBmatcher::WalkObservations((KeyFrameT*)nullptr, vpMP, true, frameOf, L.obs, [&](size_t, KeyFrameT* pKFi, size_t) {
      L.ba_kf_bad.push_back(pKFi->isBad() || pKFi->mnId > maxKFid ? 1 : 0);
    });
    if (L.ba_kf_bad.empty()) L.ba_kf_bad.push_back(0);   // as the walk pads kf_bad
  }
  // lLocalKeyFrames, lLocalMapPoints and (through `resident`) lFixedCameras, and what the device is given for them
  template <class KeyFrameT, class MapPointT>
  struct LocalBaLists {
    std::vector<KeyFrameT*> local, fixed;        // lLocalKeyFrames, lFixedCameras, in the reference's order
    std::vector<MapPointT*> points;              // lLocalMapPoints
    std::vector<KeyFrameT*> resident;            // the keyframes of both lists that are frames of the ref extractor ...
    std::vector<int> resident_frame;             // ... and their frames
    std::vector<uint8_t> kf_role;                // sd_track_set_ba_keyframes
    int cur_role = 1;
    ORBmatcher::ObservationLists obs;            // sd_track_set_observations; left[i]: the reference keyframe is not an observation
    std::vector<KeyFrameT*> edge_kf;             // per CSR entry: its keyframe ...
    std::vector<int32_t> edge_pt;                // ... its point ...
    std::vector<uint8_t> edge_stereo;            // ... and mvuRight >= 0
  };
  struct LocalBaResult {
    std::vector<double> T_ref, Xw;
    double T_cur[16] = {};
    std::vector<uint8_t> point_status, obs_erase;
    int32_t info[16] = {};
    LocalBaResult(size_t n_ref, size_t n, size_t e) : T_ref(n_ref * 16 + 16, 0.0), Xw(n * 3 + 3, 0.0), point_status(n + 1, 0), obs_erase(e + 1, 0) {}
  };
  // Host code only: :418-460, then the roles and the CSR lists
  template <class KeyFrameT, class MapPointT, class FrameOf>
  static void BuildLocalBaLists(KeyFrameT* pKF, FrameOf frameOf, LocalBaLists<KeyFrameT, MapPointT>& L) {
    L.local.assign(1, pKF);
    pKF->mnBALocalForKF = pKF->mnId;
    for (KeyFrameT* pKFi : pKF->GetVectorCovisibleKeyFrames()) {
      pKFi->mnBALocalForKF = pKF->mnId;
      if (!pKFi->isBad()) L.local.push_back(pKFi);
    }
    L.points.clear();
    for (KeyFrameT* kf : L.local)
      for (MapPointT* pMP : kf->GetMapPointMatches())
        if (pMP && !pMP->isBad() && pMP->mnBALocalForKF != pKF->mnId) {
          L.points.push_back(pMP);
          pMP->mnBALocalForKF = pKF->mnId;
        }
    L.fixed.clear();
    for (MapPointT* pMP : L.points)
      for (const auto& ob : pMP->GetObservations()) {
        KeyFrameT* pKFi = ob.first;
        if (pKFi->mnBALocalForKF != pKF->mnId && pKFi->mnBAFixedForKF != pKF->mnId) {
          pKFi->mnBAFixedForKF = pKF->mnId;
          if (!pKFi->isBad()) L.fixed.push_back(pKFi);
        }
      }
    L.resident.clear(); L.resident_frame.clear(); L.kf_role.clear();
    L.cur_role = pKF->mnId == 0 ? 2 : 1;
    for (int pass = 0; pass < 2; pass++)
      for (KeyFrameT* kf : pass ? L.fixed : L.local) {
        const int f = kf == pKF ? -1 : (int)frameOf(kf);
        if (f < 0) continue;
        L.resident.push_back(kf);
        L.resident_frame.push_back(f);
        if (pass == 0) {
          if (L.kf_role.size() <= (size_t)f) L.kf_role.resize((size_t)f + 1, 0);
          L.kf_role[(size_t)f] = kf->mnId == 0 ? 2 : 1;
        }
      }
    BuildBaObservations(pKF, frameOf, L);
  }
  // Host code only: the observations of L.points as they are now, in iteration order
  template <class KeyFrameT, class MapPointT, class FrameOf>
  static void BuildBaObservations(KeyFrameT* pKF, FrameOf frameOf, LocalBaLists<KeyFrameT, MapPointT>& L) {
    L.edge_kf.clear(); L.edge_pt.clear(); L.edge_stereo.clear();
    // (lLocalMapPoints is sent as collected: isBad() is not asked again, nor after the erasures)
    ORBmatcher::WalkObservations(pKF, L.points, false, frameOf, L.obs, [&](size_t i, KeyFrameT* pKFi, size_t kp) {
      L.edge_kf.push_back(pKFi);
      L.edge_pt.push_back((int32_t)i);
      L.edge_stereo.push_back(kp < pKFi->mvuRight.size() && !(pKFi->mvuRight[kp] < 0) ? 1 : 0);
    });
  }
  // Host code only: :685-713 without the refresh.  Returns whether anything was erased.
  template <class KeyFrameT, class MapPointT>
  static bool ApplyLocalBa(KeyFrameT* pKF, const LocalBaLists<KeyFrameT, MapPointT>& L, const LocalBaResult& r) {
    bool erased = false;
    for (int stereo = 0; stereo < 2; stereo++)   // vToErase: the mono loop's entries, then the stereo loop's
      for (size_t e = 0; e < L.edge_kf.size(); e++)
        if (r.obs_erase[e] && L.edge_stereo[e] == stereo) {
          L.edge_kf[e]->EraseMapPointMatch(L.points[(size_t)L.edge_pt[e]]);
          L.points[(size_t)L.edge_pt[e]]->EraseObservation(L.edge_kf[e]);
          erased = true;
        }
    for (KeyFrameT* kf : L.local) {
      if (kf == pKF) { kf->SetPose(r.T_cur); continue; }
      for (size_t k = 0; k < L.resident.size(); k++)
        if (L.resident[k] == kf) kf->SetPose(&r.T_ref[(size_t)L.resident_frame[k] * 16]);
    }
    for (size_t i = 0; i < L.points.size(); i++) L.points[i]->SetWorldPos(&r.Xw[i * 3]);
    return erased;
  }
};

// void LocalMapping::KeyFrameCulling()          src/LocalMapping.cc:580-634, the last step of LocalMapping::Run
// on the device (sd_track_cull_keyframes), on the observation lists that are resident: the caller's last
// sd_track_set_observations (Optimizer::LocalBundleAdjustment leaves the local points' lists there), as
// sd_track_erase_observations may have compacted them.
class LocalMapping {
 public:
  // What the device is asked: the candidates in GetVectorCovisibleKeyFrames() order and their flags
  struct CullCandidates {
    std::vector<int32_t> frame;
    std::vector<uint8_t> flags;
    bool resident = true;   // false: a covisible keyframe is not a frame of the ref extractor
  };
  // Host code only.  frameOf(KeyFrameT*): the frame of the ref extractor that holds a keyframe, negative: not resident;
  // notErase(KeyFrameT*): mbNotErase
  template <class KeyFrameT, class FrameOf, class NotErase>
  static CullCandidates BuildCullCandidates(const std::vector<KeyFrameT*>& vpLocalKeyFrames, FrameOf frameOf, NotErase notErase) {
    CullCandidates c;
    for (KeyFrameT* pKF : vpLocalKeyFrames) {
      const int f = (int)frameOf(pKF);
      if (f < 0) c.resident = false;
      c.frame.push_back(f);
      c.flags.push_back((uint8_t)((pKF->mnId == 0 ? 1 : 0) | (notErase(pKF) ? 2 : 0)));
    }
    return c;
  }
  // Host code only: pKF->SetBadFlag() on the keyframes the test passed for, in candidate order -- the caller's own objects do their
  // own cascade (EraseObservation, MapPoint::SetBadFlag, the spanning tree), and a keyframe with mbNotErase sets mbToBeErased.
  // Returns the number of calls.
  template <class KeyFrameT>
  static int ApplyCullVerdicts(const std::vector<KeyFrameT*>& vpLocalKeyFrames, const std::vector<uint8_t>& verdict) {
    int n = 0;
    for (size_t c = 0; c < vpLocalKeyFrames.size(); c++)
      if (verdict[c] == SD_CULL_CULLED || verdict[c] == SD_CULL_TO_BE_ERASED) vpLocalKeyFrames[c]->SetBadFlag(), n++;
    return n;
  }
  // Returns false, with no object touched, when a covisible keyframe is not resident or the device refuses (an observation of a
  // live point in a keyframe that is not resident, a keypoint index outside its frame).  KeyFrameT needs mnId,
  // GetVectorCovisibleKeyFrames() and SetBadFlag().
  template <class KeyFrameT, class FrameOf, class NotErase>
  static bool KeyFrameCulling(TrackBatch& batch, KeyFrameT* pCurrentKF, bool bMonocular, float thDepth, FrameOf frameOf, NotErase notErase) {
    const std::vector<KeyFrameT*> vpLocalKeyFrames = pCurrentKF->GetVectorCovisibleKeyFrames();
    const CullCandidates c = BuildCullCandidates(vpLocalKeyFrames, frameOf, notErase);
    if (!c.resident) return false;
    const int n = (int)c.frame.size();
    check(sd_track_cull_keyframes(batch.handle(), n, c.frame.data(), c.flags.data(), bMonocular ? 1 : 0, thDepth));
    std::vector<uint8_t> verdict((size_t)n + 1, 0);
    int32_t info[8];
    check(sd_track_get_culled(batch.handle(), verdict.data(), nullptr, nullptr, nullptr, nullptr, nullptr, info, n, 0, 0));
    if (info[0] != SD_CULL_OK) return false;
    ApplyCullVerdicts(vpLocalKeyFrames, verdict);
    return true;
  }
  // ... with mbNotErase read off the keyframe
  template <class KeyFrameT, class FrameOf>
  static bool KeyFrameCulling(TrackBatch& batch, KeyFrameT* pCurrentKF, bool bMonocular, float thDepth, FrameOf frameOf) {
    return KeyFrameCulling(batch, pCurrentKF, bMonocular, thDepth, frameOf, [](KeyFrameT* pKF) { return pKF->mbNotErase; });
  }
};

// Tracking::Relocalization (src/Tracking.cc:1064-1097): every keyframe attempt of the loop is one slot of `batch`
// (slot order = the order the reference tries them, kfs.rbegin() first; SetLastFrame = the keyframe's map points,
// SetPoses(kf pose, kf pose)).  Returns the slot at which the reference's loop returns true, or -1.
class Tracking {
 public:
  struct Tracked {
    bool ok;            // return value of TrackWithMotionModel
    int nmatches;       // after "Discard outliers"
    int nmatchesMap;
    bool retried;       // the 2 * threshold search ran
  };
  // Tracking::TrackWithMotionModel (src/Tracking.cc:654-718) for every frame of the batch; the caller has set the last
  // frame (SetLastFrame) and the poses (SetPoses: last pose, motion-model prediction).  referenceKF: ImageAlign against
  // the slot's keyframe as TrackReferenceKeyFrame does (:583-644); align_image = Tracking::align_image_ (:122).
  static void TrackWithMotionModel(TrackBatch& batch, int n_frames, float threshold, bool bMono, bool align_image = true,
                                   bool referenceKF = false) {
    check(sd_track_with_motion_model(batch.handle(), n_frames, align_image ? (referenceKF ? 1 : 0) : -1, threshold, bMono ? 1 : 0, 20, 10));
  }
  // Tracking::TrackLocalMap (src/Tracking.cc:720-751) on top of TrackWithMotionModel's matches and pose; the local map is
  // TrackBatch::SetLocalMap (UpdateLocalMap stays with the caller).  th: 1, 3 for RGB-D, 5 right after a relocalisation.
  static void TrackLocalMap(TrackBatch& batch, int n_frames, float th = 1.f) { check(sd_track_local_map(batch.handle(), n_frames, th, 0.8f, 0.5f, 30)); }
  // returns TrackLocalMap's return value; mnMatchesInliers and mvpMapPoints (v < max_points: last-frame point v, else
  // local map point v - max_points) on request
  static bool LocalMapResult(TrackBatch& batch, int frame, int* mnMatchesInliers = nullptr, std::vector<int32_t>* mvpMapPoints = nullptr,
                             int kp_cap = 0) {
    int32_t i4[4];
    if (mvpMapPoints) mvpMapPoints->resize(kp_cap);
    check(sd_track_get_local_map(batch.handle(), frame, 1, mvpMapPoints ? mvpMapPoints->data() : nullptr, kp_cap, i4));
    if (mnMatchesInliers) *mnMatchesInliers = i4[2];
    return i4[0] == 2;
  }
  // Tracking::NeedNewKeyFrame (src/Tracking.cc:753-826) for every slot, queued, on TrackLocalMap's mnMatchesInliers, the counts
  // of TrackBatch::CloseTrackedPoints(n_frames, 1, mThDepth) and TrackBatch::SetKeyFrameState; frame_id = mCurrentFrame.mnId.
  // The answer is TrackBatch::KeyFrameFlags, or feeds CreateNewKeyFrame directly.
  static void NeedNewKeyFrame(TrackBatch& batch, int n_frames, bool rgbd, int frame_id, int mMinFrames, int mMaxFrames) {
    check(sd_track_need_keyframe(batch.handle(), n_frames, rgbd ? 1 : 0, frame_id, mMinFrames, mMaxFrames));
  }
  // The RGB-D part of Tracking::CreateNewKeyFrame (:837-888, mnLastKeyFrameId :894) for the tracked slots (with use_flags: those
  // whose decision bit 0 is set), queued; source as in AdvanceLastFrame, which then carries the points.
  static void CreateNewKeyFrame(TrackBatch& batch, int n_frames, int source, float mThDepth, bool use_flags, int frame_id) {
    check(sd_track_create_keyframe_points(batch.handle(), n_frames, source, mThDepth, use_flags ? 1 : 0, frame_id));
  }
  static Tracked Result(TrackBatch& batch, int frame) {
    int32_t i4[4];
    check(sd_track_get_tracked(batch.handle(), frame, 1, i4));
    return Tracked{i4[0] == 2, i4[1], i4[2], i4[3] != 0};
  }
  static int Relocalization(TrackBatch& batch, int n_keyframes, int cur_frame, float threshold, bool bMono) {
    int32_t winner = -1;
    check(sd_track_relocalize(batch.handle(), n_keyframes, cur_frame, threshold, bMono ? 1 : 0, 20, 10, &winner, nullptr));
    return winner;
  }
};

// Sim3Solver(pKF1, pKF2, vpMatched12, bFixScale) for the batch (src/Sim3Solver.h, src/Sim3Solver.cc): slot f solves KF1 = the
// batch's current frame f (or the broadcast frame) against KF2 = frame f of the ref extractor, on the match vector
// ORBmatcher::SearchByPoints left on the device (TrackBatch's SearchByPoints) or on one given to SetMatches.
class Sim3Solver {
 public:
  explicit Sim3Solver(bool bFixScale = false) : fix_(bFixScale) { SetRansacParameters(); }
  void SetRansacParameters(double probability = 0.99, int minInliers = 6, int maxIterations = 300) {
    p_ = probability; minInl_ = minInliers; maxIts_ = maxIterations;
  }
  // pMP->GetWorldPos() of both keyframes' map points, [n_frames][n][3], by keypoint index (GetIndexInKeyFrame = identity)
  static void SetPoints(TrackBatch& batch, int frame0, int n_frames, const double* Xw_cur, const double* Xw_ref, int n) {
    check(sd_track_set_sim3_points(batch.handle(), frame0, n_frames, Xw_cur, Xw_ref, n));
  }
  // vpMatched12 of the caller's (indices of pKF2 keypoints, -1 = NULL) instead of SearchByPoints' result
  static void SetMatches(TrackBatch& batch, int frame, const int32_t* vpMatched12, int n) {
    check(sd_track_set_point_matches(batch.handle(), frame, 1, vpMatched12, n));
  }
  // Eigen::Matrix4d iterate(int nIterations, bool &bNoMore, vector<bool> &vbInliers, int &nInliers) for slots 0 .. n_frames - 1:
  // constructs the solvers.  rand_values: 3 raw rand() values per iteration and slot (what SD_SLAM::Random would draw)
  void iterate(TrackBatch& batch, int n_frames, int nIterations, const int32_t* rand_values, int per_frame) {
    check(sd_track_set_rand(batch.handle(), 0, n_frames, rand_values, per_frame));
    check(sd_track_sim3(batch.handle(), n_frames, fix_ ? 1 : 0, p_, minInl_, maxIts_, nIterations));
  }
  // the same on a rand() stream the slots already hold
  void iterate(TrackBatch& batch, int n_frames, int nIterations) {
    check(sd_track_sim3(batch.handle(), n_frames, fix_ ? 1 : 0, p_, minInl_, maxIts_, nIterations));
  }
  // Eigen::Matrix4d find(vector<bool> &vbInliers12, int &nInliers): iterate(mRansacMaxIts)
  void find(TrackBatch& batch, int n_frames) { iterate(batch, n_frames, maxIts_); }
  // a further iterate(nIterations) on the same solvers (mnIterations, the best hypothesis and the stream position carry over)
  void iterateAgain(TrackBatch& batch, int n_frames, int nIterations) { check(sd_track_sim3_iterate(batch.handle(), n_frames, nIterations)); }
  // T12: Eigen::Matrix4d::data() order (column-major); returns false for the reference's Matrix4d::Zero()
  bool Result(TrackBatch& batch, int frame, double T12[16], bool& bNoMore, std::vector<uint8_t>& vbInliers, int& nInliers, int kp_cap,
              int* mnIterations = nullptr) {
    int32_t info[8];
    vbInliers.resize(kp_cap);
    check(sd_track_get_sim3(batch.handle(), frame, 1, T12, nullptr, nullptr, nullptr, vbInliers.data(), kp_cap, info));
    bNoMore = info[2] != 0;
    nInliers = info[1];
    if (mnIterations) *mnIterations = info[3];
    return info[0] != 0;
  }
  // Eigen::Matrix3d GetEstimatedRotation() (column-major), Eigen::Vector3d GetEstimatedTranslation(), float GetEstimatedScale()
  void GetEstimatedRotation(TrackBatch& batch, int frame, double R12[9]) {
    check(sd_track_get_sim3(batch.handle(), frame, 1, nullptr, R12, nullptr, nullptr, nullptr, 0, nullptr));
  }
  void GetEstimatedTranslation(TrackBatch& batch, int frame, double t12[3]) {
    check(sd_track_get_sim3(batch.handle(), frame, 1, nullptr, nullptr, t12, nullptr, nullptr, 0, nullptr));
  }
  float GetEstimatedScale(TrackBatch& batch, int frame) {
    double s = 0;
    check(sd_track_get_sim3(batch.handle(), frame, 1, nullptr, nullptr, nullptr, &s, nullptr, 0, nullptr));
    return (float)s;
  }

 private:
  bool fix_;
  double p_;
  int minInl_, maxIts_;
};

// The candidate search of LoopClosing::DetectLoop (src/LoopClosing.cc:115-149): slot i = kfs[i]; excluded[i] marks the
// current keyframe itself and its connected keyframes.  Returns the slots with error < 1.5 * best (vpCandidateKFs as a set).
class LoopClosing {
 public:
  static std::vector<int32_t> DetectLoopCandidates(TrackBatch& batch, int n_keyframes, int cur_frame, const std::vector<uint8_t>& excluded,
                                                   double* best_error = nullptr) {
    if (!excluded.empty() && (int)excluded.size() < n_keyframes) throw Error(SD_ERR_INVALID_ARG, "excluded shorter than n_keyframes");
    std::vector<int32_t> cand(n_keyframes);
    int32_t n = 0;
    check(sd_track_detect_loop(batch.handle(), n_keyframes, cur_frame, excluded.empty() ? nullptr : excluded.data(), cand.data(),
                               n_keyframes, &n, best_error, nullptr));
    cand.resize(n);
    return cand;
  }

  // The RANSAC round-robin of LoopClosing::ComputeSim3 (src/LoopClosing.cc:270-290) over candidate slots 0 .. n - 1 whose
  // solvers hold their matches, points and rand() streams: SetRansacParameters(0.99, 20, 300) is the caller's (`solver`), then
  // `while (nCandidates > 0 && !bMatch)` every slot not yet discarded runs iterate(5); a slot that reports bNoMore is discarded
  // (:279-282), a slot that returns a Sim3 is offered to accept(slot) -- the reference's SearchBySim3 + OptimizeSim3 (:285-308),
  // which stay with the caller -- and the first accepted slot is returned (bMatch).  A rejected slot stays in the round-robin, as
  // in the reference; -1 when every slot has been discarded.  discarded (may be NULL): the reference's vbDiscarded on entry
  // (candidates with too few matches, :257-260) and on return.
  // The batch iterates slots 0 .. n - 1 together, so a slot rejected or discarded mid-round costs nothing extra and the slots
  // after it in the round run as they would have; the slots after an ACCEPTED one have run one iterate(5) the reference skips
  // (it leaves the loop), which no result read afterwards depends on.
  template <class Accept>
  static int ComputeSim3Candidates(TrackBatch& batch, int n, Sim3Solver& solver, int kp_cap, std::vector<uint8_t>* discarded, Accept accept,
                                   std::vector<int>* iterations = nullptr) {
    std::vector<uint8_t> local((size_t)n, 0);
    std::vector<uint8_t>& gone = discarded ? *discarded : local;
    gone.resize((size_t)n, 0);
    int candidates = 0;
    for (int i = 0; i < n; i++) candidates += !gone[i];
    if (iterations) iterations->assign((size_t)n, 0);
    std::vector<uint8_t> inl;
    bool first = true;
    while (candidates > 0) {
      if (first) solver.iterate(batch, n, 5);
      else solver.iterateAgain(batch, n, 5);
      first = false;
      for (int i = 0; i < n; i++) {
        if (gone[i]) continue;
        double T12[16];
        bool no_more = false;
        int n_inliers = 0, its = 0;
        const bool got = solver.Result(batch, i, T12, no_more, inl, n_inliers, kp_cap, &its);
        if (iterations) (*iterations)[i] = its;
        if (no_more) {
          gone[i] = 1;
          candidates--;
        }
        if (got && accept(i)) {
          // the later slots ran this round too (see above): report the state they are in
          for (int j = i + 1; iterations && j < n; j++)
            if (!gone[j]) {
              solver.Result(batch, j, T12, no_more, inl, n_inliers, kp_cap, &its);
              (*iterations)[j] = its;
            }
          return i;
        }
      }
    }
    return -1;
  }
  static int ComputeSim3Candidates(TrackBatch& batch, int n, Sim3Solver& solver, int kp_cap) {
    return ComputeSim3Candidates(batch, n, solver, kp_cap, nullptr, [](int) { return true; });
  }
};

// ------------------------------------------------------------------------------------------------------------------
// Drop-in overloads on the reference's OWN Frame / MapPoint types: the call sites of
// src/Tracking.cc:668-693 keep their arguments -- `image_align.ComputePose(mCurrentFrame, mLastFrame)`,
// `matcher.SearchByProjection(mCurrentFrame, mLastFrame, th, bMono)`, `Optimizer::PoseOptimization(&mCurrentFrame)` --
// and the SoA flattening of INTEGRATION.md section 3 happens in here.  FrameT / its map-point type only need the reference's
// member names (src/Frame.h, src/MapPoint.h): N, mvpMapPoints, mvbOutlier, mvKeys, mvKeysUn, GetPose(), SetPose(),
// static fx fy cx cy mnMinX mnMaxX mnMinY mnMaxY, mbf; GetWorldPos() (indexable by (k)), GetDescriptor() (with .data),
// Observations(), isBad().  One FrameTracker per camera: `cur` holds the extraction of the current frame, `last` that of the
// previous one (the shimmed ORBextractor of INTEGRATION.md section 3 fills them from Frame's constructor; swap per frame).
class FrameTracker {
 public:
  FrameTracker(ORBextractor& cur, ORBextractor& last, int max_points = 2048, int pnp_max_iterations = 300)
      : batch_(cur, last, max_points, 1, pnp_max_iterations), max_points_(max_points), pnp_max_its_(pnp_max_iterations) {}
  TrackBatch& batch() { return batch_; }
  // What the tracker's map-point arrays hold is remembered between calls: the three calls of one TrackWithMotionModel body
  // (ComputePose, SearchByProjection, PoseOptimization on the same two frames) flatten and upload mLastFrame ONCE.  The key is
  // (object address, mnId, N, the mvpMapPoints pointers and outlier flags); call this when a frame's map points were edited in
  // place some other way (world positions moved by a bundle adjustment between two calls, say).
  void InvalidateCache() { kind_ = NONE; }

  // bool ImageAlign::ComputePose(Frame &CurrentFrame, const Frame &LastFrame)          src/ImageAlign.h:36, src/Tracking.cc:668
  template <class FrameT>
  bool ComputePose(FrameT& CurrentFrame, const FrameT& LastFrame, double* error = nullptr) {
    Upload(CurrentFrame, LastFrame);
    return Align(CurrentFrame, 0, error);
  }
  // bool ImageAlign::ComputePose(Frame &CurrentFrame, KeyFrame *LastKF, bool fast = false)
  //                                                      src/ImageAlign.h:39, src/ImageAlign.cc:106-176, src/Tracking.cc:595,1077
  // The points are LastKF->GetMapPoints() in ITS iteration order (a std::set<MapPoint*> in the reference: pointer order), the
  // first 300 (100 when fast); neither isBad() nor outlier flags are looked at (src/ImageAlign.cc:129-136).  The `last`
  // extractor must hold the keyframe's frame (its pyramid is what the reference reads from LastKF->mvImagePyramid).
  template <class FrameT, class KeyFrameT>
  bool ComputePose(FrameT& CurrentFrame, KeyFrameT* LastKF, bool fast = false, double* error = nullptr) {
    SetCameraOf(CurrentFrame);
    UploadSetPoints(LastKF);
    const auto Tl = LastKF->GetPose();
    const auto Tc = CurrentFrame.GetPose();
    for (int i = 0; i < 16; i++) last_pose_[i] = Tl.data()[i];
    check(sd_track_set_poses(batch_.handle(), 0, 1, Tl.data(), Tc.data()));
    return Align(CurrentFrame, fast ? 2 : 1, error);
  }
  // bool ImageAlign::ComputePose(KeyFrame *CurrentKF, KeyFrame *LastKF)                src/ImageAlign.h:42, src/LoopClosing.cc:133
  // level 4 only, identity start, rejected above 0.03; no pose is written.  The `cur` extractor holds CurrentKF's frame.
  template <class KeyFrameT>
  bool ComputePose(KeyFrameT* CurrentKF, KeyFrameT* LastKF, double* error = nullptr) {
    SetCameraOf(*CurrentKF);
    UploadSetPoints(LastKF);
    const auto Tl = LastKF->GetPose();
    const auto Tc = CurrentKF->GetPose();
    check(sd_track_set_poses(batch_.handle(), 0, 1, Tl.data(), Tc.data()));
    check(sd_track_align(batch_.handle(), 1, 3));
    int32_t ok = 0;
    check(sd_track_get_align(batch_.handle(), 0, 1, nullptr, error, &ok, nullptr, nullptr));
    return ok != 0;
  }
  // int ORBmatcher::SearchByProjection(Frame &CurrentFrame, const Frame &LastFrame, const float th, const bool bMono)
  //                                                                                     src/ORBmatcher.h:46, src/Tracking.cc:677
  template <class FrameT>
  int SearchByProjection(FrameT& CurrentFrame, const FrameT& LastFrame, float th, bool bMono, bool checkOrientation = true) {
    Upload(CurrentFrame, LastFrame);
    return Search(CurrentFrame, LastFrame.mvpMapPoints, th, bMono, checkOrientation);
  }
  // int ORBmatcher::SearchByProjection(Frame &CurrentFrame, KeyFrame *pKF, const float th, const bool bMono)
  //                                                      src/ORBmatcher.h:52, src/ORBmatcher.cc:1077-1207, src/Tracking.cc:603,1083
  // over pKF->GetMapPointMatches() (NULL and isBad() points skipped), octave / angle from pKF->mvKeys / mvKeysUn
  template <class FrameT, class KeyFrameT>
  int SearchByProjection(FrameT& CurrentFrame, KeyFrameT* pKF, float th, bool bMono, bool checkOrientation = true) {
    SetCameraOf(CurrentFrame);
    const auto vpMapPointMatches = pKF->GetMapPointMatches();
    const int n = (int)vpMapPointMatches.size();
    if (!Cached(KF_MATCHES, pKF, IdOf(*pKF, 0), n, vpMapPointMatches, nullptr)) {
      LastFrameView v;
      Blank(v, n);
      for (int i = 0; i < n; i++) {
        v.octave[i] = pKF->mvKeys[i].octave;
        v.angle[i] = pKF->mvKeysUn[i].angle;
        auto* p = vpMapPointMatches[i];
        if (!p || p->isBad()) continue;
        FillPoint(v, i, p);
      }
      batch_.SetLastFrame(0, v);
    }
    const auto Tl = pKF->GetPose();
    const auto Tc = CurrentFrame.GetPose();
    for (int i = 0; i < 16; i++) last_pose_[i] = Tl.data()[i];
    check(sd_track_set_poses(batch_.handle(), 0, 1, Tl.data(), Tc.data()));
    return Search(CurrentFrame, vpMapPointMatches, th, bMono, checkOrientation);
  }
  // int ORBmatcher::SearchByProjection(Frame &F, const vector<MapPoint*> &vpMapPoints, const float th)
  //                                                      src/ORBmatcher.h:47, src/ORBmatcher.cc:43-119, src/Tracking.cc:937
  // on the isInFrustum results the caller's SearchLocalPoints left in the map points (mbTrackInView, mTrackProjX / Y / XR,
  // mnTrackScaleLevel, mTrackViewCos); keypoints of F that already hold a point with Observations() > 0 stay closed.
  template <class FrameT, class MapPointT>
  int SearchByProjection(FrameT& F, const std::vector<MapPointT*>& vpMapPoints, float th, float nnratio = 0.8f) {
    SetCameraOf(F);
    kind_ = NONE;
    const int n = (int)vpMapPoints.size();
    if (n > max_points_) throw Error(SD_ERR_CAPACITY, "more local map points than the tracker's max_points");
    std::vector<uint8_t> in_view((size_t)max_points_, 0), desc((size_t)max_points_ * 32, 0), claimed((size_t)cap(F), 0);
    std::vector<float> proj((size_t)max_points_ * 3, 0.f), vcos((size_t)max_points_, 0.f);
    std::vector<int32_t> level((size_t)max_points_, 0), obs((size_t)max_points_, 0);
    for (int i = 0; i < n; i++) {
      auto* p = vpMapPoints[i];
      if (!p->mbTrackInView || p->isBad()) continue;
      in_view[i] = 1;
      proj[(size_t)i * 3] = p->mTrackProjX; proj[(size_t)i * 3 + 1] = p->mTrackProjY; proj[(size_t)i * 3 + 2] = p->mTrackProjXR;
      level[i] = p->mnTrackScaleLevel;
      vcos[i] = p->mTrackViewCos;
      const auto D = p->GetDescriptor();
      for (int k = 0; k < 32; k++) desc[(size_t)i * 32 + k] = D.data[k];
      obs[i] = p->Observations();
    }
    for (int i = 0; i < F.N; i++) claimed[i] = F.mvpMapPoints[i] && F.mvpMapPoints[i]->Observations() > 0;
    UploadURight(F, 0);
    check(sd_track_set_local_view(batch_.handle(), 0, 1, &n, in_view.data(), proj.data(), level.data(), vcos.data(), desc.data(), obs.data(),
                                  claimed.data()));
    check(sd_track_match_local_view(batch_.handle(), 1, th, nnratio));
    std::vector<int32_t> idx(cap(F));
    int32_t nm = 0;
    check(sd_track_get_local(batch_.handle(), 0, 1, idx.data(), (int)idx.size(), &nm, nullptr, nullptr, nullptr, nullptr));
    for (int i = 0; i < F.N; i++)
      if (idx[i] >= 0) F.mvpMapPoints[i] = vpMapPoints[idx[i]];
    return nm;
  }
  // int Optimizer::PoseOptimization(Frame *pFrame)                                       src/Optimizer.h, src/Tracking.cc:693
  // on whatever pFrame->mvpMapPoints holds.  Right behind a SearchByProjection on the same frame -- mvpMapPoints still exactly what
  // that search assigned -- the matches and map points are already on the device and only the pose travels; otherwise keypoint
  // i <-> map point i is flattened (sd_track_set_matches).
  template <class FrameT>
  int PoseOptimization(FrameT* pFrame) {
    FrameT& F = *pFrame;
    SetCameraOf(F);
    bool resident = searched_frame_ == (const void*)pFrame && searched_id_ == IdOf(F, 0) && (int)assigned_.size() == F.N && kind_ != NONE &&
                    kind_ != CUR_POINTS;
    for (int i = 0; resident && i < F.N; i++) resident = (const void*)F.mvpMapPoints[i] == assigned_[i];
    const auto Tc = F.GetPose();
    if (resident) {
      check(sd_track_set_poses(batch_.handle(), 0, 1, last_pose_, Tc.data()));
    } else {
      LastFrameView v;
      std::vector<int32_t> cm((size_t)F.N, -1);
      Blank(v, F.N);
      for (int i = 0; i < F.N; i++) {
        auto* p = F.mvpMapPoints[i];
        if (!p) continue;
        v.valid[i] = 1;
        cm[i] = i;
        const auto X = p->GetWorldPos();
        for (int k = 0; k < 3; k++) v.Xw[(size_t)i * 3 + k] = X(k);
        v.obs[i] = p->Observations();
      }
      batch_.SetLastFrame(0, v);
      kind_ = CUR_POINTS;
      check(sd_track_set_poses(batch_.handle(), 0, 1, Tc.data(), Tc.data()));
      check(sd_track_set_matches(batch_.handle(), 0, 1, cm.data(), F.N));
    }
    UploadURight(F, 0);                        // stereo edges where mvuRight >= 0 (src/Optimizer.cc:262-300)
    check(sd_track_pose_opt(batch_.handle(), 1, 0));
    std::vector<uint8_t> outl(cap(F));
    double T[16];
    int32_t info[8];
    check(sd_track_get_pose_opt(batch_.handle(), 0, 1, T, outl.data(), (int)outl.size(), info));
    SetPoseOf(F, T);
    for (int i = 0; i < F.N; i++)
      if (F.mvpMapPoints[i]) F.mvbOutlier[i] = outl[i] != 0;
    return info[5];
  }

  // PnPsolver(const Frame &F, const vector<MapPoint*> &vpMapPointMatches) + SetRansacParameters + find / iterate
  //                                                      src/PnPsolver.h:67-76, src/PnPsolver.cc:71-244
  // (dead code in the reference; kept because BASELINE names it).  One solver per FrameTracker at a time.  rand_fn
  // supplies what SD_SLAM::Random would draw from rand() (src/extra/utils.cc:23-26): minSet values per iteration, drawn up
  // front for the iterations the call may run (the reference draws them one iteration at a time).
  template <class FrameT, class MapPointT>
  void PnPsolverConstruct(const FrameT& F, const std::vector<MapPointT*>& vpMapPointMatches) {
    SetCameraOf(F);
    const int n = (int)vpMapPointMatches.size();
    LastFrameView v;
    Blank(v, n);
    std::vector<int32_t> cm((size_t)n, -1);
    for (int i = 0; i < n; i++) {
      auto* p = vpMapPointMatches[i];
      if (!p || p->isBad()) continue;          // src/PnPsolver.cc:84-87
      v.valid[i] = 1;
      cm[i] = i;
      const auto X = p->GetWorldPos();
      for (int k = 0; k < 3; k++) v.Xw[(size_t)i * 3 + k] = X(k);
    }
    batch_.SetLastFrame(0, v);
    kind_ = CUR_POINTS;
    const auto Tc = F.GetPose();
    check(sd_track_set_poses(batch_.handle(), 0, 1, Tc.data(), Tc.data()));
    check(sd_track_set_matches(batch_.handle(), 0, 1, cm.data(), n));
    pnp_n_ = n;
    pnp_started_ = false;
    SetRansacParameters();
  }
  void SetRansacParameters(double probability = 0.99, int minInliers = 8, int maxIterations = 300, int minSet = 4, float epsilon = 0.4f,
                           float th2 = 5.991f) {
    pnp_p_ = probability; pnp_min_inl_ = minInliers; pnp_max_iterations_ = maxIterations; pnp_min_set_ = minSet; pnp_eps_ = epsilon;
    pnp_th2_ = th2;
    pnp_started_ = false;
  }
  // cv::Mat iterate(int nIterations, bool &bNoMore, vector<bool> &vbInliers, int &nInliers): Tcw = 4 x 4 CV_32F row-major;
  // returns false for the reference's empty Mat
  template <class RandFn>
  bool iterate(int nIterations, bool& bNoMore, std::vector<bool>& vbInliers, int& nInliers, float Tcw[16], RandFn rand_fn) {
    if (pnp_n_ < 0) throw Error(SD_ERR_INVALID_ARG, "PnPsolverConstruct has not been called");
    if (!pnp_started_) {
      // the first call may run to max(mRansacMaxIts, nIterations) (the `||` of src/PnPsolver.cc:177); later calls add nIterations each
      const int per_frame = 4 * pnp_max_its_;
      std::vector<int32_t> r((size_t)per_frame);
      for (auto& x : r) x = (int32_t)rand_fn();
      check(sd_track_set_rand(batch_.handle(), 0, 1, r.data(), per_frame));
      check(sd_track_pnp(batch_.handle(), 1, pnp_p_, pnp_min_inl_, pnp_max_iterations_, pnp_min_set_, pnp_eps_, pnp_th2_, nIterations));
      pnp_started_ = true;
    } else {
      check(sd_track_pnp_iterate(batch_.handle(), 1, nIterations));
    }
    std::vector<uint8_t> inl((size_t)(pnp_n_ > max_points_ ? pnp_n_ : max_points_));
    int32_t info[8];
    check(sd_track_get_pnp(batch_.handle(), 0, 1, Tcw, inl.data(), (int)inl.size(), info));
    bNoMore = info[2] != 0;
    nInliers = info[1];
    vbInliers.assign((size_t)pnp_n_, false);
    for (int i = 0; i < pnp_n_; i++) vbInliers[i] = inl[i] != 0;
    return info[0] != 0;
  }
  // cv::Mat find(vector<bool> &vbInliers, int &nInliers) { bool bFlag; return iterate(mRansacMaxIts, bFlag, vbInliers, nInliers); }
  template <class RandFn>
  bool find(std::vector<bool>& vbInliers, int& nInliers, float Tcw[16], RandFn rand_fn) {
    bool bFlag;
    return iterate(pnp_max_iterations_, bFlag, vbInliers, nInliers, Tcw, rand_fn);
  }

 private:
  enum Kind { NONE, FRAME_POINTS, KF_SET_POINTS, KF_MATCHES, CUR_POINTS };
  template <class FrameT>
  int cap(const FrameT& F) { return F.N > max_points_ ? F.N : max_points_; }
  // frame / keyframe identity for the cache: mnId where the type has one (src/Frame.h:121, src/KeyFrame.h:112)
  template <class T>
  static auto IdOf(const T& F, int) -> decltype((unsigned long long)F.mnId) { return (unsigned long long)F.mnId; }
  template <class T>
  static unsigned long long IdOf(const T&, long) { return 0; }
  static void Blank(LastFrameView& v, int n) {
    v.valid.assign(n, 0); v.Xw.assign((size_t)n * 3, 0.0); v.desc.assign((size_t)n * 32, 0);
    v.octave.assign(n, 0); v.angle.assign(n, 0.f); v.obs.assign(n, 0);
  }
  template <class MapPointT>
  static void FillPoint(LastFrameView& v, int i, MapPointT* p) {
    v.valid[i] = 1;
    const auto X = p->GetWorldPos();
    for (int k = 0; k < 3; k++) v.Xw[(size_t)i * 3 + k] = X(k);
    const auto D = p->GetDescriptor();
    for (int k = 0; k < 32; k++) v.desc[(size_t)i * 32 + k] = D.data[k];
    v.obs[i] = p->Observations();
  }
  // is (kind, object, id, the pointer vector [+ outlier flags]) what the tracker's arrays already hold?  Records it otherwise.
  template <class Vec>
  bool Cached(Kind kind, const void* obj, unsigned long long id, int n, const Vec& pts, const std::vector<bool>* outl) {
    bool same = kind_ == kind && key_obj_ == obj && key_id_ == id && (int)key_pts_.size() == n;
    for (int i = 0; same && i < n; i++) same = key_pts_[i] == (const void*)pts[i] && (!outl || key_outl_[i] == (*outl)[i]);
    if (same) return true;
    kind_ = kind; key_obj_ = obj; key_id_ = id;
    key_pts_.resize(n);
    key_outl_.assign(n, false);
    for (int i = 0; i < n; i++) {
      key_pts_[i] = (const void*)pts[i];
      if (outl) key_outl_[i] = (*outl)[i];
    }
    return false;
  }
  // CurrentFrame.mvuRight (filled by Frame::ComputeStereoFromRGBD / ComputeStereoMatches in the reference's constructor)
  template <class FrameT>
  auto UploadURight(const FrameT& F, int) -> decltype((void)F.mvuRight) {
    if (!F.mvuRight.empty()) batch_.SetURight(0, F.mvuRight.data(), (int)F.mvuRight.size());
  }
  template <class FrameT>
  void UploadURight(const FrameT&, long) {}   // frame types without mvuRight (monocular builds)
  // Frame's camera members are static (src/Frame.h:109-112,175-178), KeyFrame's are per-object constants (src/KeyFrame.h:148,169-172):
  // instance access reads both
  template <class FrameT>
  void SetCameraOf(const FrameT& F) {
    batch_.SetCamera(F.fx, F.fy, F.cx, F.cy, F.mbf, (float)F.mnMinX, (float)F.mnMaxX, (float)F.mnMinY, (float)F.mnMaxY);
  }
  template <class FrameT>
  static void SetPoseOf(FrameT& F, const double T[16]) {
    auto M = F.GetPose();                      // Eigen::Matrix4d: 16 doubles column-major behind data()
    for (int i = 0; i < 16; i++) M.data()[i] = T[i];
    F.SetPose(M);
  }
  template <class FrameT>
  bool Align(FrameT& CurrentFrame, int mode, double* error) {
    check(sd_track_align(batch_.handle(), 1, mode));
    double T[16];
    int32_t ok = 0;
    check(sd_track_get_align(batch_.handle(), 0, 1, T, error, &ok, nullptr, nullptr));
    if (ok) SetPoseOf(CurrentFrame, T);
    return ok != 0;
  }
  // the search on what the tracker's arrays hold; `source` = the pointer vector the indices refer to
  template <class FrameT, class Vec>
  int Search(FrameT& CurrentFrame, const Vec& source, float th, bool bMono, bool checkOrientation) {
    if (!bMono) UploadURight(CurrentFrame, 0);   // RGB-D / stereo: the mvuRight gate of src/ORBmatcher.cc:1020-1025
    check(sd_track_match(batch_.handle(), 1, th, bMono ? 1 : 0, checkOrientation ? 1 : 0));
    std::vector<int32_t> idx(CurrentFrame.N > 0 ? cap(CurrentFrame) : 1);
    int32_t n = 0;
    check(sd_track_get_matches(batch_.handle(), 0, 1, idx.data(), (int)idx.size(), &n));
    for (int i = 0; i < CurrentFrame.N; i++)
      if (idx[i] >= 0) CurrentFrame.mvpMapPoints[i] = source[idx[i]];   // the search only ever ASSIGNS
    // remembered for PoseOptimization's resident path: valid when the caller had cleared mvpMapPoints before the search, as
    // every call site of the reference does (src/Tracking.cc:602,676,1080) -- PoseOptimization compares pointer by pointer
    searched_frame_ = (const void*)&CurrentFrame;
    searched_id_ = IdOf(CurrentFrame, 0);
    assigned_.assign((size_t)CurrentFrame.N, nullptr);
    for (int i = 0; i < CurrentFrame.N; i++)
      if (idx[i] >= 0) assigned_[i] = (const void*)source[idx[i]];
    return n;
  }
  // LastKF->GetMapPoints() in iteration order, the first 300 (what ImageAlign's KeyFrame overloads gather)
  template <class KeyFrameT>
  void UploadSetPoints(KeyFrameT* LastKF) {
    const auto mappoints = LastKF->GetMapPoints();
    std::vector<const void*> ptrs;
    for (auto it = mappoints.begin(); it != mappoints.end() && (int)ptrs.size() < 300; ++it) ptrs.push_back((const void*)*it);
    const int n = (int)ptrs.size();
    if (n > max_points_) throw Error(SD_ERR_CAPACITY, "FrameTracker max_points below 300");
    if (Cached(KF_SET_POINTS, LastKF, IdOf(*LastKF, 0), n, ptrs, nullptr)) return;
    LastFrameView v;
    Blank(v, n);
    int i = 0;
    for (auto it = mappoints.begin(); it != mappoints.end() && i < n; ++it, ++i) {
      v.valid[i] = 1;
      const auto X = (*it)->GetWorldPos();
      for (int k = 0; k < 3; k++) v.Xw[(size_t)i * 3 + k] = X(k);
    }
    batch_.SetLastFrame(0, v);
  }
  // what TrackWithMotionModel reads of mLastFrame (src/ImageAlign.cc:64-72, src/ORBmatcher.cc:968-1042) + both poses
  template <class FrameT>
  void Upload(const FrameT& CurrentFrame, const FrameT& LastFrame) {
    SetCameraOf(CurrentFrame);
    const int n = LastFrame.N;
    if (!Cached(FRAME_POINTS, &LastFrame, IdOf(LastFrame, 0), n, LastFrame.mvpMapPoints, &LastFrame.mvbOutlier)) {
      LastFrameView v;
      Blank(v, n);
      for (int i = 0; i < n; i++) {
        v.octave[i] = LastFrame.mvKeys[i].octave;
        v.angle[i] = LastFrame.mvKeysUn[i].angle;
        auto* p = LastFrame.mvpMapPoints[i];
        if (!p || LastFrame.mvbOutlier[i]) continue;
        FillPoint(v, i, p);
      }
      batch_.SetLastFrame(0, v);
    }
    const auto Tl = LastFrame.GetPose();
    const auto Tc = CurrentFrame.GetPose();
    for (int i = 0; i < 16; i++) last_pose_[i] = Tl.data()[i];
    check(sd_track_set_poses(batch_.handle(), 0, 1, Tl.data(), Tc.data()));
  }
  TrackBatch batch_;
  int max_points_, pnp_max_its_;
  Kind kind_ = NONE;
  const void* key_obj_ = nullptr;
  unsigned long long key_id_ = 0;
  std::vector<const void*> key_pts_;
  std::vector<bool> key_outl_;
  const void* searched_frame_ = nullptr;
  unsigned long long searched_id_ = 0;
  std::vector<const void*> assigned_;
  double last_pose_[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
  int pnp_n_ = -1;
  bool pnp_started_ = false;
  double pnp_p_ = 0.99;
  int pnp_min_inl_ = 8, pnp_max_iterations_ = 300, pnp_min_set_ = 4;
  float pnp_eps_ = 0.4f, pnp_th2_ = 5.991f;
};

class PnPsolver {
 public:
  PnPsolver() { SetRansacParameters(); }
  void SetRansacParameters(double probability = 0.99, int minInliers = 8, int maxIterations = 300, int minSet = 4, float epsilon = 0.4f,
                           float th2 = 5.991f) {
    p_ = probability; minInl_ = minInliers; maxIts_ = maxIterations; minSet_ = minSet; eps_ = epsilon; th2_ = th2;
  }
  // cv::Mat iterate(int nIterations, bool &bNoMore, vector<bool> &vbInliers, int &nInliers) for the batch;
  // rand_values: 4 raw rand() values per iteration and frame (what SD_SLAM::Random would draw)
  void iterate(TrackBatch& batch, int n_frames, int nIterations, const int32_t* rand_values, int per_frame) {
    check(sd_track_set_rand(batch.handle(), 0, n_frames, rand_values, per_frame));
    check(sd_track_pnp(batch.handle(), n_frames, p_, minInl_, maxIts_, minSet_, eps_, th2_, nIterations));
  }
  // a further iterate(nIterations) on the same solvers (mnIterations and the best hypothesis carry over, src/PnPsolver.cc:177)
  void iterateAgain(TrackBatch& batch, int n_frames, int nIterations) { check(sd_track_pnp_iterate(batch.handle(), n_frames, nIterations)); }
  // PnPsolver(F, vpMapPointMatches) on a match vector of the caller's (indices into the last-frame arrays, -1 = NULL)
  static void SetMatches(TrackBatch& batch, int frame, const int32_t* vpMapPointMatches, int n) {
    check(sd_track_set_matches(batch.handle(), frame, 1, vpMapPointMatches, n));
  }
  // Tcw: 4x4 CV_32F row-major; returns false for the reference's empty cv::Mat
  bool Result(TrackBatch& batch, int frame, float Tcw[16], bool& bNoMore, std::vector<uint8_t>& vbInliers, int& nInliers, int kp_cap) {
    int32_t info[8];
    vbInliers.resize(kp_cap);
    check(sd_track_get_pnp(batch.handle(), frame, 1, Tcw, vbInliers.data(), kp_cap, info));
    bNoMore = info[2] != 0;
    nInliers = info[1];
    return info[0] != 0;
  }

 private:
  double p_;
  int minInl_, maxIts_, minSet_;
  float eps_, th2_;
};

}  // namespace SD_SLAM
