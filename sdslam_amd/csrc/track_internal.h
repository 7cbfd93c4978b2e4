// Internal structures of the sd_track handle (batched TrackWithMotionModel context).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "orb_internal.h"

namespace sd {

// Device-resident per-frame arrays (frame index f selects a slice of each).
struct TrackBuffers {
  int max_points;        // capacity M of the last-frame arrays
  int kp_cap;            // keypoint capacity of the current frame (extractor's nsel)
  int cur_bcast;         // >= 0: every batch slot pairs with THIS frame of the `cur` extractor (one current frame against
                         // many keyframes: Relocalization, DetectLoop); -1: slot f pairs with current frame f
  // last frame (LastFrame.mvpMapPoints flattened; index i == last-frame keypoint index)
  uint8_t* valid;        // [B][M]   pMP != NULL && !mvbOutlier[i]
  double* Xw;            // [B][M][3] pMP->GetWorldPos()
  uint8_t* mp_desc;      // [B][M][32] pMP->GetDescriptor()
  int32_t* octave;       // [B][M]   LastFrame.mvKeys[i].octave
  float* angle;          // [B][M]   LastFrame.mvKeysUn[i].angle
  int32_t* obs;          // [B][M]   pMP->Observations()
  int32_t* n_last;       // [B]
  int32_t* last_id;      // [B][M]   caller's identity of the point (sd_track_set_map_ids 0), -1: none
  // second last-frame SoA: sd_track_advance writes the next last frame here, then the handle swaps the two
  uint8_t* valid2;
  double* Xw2;
  uint8_t* mp_desc2;
  int32_t* octave2;
  float* angle2;
  int32_t* obs2;
  int32_t* last_id2;
  // poses, 16 doubles column-major (Eigen::Matrix4d::data())
  double* Tref;          // [B][16]  LastFrame.GetPose()
  double* Tprior;        // [B][16]  CurrentFrame pose before alignment (motion-model prediction)
  double* Tcur;          // [B][16]  CurrentFrame pose after ImageAlign (= Tprior when it returns false)
  // ImageAlign outputs
  int32_t* al_ok;        // [B]
  double* al_err;        // [B]  error_
  double* al_chi2;       // [B]  chi2_
  int32_t* al_iters;     // [B][16] iterations run per pyramid level
  // SearchByProjection outputs
  int32_t* cur_match;    // [B][kp_cap]  index into the last-frame arrays or -1
  int32_t* n_matches;    // [B]
  uint32_t* mt_list;     // [B][8192] split matcher: candidate keys of the frame's points, in point order (track_match.hip)
  uint32_t* mt_pt;       // [B][M]    ... offset << 16 | count of every point's keys
  uint32_t* mt_key;      // [B][2048] ... the frame's sorted grid keys and cell starts (slow path of the assignment loop)
  uint16_t* mt_cstart;   // [B][64*48+4]
  int32_t* retry_list;   // [1 + B]: count, then the frames whose first search found too few matches (TrackWithMotionModel's retry)
  float* uright;         // [B][kp_cap]  CurrentFrame.mvuRight (-1: no stereo/depth information)
  float* depth;          // [B][kp_cap]  CurrentFrame.mvDepth
  // PnP
  int32_t* rand_stream;  // [B][4*pnp_max_its] raw rand() values
  float* pnp_T;          // [B][16] row-major CV_32F 4x4
  uint8_t* pnp_inliers;  // [B][kp_cap]
  int32_t* pnp_info;     // [B][8]: ok, nInliers, noMore, iterations, N, minInliers, maxIts, refined
  float* pnp_scratch;    // [B][kp_cap*5] EPnP refit: the best set's correspondences, compacted (pws f32 x 3 | us f32 x 2)
  float* pnp_pts;        // [B][kp_cap][6] gathered correspondences {u, v, X, Y, Z, maxErr}
  uint16_t* pnp_kpidx;   // [B][kp_cap] mvKeyPointIndices
  // PnPsolver members that persist between iterate() calls (sd_track_pnp constructs, sd_track_pnp_iterate continues)
  int32_t* pnp_state;    // [B][4]: mnIterations, mnBestInliers, Refine() outcome for the current best set, 0
  unsigned long long* pnp_best_mask;   // [B][32] mvbBestInliers as bits over the gathered correspondences
  float* pnp_best_T;     // [B][12] mBestTcw (R row-major, t)
  // ORBmatcher::SearchByPoints (brute-force Hamming between two keyframes' map points)
  uint8_t* sp_valid1;    // [B][kp_cap] currentKF keypoint holds a map point that is not bad
  uint8_t* sp_valid2;    // [B][kp_cap] the same for pKF (the `ref` extractor's frame)
  int32_t* sp_match;     // [B][kp_cap] pKF keypoint index assigned to the currentKF keypoint, or -1
  int32_t* sp_n;         // [B]
  // ORBmatcher::SearchForTriangulation (track_tri.hip) on the same pairing and the same flags, read as "holds a map point"
  float* uright_ref;     // [B][kp_cap]  mvuRight of the ref extractor's frames (-1: none)
  double* tri_F12_set;   // [B][9] the caller's F12, row-major (sd_track_set_f12)
  double* tri_F12;       // [B][9] the F12 the last search used: ComputeF12 or the caller's
  float* tri_epi;        // [B][2] the epipole in KF2
  int32_t* tri_match;    // [B][kp_cap] KF2 keypoint index matched to the KF1 keypoint, or -1
  int32_t* tri_n;        // [B]
  // local map (TrackLocalMap's search); capacity M like the last-frame arrays
  uint8_t* lm_cand;      // [B][M]   point reaches isInFrustum (not bad, not already seen in this frame)
  double* lm_Xw;         // [B][M][3]
  double* lm_normal;     // [B][M][3] GetNormal()
  float* lm_min;         // [B][M]   GetMinDistanceInvariance()
  float* lm_max;         // [B][M]   GetMaxDistanceInvariance()
  float* lm_mfmax;       // [B][M]   mfMaxDistance
  uint8_t* lm_desc;      // [B][M][32]
  int32_t* lm_obs;       // [B][M]
  int32_t* lm_id;        // [B][M]   caller's identity of the point (sd_track_set_map_ids 1), -1: none
  int32_t* lm_n;         // [B]
  uint8_t* lm_kclaim;    // [B][kp_cap] keypoint already holds a point with Observations() > 0
  // outputs
  uint8_t* lm_inview;    // [B][M]   mbTrackInView
  float* lm_proj;        // [B][M][3] mTrackProjX, mTrackProjY, mTrackProjXR
  int32_t* lm_level;     // [B][M]   mnTrackScaleLevel
  float* lm_cos;         // [B][M]   mTrackViewCos
  int32_t* lm_match;     // [B][kp_cap] index into the local-map arrays or -1
  int32_t* lm_nmatch;    // [B]
  // Optimizer::PoseOptimization outputs
  double* po_T;          // [B][16] optimised Tcw, column-major
  uint8_t* po_outlier;   // [B][kp_cap] mvbOutlier
  int32_t* po_info;      // [B][8]: nInitialCorrespondences, nBad, rounds, g2o iterations, LM trials, nInitial - nBad
  // Tracking::TrackWithMotionModel outcome (sd_track_with_motion_model)
  int32_t* tw_info;      // [B][4]: status (0 few matches, 1 few inliers, 2 tracked), nmatches after the outlier discard,
                         //         nmatchesMap, 1 if the wider-window retry ran
  int32_t* tw_seen;      // [B][kp_cap] the final search's matches BEFORE the outlier discard: the points whose mnLastFrameSeen
                         //             TrackWithMotionModel sets, which SearchLocalPoints skips (src/Tracking.cc:703, :900-918)
  uint32_t* tw_seen_ids; // [B][kp_cap] their ids (last_id), ascending, 0xFFFFFFFF for none (k_seen_ids, sd_track_local_map)
  // Tracking::TrackLocalMap (sd_track_local_map): mvpMapPoints after SearchLocalPoints = frame matches + local matches
  int32_t* un_match;     // [B][kp_cap] -1 | v < M: last-frame point v | v >= M: local map point v - M
  int32_t* tl_info;      // [B][4]: status (1 failed, 2 tracked), points in mvpMapPoints, mnMatchesInliers, local matches
  // map point creation (track_newpoints.hip): Tracking::StereoInitialization / CreateNewKeyFrame on the current frame
  uint8_t* np_flag;      // [B][kp_cap] keypoint i received a new map point in the last creation call
  double* np_Xw;         // [B][kp_cap][3] its world position (Frame::UnprojectStereo), valid where np_flag
  int32_t* np_id;        // [B][kp_cap] its id (MapPoint::nNextId order), valid where np_flag
  int32_t* np_list;      // [B][kp_cap] the created keypoint indices in creation order
  int32_t* np_info;      // [B][4]: mode (0 nothing ran on the slot, 1 keyframe, 2 initialisation), created, P (entries of the
                         //         depth-sorted list the loop processed), candidates (keypoints with mvDepth > 0)
  int32_t* next_id;      // [B]    MapPoint::nNextId of the slot's map (sd_track_set_next_map_id)
  int32_t* kf_state;     // [B][8] NeedNewKeyFrame's caller state: nKFs, nRefMatches, mnLastKeyFrameId, mnLastRelocFrameId, flags
  uint8_t* kf_flags;     // [B]    bit 0 insert a keyframe, bit 1 wanted but the mapper is busy (InterruptBA)
  // motion model (track_motion.hip): EKF + ConstantVelocity of every slot
  double* mo_X;          // [B][6]  X_ = (v, w)
  double* mo_P;          // [B][6]  diagonal of P_ (the off-diagonals are exactly 0, see track_motion.hip)
  int32_t* mo_started;   // [B]     updated_ (EKF::Started())
  double* mo_it;         // [B]     it_time_
  double* mo_last;       // [B][16] Sensor::last_pose_ (SetLastPose), column-major
  double* mo_E;          // [B][16] Exp(X_) of the last prediction, column-major
  // IMU sensor model (track_imu.hip): EKF + IMU of every slot, used instead of mo_* under SD_SENSOR_IMU
  double* im_X;          // [B][16] X_ = (x, q as w x y z, v, w, a)
  double* im_P;          // [B][256] P_, dense, row-major
  double* im_g;          // [B][3]  IMU::gravity_
  int32_t* im_started;   // [B]     updated_
  double* im_it;         // [B]     it_time_
  double* im_last;       // [B][16] Sensor::last_pose_, column-major
  double* im_meas;       // [B][6]  Tracking::measurements_ (SetMeasurements): gyro xyz, accelerometer xyz
  // Sim3Solver (track_sim3.hip) on the SearchByPoints pairing: KF1 = the cur slot (pose Tcur), KF2 = the ref slot (pose Tref),
  // matches = sp_match, validity = sp_valid1 / sp_valid2
  double* s3_Xw1;        // [B][kp_cap][3] GetWorldPos() of KF1's map points, by KF1 keypoint index (sd_track_set_sim3_points)
  double* s3_Xw2;        // [B][kp_cap][3] the same for KF2
  // the constructor's gather, in mvnIndices1 order (structure of arrays, stride kp_cap)
  double* s3_X;          // [B][6][kp_cap] mvX3Dc1 xyz | mvX3Dc2 xyz
  float* s3_F;           // [B][6][kp_cap] mvP1im1 uv | mvP2im2 uv (float values, see FromCameraToImage) | mvnMaxError1 | mvnMaxError2
  uint16_t* s3_idx;      // [B][kp_cap] mvnIndices1
  // Sim3Solver members that persist between iterate() calls
  int32_t* s3_state;     // [B][8]: mnIterations, mnBestInliers, N, mRansacMaxIts, mRansacMinInliers, mbFixScale, 0, 0
  unsigned long long* s3_best_mask;   // [B][32] mvbBestInliers as bits over the gathered correspondences
  double* s3_bestT;      // [B][16] mBestT12, column-major
  double* s3_R;          // [B][9]  mBestRotation, column-major
  double* s3_t;          // [B][3]  mBestTranslation
  double* s3_s;          // [B]     mBestScale (a float value)
  // iterate() outputs
  double* s3_T;          // [B][16] the returned matrix, column-major (zeros: none)
  uint8_t* s3_inliers;   // [B][kp_cap] vbInliers, over KF1 keypoints
  int32_t* s3_info;      // [B][8]: returned, nInliers, bNoMore, mnIterations, N, mRansacMaxIts, mnBestInliers, 0
};

// Entry (r, c) of the 4x4 product A * B, both column-major: k = 0..3 in order, every product and sum rounded on its own (no
// FMA contraction), as a plain host loop does.  The one product behind every prior: k_set_prior (T * Tref) and
// k_motion_predict (Exp(X) * Tref) must agree bit for bit.
__device__ __forceinline__ double pose_product_entry(const double* __restrict__ A, const double* __restrict__ B, int r, int c) {
  double v = __dmul_rn(A[r], B[c * 4]);
#pragma unroll
  for (int k = 1; k < 4; k++) v = __dadd_rn(v, __dmul_rn(A[k * 4 + r], B[c * 4 + k]));
  return v;
}

// (x0 * y0 + x1 * y1) + x2 * y2, every product and sum rounded on its own: the 3-vector product of track_tri.hip and
// track_newpoints_tri.hip
__device__ __forceinline__ double dot3(double x0, double x1, double x2, double y0, double y1, double y2) {
  return __dadd_rn(__dadd_rn(__dmul_rn(x0, y0), __dmul_rn(x1, y1)), __dmul_rn(x2, y2));
}

// KeyFrame::GetCameraCenter, Ow = -Rcw^T * tcw, of a pose T (column-major, Rcw[r][c] = T[c * 4 + r], tcw = T[12..14]):
// Ow[r] = -dot3(Rwc row r, tcw).  The one statement of it: k_triangulate / k_new_points_resolve (fill_pose) and
// k_refresh_centres must agree bit for bit, and tests/new_points_ref.py restates this order.
__device__ __forceinline__ double camera_centre(const double* __restrict__ T, int r) {
  return -dot3(T[r * 4], T[r * 4 + 1], T[r * 4 + 2], T[12], T[13], T[14]);
}

// The map point mvpMapPoints[i] = m keeps after Tracking::Track's "Clean VO matches" (Observations() >= 1, reference
// src/Tracking.cc:250-257) and outlier discard (:272-275): source 0 = cur_match after TrackWithMotionModel's discard (no
// outlier flags left), 1 = un_match after TrackLocalMap, m >= M naming local point m - M, outl_i = &mvbOutlier[i].
// Returns its Observations() if it is kept, else 0; *e / *loc locate it.  o = slot * M.  k_advance keeps these points and
// k_close_points counts them as tracked: one test for both.  with_outliers: the state BEFORE the outlier discard, which
// CreateNewKeyFrame sees (:861-867 run between :257 and :272) -- a flagged point with Observations() >= 1 is still there.
__device__ __forceinline__ int kept_point_obs(const TrackBuffers& tb, int source, int m, const uint8_t* outl_i, size_t o, size_t* e,
                                              bool* loc, bool with_outliers = false) {
  if (m < 0 || (source == 1 && !with_outliers && *outl_i)) return 0;
  *loc = m >= tb.max_points;
  *e = o + (*loc ? m - tb.max_points : m);
  const int n_obs = *loc ? tb.lm_obs[*e] : tb.obs[*e];
  return n_obs >= 1 ? n_obs : 0;
}

// Whether the tracking call `source` left slot f tracked: -1 every slot counts, 0 tw_info status 2, 1 tl_info status 2
__device__ __forceinline__ bool slot_tracked(const TrackBuffers& tb, int source, int f) {
  if (source == 0) return tb.tw_info[(size_t)f * 4] == 2;
  if (source == 1) return tb.tl_info[(size_t)f * 4] == 2;
  return true;
}

struct TrackCam {
  double fx, fy, cx, cy;                 // (double)(float) like ImageAlign::cam_fx_
  float ffx, ffy, fcx, fcy;              // Frame::fx ... (static floats)
  float min_x, max_x, min_y, max_y;      // Frame::mnMinX ...
  float bf, mb;                          // Frame::mbf, mb = mbf / fx
};
static inline TrackCam make_cam(float fx, float fy, float cx, float cy, float bf, float min_x, float max_x, float min_y, float max_y) {
  return TrackCam{fx, fy, cx, cy, fx, fy, cx, cy, min_x, max_x, min_y, max_y, bf, bf / fx};
}

struct PnpParams {
  double probability;
  int min_inliers, max_iterations, min_set;
  float epsilon, th2;
  int n_iterations;     // argument of iterate()
  int rand_per_frame;   // entries of rand_stream per frame
  int resume;           // 0: freshly constructed solver; 1: a further iterate() on the state the last call left
};

int launch_align(const sd_orb* cur, const sd_orb* ref, const TrackBuffers& tb, const TrackCam& cam, const float* d_inv_sf,
                 const float* d_sf, int n_frames, int mode, hipStream_t s);
// retry_below > 0: only frames whose last search found fewer matches run, from the PRIOR pose (which becomes the frame's pose)
int launch_match(const sd_orb* cur, const TrackBuffers& tb, const TrackCam& cam, const float* d_sf, int n_frames, float th,
                 int mono, int check_ori, hipStream_t s, int retry_below = 0, int note_below = 0);
// min_matches > 0: the tail of Tracking::TrackWithMotionModel around PoseOptimization (gate, outlier discard, tw_info)
// source 2 (+ min_inliers): TrackLocalMap -- the union of both match vectors, mnMatchesInliers, tl_info
int launch_pose_opt(const sd_orb* cur, const TrackBuffers& tb, const TrackCam& cam, const float* d_inv_sigma2, int source, int n_frames,
                    hipStream_t s, int min_matches = 0, int min_inliers = 0);
// claim_from_matches: "keypoint already holds a point with Observations() > 0" is read off the frame-to-frame matches
// (tb.cur_match / tb.obs) instead of the caller's lm_kclaim flags
// exclude_seen: a local point whose id (lm_id) equals the id of a last-frame point in tw_seen is no candidate
int launch_match_local(const sd_orb* cur, const TrackBuffers& tb, const TrackCam& cam, const float* d_sf, const float* d_scale_thr,
                       int nlevels, int n_frames, float th, float nnratio, float cos_limit, hipStream_t s, int claim_from_matches = 0,
                       int frustum_given = 0, int exclude_seen = 0);
int launch_features_in_area(const sd_orb* cur, const TrackBuffers& tb, const TrackCam& cam, int frame, float x, float y, float r,
                            int min_level, int max_level, int32_t* d_out, int out_cap, int32_t* d_n, int32_t* d_grid, hipStream_t s);
int launch_search_points(const sd_orb* cur, const sd_orb* ref, const TrackBuffers& tb, int n_frames, float nnratio, int check_ori,
                         hipStream_t s);
// ComputeF12 (use_set_f12: tri_F12_set instead) and the epipole of every slot, then SearchForTriangulation (track_tri.hip)
int launch_tri(const sd_orb* cur, const sd_orb* ref, const TrackBuffers& tb, const TrackCam& cam, const float* d_sf, const float* d_sigma2,
               int n_frames, int use_set_f12, int check_ori, hipStream_t s);
// ORBmatcher::Fuse (track_fuse.hip): what the search owns besides the local-map point rows (lm_*) it reads.  Kept out of
// TrackBuffers, which travels by value with every other kernel.
struct FuseBuffers {
  double* Scw;           // [B][16] the caller's Scw, column-major (sd_track_set_fuse_scw)
  double* pose;          // [B][15] what the last search projected with: Rcw row-major | tcw | Ow
  int32_t* idx;          // [B][M]  best_idx
  int32_t* dist;         // [B][M]  best_dist
  int32_t* n;            // [B]     points with best_idx >= 0
};
// kf_side 0: KF = the slot's cur frame (or the broadcast frame), Tcur, tb.uright; 1: frame f of `ref`, Tref, tb.uright_ref
int launch_fuse(const sd_orb* cur, const sd_orb* ref, const TrackBuffers& tb, const FuseBuffers& fb, const TrackCam& cam, const float* d_sf,
                const float* d_inv_sigma2, const float* d_scale_thr, int n_frames, int kf_side, int point_row, float th, int sim3,
                hipStream_t s);
// LocalMapping::CreateNewMapPoints after the search (track_newpoints_tri.hip): what triangulation owns besides the search's
// result (tb.tri_match), the pairing's keypoints, mvuRight rows and poses it reads.  Kept out of TrackBuffers like FuseBuffers.
struct TriangBuffers {
  float* depth_ref;      // [B][kp_cap] mvDepth of the ref extractor's frames (the cur side's is tb.depth)
  float* median;         // [B]   ComputeSceneMedianDepth(2) of KF2; negative: the slot's baseline gate is off
  uint8_t* verdict;      // [B][kp_cap] 0 no match, 1 accepted, 2.. the gate that rejected (SD_TRI_* of sdslam_hip.h)
  uint8_t* branch;       // [B][kp_cap] 0 none, 1 linear triangulation, 2 UnprojectStereo(idx1), 3 UnprojectStereo(idx2)
  double* Xw;            // [B][kp_cap][3] x3D of every row that chose a branch
  int32_t* count;        // [B][2] rows with verdict 1 | rows that became a point of this slot
  // the new points in (slot, idx1) order, B * kp_cap rows
  int32_t* info;         // [4]: points, the broadcast setting, slots, MapPoint::nNextId after the last one
  int32_t* pt;           // [..][4] KF1 keypoint | the neighbour (slot) that triangulated it | KF2 keypoint | id
  double* geo;           // [..][6] Xw | mNormalVector
  float* dist;           // [..][2] mfMaxDistance | mfMinDistance
  uint8_t* desc;         // [..][32] GetDescriptor()
  int32_t* appended;     // [B][3] the last sd_track_append_new_points, per local row: base | appended | dropped (track_append.hip)
};
// k_triangulate on the live search result of slots < n_frames, then k_new_points_resolve.  ratio_factor = 1.5f * mfScaleFactor
int launch_triangulate(const sd_orb* cur, const sd_orb* ref, const TrackBuffers& tb, const TriangBuffers& nb, const TrackCam& cam,
                       const float* d_sf, const float* d_sigma2, float ratio_factor, int n_frames, int monocular, hipStream_t s);
// k_append_points, then k_append_commit (track_append.hip): the points of the resolve result behind the points of local row
// point_row (>= 0, cand of rows < n_cand_rows) or of each point's own slot's row (-1); mark_flags: sp_valid1 / sp_valid2 too
int launch_append_points(const TrackBuffers& tb, const TriangBuffers& nb, int max_batch, int point_row, int n_cand_rows, int mark_flags,
                         hipStream_t s);
// MapPoint::ComputeDistinctiveDescriptors + UpdateNormalAndDepth (track_refresh.hip): what the refresh owns besides the point
// row (lm_*) it reads and, with write_local, rewrites.  Kept out of TrackBuffers like FuseBuffers.
struct RefreshBuffers {
  // The observation lists of the last sd_track_set_observations: ONE device block and its pinned mirror, packed per call as
  // obs_off | ref_obs | obs_frame | obs_kp | point_bad | obs_kf_bad.  Allocated by sd_track_create for max_points points of 16
  // observations each; sd_track_set_observations replaces both by larger ones (after a wait for the tracking stream) when a call
  // needs more, and never shrinks them.  Nothing is allocated in sd_track_refresh_points.
  uint8_t* obs;          // device
  uint8_t* twin;         // device, as large as obs: sd_track_erase_observations compacts the lists into it and swaps the two
  uint8_t* stage;        // pinned host
  size_t obs_bytes;      // capacity of each
  hipEvent_t ev_staged;  // the copy out of `stage` has run
  bool staged;
  size_t o_off, o_ref, o_frame, o_kp, o_pbad, o_kbad;   // byte offsets of the arrays of the last upload; o_pbad / o_kbad 0: NULL
  size_t at_pbad, at_kbad;   // where the block keeps room for the two flag arrays, given or not
  int n_points;          // -1: no observations have been set
  int n_obs;             // entries the block was packed for; after an erase an upper bound, the lists end at obs_off[n_points]
  unsigned long long serial;   // counts the uploads and erasures: what ran on the lists is stamped with it
  int max_ref_frame;     // largest obs_frame of the last upload (-1: none)
  bool has_cur;          // an observation names the current keyframe (-1)
  double* centre;        // [B + 1][3] camera centres of the ref frames (Tref), then of the current keyframe (Tcur of slot 0)
  // results, one entry per point of the list
  uint8_t* status;       // [M] SD_REFRESH_* bits
  int32_t* best_obs;     // [M] BestIdx as a position in the caller's list
  int32_t* best_median;  // [M]
  uint8_t* desc;         // [M][32]
  double* normal;        // [M][3]
  float* max_dist;       // [M] mfMaxDistance
  float* min_dist;       // [M] mfMinDistance
};
// k_refresh_centres, then k_refresh_points on the points of row `point_row`; write_local: the results also go into that row
int launch_refresh(const sd_orb* cur, const sd_orb* ref, const TrackBuffers& tb, const RefreshBuffers& rf, const float* d_sf, int n_batch,
                   int point_row, int write_local, hipStream_t s);
// LocalMapping::KeyFrameCulling and the erasure of observations (track_cull.hip): ONE device allocation carved by cull_carve for
// cap_points points, cap_obs observations and n_cand candidates.  sd_track_create allocates it beside the bundle adjustment's
// scratch and sd_track_set_observations grows it with its own block.  Nothing is allocated in either call.
struct CullBuffers {
  uint8_t* base;
  size_t bytes, cap_points, cap_obs;
  // what k_cull_gather makes of the resident lists, per observation: its camera (ref frame, max_batch = the current keyframe),
  // octave, mvDepth (ref side) and weight in nObs (2: mvuRight >= 0); per point the refusal bits of its entries
  int32_t* e_kf;
  int32_t* e_oct;
  float* e_depth;
  uint8_t* e_w;
  uint8_t* p_flag;
  int32_t* cand;         // [2 n_cand] the candidates' frames, then their flags
  // the last cull
  uint8_t* verdict;      // [n_cand]
  int32_t* counts2;      // [n_cand][2]
  uint8_t* dead;         // [E]
  uint8_t* pbad;         // [P] went bad in the run
  int32_t* ref_new;      // [P]
  int32_t* nobs;         // [P]
  int32_t* info;         // [8]
  // the last erasure
  int32_t* er_map;       // [E] old entry -> new position, -1: erased
  int32_t* er_nobs;      // [P]
  int32_t* er_cnt;       // [P] survivors
  int32_t* er_info;      // [8]
  int ran_cand, ran_points, ran_obs;   // the last cull: ran_cand -1: none
  unsigned long long ran_serial;       // ... and the lists it ran on
  int er_points, er_obs;               // the last erasure: er_points -1: none
  unsigned long long er_serial;        // ... and the lists it left
};
// Optimizer::LocalBundleAdjustment (track_ba.hip): the scratch of one problem, ONE device allocation carved by ba_carve for
// cap_points points, cap_obs observations and n_kf cameras.  sd_track_create allocates it for max_points points of 16
// observations each and max_batch + 1 cameras (the ref frames, then the current keyframe); sd_track_set_observations replaces
// it by a larger one where it grows its own block.  Nothing is allocated in sd_track_local_ba.
struct BaState;
struct BaBuffers {
  uint8_t* base;         // the allocation (the handle's; a debug entry carves its own)
  size_t bytes, cap_points, cap_obs;
  int n_kf;
  int ran_points, ran_obs;   // what sd_track_get_local_ba downloads: the lists of the last run; ran_points -1: none
  int ran_global;        // that run was sd_track_global_ba's: each getter answers its own kind only
  int kcap;              // the free cameras it holds: >= SD_BA_MAX_FREE_KF; the handle's min(SD_GBA_MAX_FREE_KF, n_kf) if that is more
  double* W;             // [6 kcap + 1][48] the blocked factorisation's current panel, L D (kcap > SD_BA_MAX_FREE_KF)
  uint32_t* covis;       // [kcap][ceil(kcap / 32)] bit j of row i < j: free cameras i and j see a common point (global BA)
  BaState* st;           // the device state record: status, the Levenberg bookkeeping, info16
  // per edge (= observation, CSR order)
  double* e_meas;        // [E][3] u, v, ur (0 for a monocular edge)
  double* e_info;        // [E]    mvInvLevelSigma2[octave]
  double* err;           // [E][3] _error of the last computeActiveErrors that covered the edge
  double* chi2r;         // [E]    its term of activeRobustChi2
  double* Jl;            // [E][3][3] _jacobianOplusXi
  double* Jp;            // [E][3][6] _jacobianOplusXj
  double* wr;            // [E][3] omega_r
  double* w;             // [E]    rho[1] * information
  int32_t* e_cam;        // [E]
  int32_t* e_pt;         // [E]
  uint8_t* e_flag;       // [E] BA_LIVE | BA_STEREO | BA_LEVEL1 | the refusal bits
  uint8_t* erase;        // [E] obs_erase
  // per point
  double* Hll;           // [P][9]
  double* bl;            // [P][3]
  double* X;             // [2][P][3] the two estimate buffers
  double* X_out;         // [P][3]
  uint8_t* p_active;     // [P] has a level-0 edge in this round
  uint8_t* p_status;     // [P] SD_BA_POINT_*
  double* v_scale;       // [n_kf + P] every vertex's terms of computeScale
  // per camera
  double* pose;          // [2][n_kf][8] SE3Quat q (x y z w), t, 0
  double* T_out;         // [n_kf][16]
  int32_t* slot;         // [n_kf] number among the free cameras, -1: fixed
  uint8_t* role;         // [n_kf]
  uint8_t* c_has;        // [n_kf] some edge observes it
  uint8_t* c_act;        // [n_kf] free, with a level-0 edge in this round
  // per free camera
  double* Hpp;           // [K][36]
  double* bp;            // [K][6]
  int32_t* slot_cam;     // [K]
  int32_t* coff;         // [K + 1] its edges in clist
  int32_t* clist;        // [E]
  // the reduced system
  double* S;             // packed lower triangle of the (6K)^2 matrix, and one more row for the blocked solver's right-hand side
  double* bs;            // [6K]
  double* xp;            // [6K]
};
int launch_stereo_from_depth(const sd_orb* cur, const TrackBuffers& tb, const TrackCam& cam, const float* d_depth, int w, int h,
                             int stride_elems, size_t frame_stride_elems, int n_frames, hipStream_t s);
// the same on a depth map of uint16_t (u16 != 0, always converted) or float elements; convert: d = (float)raw * scale
int launch_stereo_from_depth_typed(const sd_orb* cur, const TrackBuffers& tb, const TrackCam& cam, const void* d_depth, int u16,
                                   int convert, float scale, int w, int h, int stride_elems, size_t frame_stride_elems, int n_frames,
                                   hipStream_t s);
// map point creation and the keyframe decision (track_newpoints.hip).  mode 1: CreateNewKeyFrame on the result of the
// tracking call `source`; 2: StereoInitialization.  inv_fx / inv_fy = Frame::invfx / invfy.
int launch_new_points(const sd_orb* cur, const TrackBuffers& tb, const TrackCam& cam, float inv_fx, float inv_fy, int n_frames, int mode,
                      int source, float th_depth, int use_flags, int frame_id, int min_keypoints, hipStream_t s);
int launch_need_keyframe(const TrackBuffers& tb, const int32_t* d_close, int n_frames, int rgbd, int frame_id, int min_frames,
                         int max_frames, hipStream_t s);
// entries of `staged` ([n][8]) equal to INT32_MIN leave the device's value
int launch_set_keyframe_state(const TrackBuffers& tb, const int32_t* staged, int frame0, int n_frames, hipStream_t s);
// motion model (track_motion.hip).  source -1: every slot < n counts as tracked; 0 / 1: tw_info / tl_info status 2
int launch_motion_init(const TrackBuffers& tb, int frame0, int n_frames, hipStream_t s);   // EKF::Restart
int launch_motion_predict(const TrackBuffers& tb, int n_frames, double dt, hipStream_t s);
int launch_motion_update(const TrackBuffers& tb, int n_frames, int source, hipStream_t s);
// IMU sensor model (track_imu.hip), one wave per slot; source as above
// full 0: EKF::Restart (IMU::Init: the diagonal blocks of P only); 1: a newly constructed EKF (all of P)
int launch_imu_init(const TrackBuffers& tb, int frame0, int n_frames, int full, hipStream_t s);
int launch_imu_predict(const TrackBuffers& tb, int n_frames, double dt, hipStream_t s);
int launch_imu_update(const TrackBuffers& tb, int n_frames, int source, hipStream_t s);
int read_pnp_prof(unsigned long long* out32, int reset);
int read_sel_prof(unsigned long long* out64, int reset);
int read_align_prof(unsigned long long* out16, int reset);
int launch_pnp(const sd_orb* cur, const TrackBuffers& tb, const TrackCam& cam, const float* d_sigma2, const PnpParams& pp,
               int n_frames, hipStream_t s);

struct Sim3Params {
  int fix_scale, min_inliers;
  int n_iterations;     // argument of iterate()
  int rand_per_frame;   // entries of rand_stream per slot
  int resume;           // 0: construct (gather, SetRansacParameters) and iterate; 1: a further iterate() on the saved state
};
// d_max_its[N], N = 0..kp_cap: mRansacMaxIts for N correspondences (host libm, see sd_track_sim3); read only when !resume
int launch_sim3(const sd_orb* cur, const sd_orb* ref, const TrackBuffers& tb, const TrackCam& cam, const float* d_sigma2,
                const int32_t* d_max_its, const Sim3Params& sp, int n_frames, hipStream_t s);

int run_epnp_debug(int n, const double* Xw, const double* uv, double fx, double fy, double cx, double cy, double* R9, double* t3,
                   double* err);

}  // namespace sd
