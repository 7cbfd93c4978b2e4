/* sdslam_hip.h -- C ABI of libsdslam_hip.so: the MI355X (gfx950) implementation of SD-SLAM's
 * per-frame tracking hot path.  Plain pointers and sizes only; every entry point returns an
 * int32 status (SD_OK = 0) and never throws.  Opaque handles own device memory and one HIP
 * stream; calls on one handle are serialised by the caller, different handles are independent
 * (re-entrancy contract of SURVEY.md §8b: Tracking thread + LoopClosing thread).
 *
 * Each group cites the reference C++ interface it replaces (paths relative to the reference
 * repository pasensio97/SDslam); INTEGRATION.md shows the reference-side binding.
 */
#ifndef SDSLAM_HIP_H_
#define SDSLAM_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SD_OK 0
#define SD_ERR_INVALID_ARG 1  /* bad pointer/size/shape                                   */
#define SD_ERR_HIP 2          /* a HIP runtime call failed (see sd_last_error)             */
#define SD_ERR_CAPACITY 3     /* caller buffer / handle capacity too small                  */
#define SD_ERR_NO_DEVICE 4    /* no gfx950 device visible                                   */
#define SD_FALSE 100          /* the reference would have returned `false` / an empty Mat   */

const char* sd_last_error(void);      /* thread-local description of the last failure      */
int sd_device_count(void);            /* number of visible HIP devices (0 on a CPU box)    */
const char* sd_version(void);

/* Process-wide options: the library's tuning and test switches.  The library never reads the environment.  Integer values;
 * unknown names and out-of-range values fail with SD_ERR_INVALID_ARG.  "plan" options are read when a handle (re)builds its
 * geometry (first extraction at a new frame size), "create" options when a handle is created, the others at every call.
 *   extract.fast0_from_frames  1     0: FAST of level 0 reads the padded pyramid copy instead of the caller's frames
 *   extract.use_graph          0     1: replay the extraction pipeline as a captured hipGraph (slower on ROCm 7.2; kept for tests)
 *   extract.select_small_cap   0     >0: cap (entries) of the per-cell selection buffer -- tests force the large-cell paths
 *   extract.select_big_cap     0     >0: cap of the per-level selection buffer -- tests force the serial fallback
 *   extract.fast_merge_from    6     plan: first pyramid level of the merged FAST launch (>= nlevels: one launch per level)
 *   extract.fast_lds_kb        24    plan: LDS budget of a FAST strip
 *   extract.fast_lds_whole_kb  40    plan: LDS budget under which a cell of the unmerged levels is processed as one strip
 *   track.stream_priority      2     create: priority of the tracking stream, 0 lowest / 1 normal / 2 highest
 *   track.align_start          2     ImageAlign of a batch may start 0: after its whole extraction, 1: after its pyramid,
 *                                    2: after its pyramid and FAST launches (beside selection + descriptors)
 *   track.align_min_waves      5     register budget of k_align in waves per SIMD (3, 4, 5)
 *   track.bf_list_k            4     SearchByPoints: keys kept per point, 1..4 -- tests force the whole-row recomputation
 *   track.poseopt_waves        0     k_pose_opt waves per frame: 0 = by batch size (4 up to 256 frames, else 1), 1, 4
 *   track.match_split          1     SearchByProjection(Frame, Frame / KeyFrame) as candidate + one-wave assignment kernels
 *                                    (6 KB of LDS per frame through the serial part); 0: the single 39-KB kernel
 *   extract.fast0_early        1     device-input extractions on the handle's own stream: FAST of level 0 starts behind the PREVIOUS
 *                                    call's selection (beside its descriptor kernel) instead of behind the whole previous call; 0: as before
 *   extract.pyr_early          0     1: ... and, on an extractor with two output sets (one a tracker is attached to), the resize chain as
 *                                    well, on the auxiliary stream in front of the blur (measured: loses 8 % with the PnP step)
 *   extract.pyr_rows           1     plan: levels resized by k_pyr_rows (runs of consecutive rows that share source rows): 0 none,
 *                                    1 the levels whose runs fill four fifths of the row blocks (scale 1.2), 2 every level tall
 *                                    enough for single-reflection borders -- tests force short runs through the kernel
 * Results never depend on an option (each setting is covered by a parity test); only speed does. */
int sd_set_option(const char* name, int value);
int sd_get_option(const char* name, int* value);
int sd_option_count(void);
const char* sd_option_name(int index);

/* cv::KeyPoint, 28 bytes: {pt.x, pt.y, size, angle, response, octave, class_id} */
typedef struct sd_keypoint {
  float x, y, size, angle, response;
  int32_t octave, class_id;
} sd_keypoint;

/* ------------------------------------------------------------------------------------------
 * ORB extractor -- replaces SD_SLAM::ORBextractor
 *   ctor            src/ORBextractor.h:38,   src/ORBextractor.cc:406-457
 *   operator()      src/ORBextractor.h:45-46, src/ORBextractor.cc:620-678
 *   Get*()          src/ORBextractor.h:48-70
 * One handle serves frames up to max_w x max_h, at most max_batch frames per call.
 * A geometry the kernels do not cover is refused with SD_ERR_INVALID_ARG and a message (sd_last_error, "unsupported geometry: ..."): image
 * sides beyond 4095, a pyramid level that collapses to zero size, a grid cell whose FAST zone is one pixel wide (frames a few dozen
 * pixels wide with hundreds of features per level).
 * ------------------------------------------------------------------------------------------ */
typedef struct sd_orb sd_orb;

int sd_orb_create(int nfeatures, float scale_factor, int nlevels, int th_fast,
                  int max_w, int max_h, int max_batch, int device, sd_orb** out);
void sd_orb_destroy(sd_orb* h);

/* GetLevels / GetScaleFactors / GetInverseScaleFactors / GetScaleSigmaSquares /
 * GetInverseScaleSigmaSquares (arrays of nlevels floats; any pointer may be NULL). */
int sd_orb_levels(const sd_orb* h);
int sd_orb_scale_tables(const sd_orb* h, float* sf, float* inv_sf, float* sigma2, float* inv_sigma2);
int sd_orb_features_per_level(const sd_orb* h, int32_t* quota);

/* Host-only geometry query (works without a GPU): per level {w, h, quota, levelCols, levelRows,
 * cellW, cellH, nfeaturesCell} (src/ORBextractor.cc:472-488,683) and per cell {level, zone x0,
 * y0, w, h, evaluated} (the FAST detection zone of src/ORBextractor.cc:501-536). */
int sd_orb_plan_info(int nfeatures, float scale_factor, int nlevels, int th_fast, int w, int hgt,
                     int32_t* level_info /* nlevels x 8 */, int32_t* cell_zones /* cap x 6, may be NULL */,
                     int cell_cap, int32_t* n_cells, uint64_t* bytes_per_frame);

/* Host-only: how pyramid level `level` of that geometry is resized under the current "extract.pyr_rows".  *n_blocks = 0: by
 * k_pyr_split (rows a quarter of the level apart).  Otherwise by k_pyr_rows, and per row block {first interior row y0, rows n
 * (1..5), first source row, 1 if a row of the block is stored a second time as a REFLECT_101 border row}: rows y0 .. y0 + n - 1
 * resize source rows sy0 + r and sy0 + r + 1. */
int sd_orb_plan_row_blocks(int nfeatures, float scale_factor, int nlevels, int th_fast, int w, int hgt, int level,
                           int32_t* blocks /* cap x 4, may be NULL */, int block_cap, int32_t* n_blocks);

/* operator()(image, mask(ignored), keypoints, descriptors, pyramid): one 8-bit grey frame in
 * host memory -> keypoints (cap entries), descriptors (cap x 32 bytes), *n_out.  The image
 * pyramid stays resident on the device (sd_orb_level_*).  Empty image => *n_out = 0, SD_OK
 * (src/ORBextractor.cc:622-623). */
int sd_orb_extract(sd_orb* h, const uint8_t* img, int w, int hgt, int stride,
                   sd_keypoint* kps_out, uint8_t* desc_out, int cap, int* n_out);

/* Batched-frames mode: n_frames independent frames of identical size.
 * Host variant copies in/out; device variant takes a device pointer, launches asynchronously
 * on the handle's stream and leaves the results resident (read them with sd_orb_download or
 * chain into sd_match_ / sd_align_ calls on the same handle).
 * When the device variant may read d_imgs: on the handle's own stream, only what was complete
 * when the call was made (a producer the host has synchronised with) or what a stream fenced
 * with sd_orb_stream_fence(h, stream, 1) before the call has queued -- the extraction may start
 * on other streams of the handle ahead of the own stream (extract.fast0_early, extract.pyr_early).
 * On a caller's stream (sd_orb_set_stream) everything queued on that stream before the call, in
 * stream order.  The frames may be overwritten once the host has synchronised with the handle
 * (sd_orb_sync, sd_orb_download) or behind sd_orb_stream_fence(h, stream, 0). */
int sd_orb_extract_batch(sd_orb* h, const uint8_t* imgs, int n_frames, int w, int hgt, int stride,
                         size_t frame_stride, sd_keypoint* kps_out, uint8_t* desc_out,
                         int cap_per_frame, int32_t* n_out);
int sd_orb_extract_batch_device(sd_orb* h, const void* d_imgs, int n_frames, int w, int hgt,
                                int stride, size_t frame_stride);
int sd_orb_download(sd_orb* h, int frame0, int n_frames, sd_keypoint* kps_out, uint8_t* desc_out,
                    int cap_per_frame, int32_t* n_out);

/* Frame::UndistortKeyPoints (src/Frame.cc:335-366): with k1 != 0 every extraction also produces
 * mvKeysUn = cv::undistortPoints(mvKeys, K, {k1,k2,p1,p2,k3}, R=I, P=K); the tracking stages read
 * the undistorted keypoints.  K is the CV_32F camera matrix Converter::toCvMat builds. */
int sd_orb_set_distortion(sd_orb* h, float fx, float fy, float cx, float cy, float k1, float k2,
                          float p1, float p2, float k3);
int sd_orb_download_undistorted(sd_orb* h, int frame0, int n_frames, sd_keypoint* kps_un_out,
                                int cap_per_frame);

/* std::vector<cv::Mat>& imagePyramid of operator(): level geometry and a host copy of one
 * level of one frame of the last batch (padded != 0: including the 19-px REFLECT_101 border
 * the reference keeps around each level, src/ORBextractor.cc:684-697). */
int sd_orb_level_info(const sd_orb* h, int level, int* w, int* hgt);
int sd_orb_level_copy(sd_orb* h, int frame, int level, int padded, uint8_t* out, int out_stride);

/* Diagnostics used by the parity tests (stage outputs of the last batch). */
int sd_orb_debug_blurred(sd_orb* h, int frame, int level, uint8_t* out, int out_stride);
int sd_orb_debug_cell_counts(sd_orb* h, int frame, int level, int32_t* out, int cap, int* n_cells);
int sd_orb_debug_level_keys(sd_orb* h, int frame, int level, uint32_t* keys_out, int cap, int* n);
/* Plants the caller's keypoints and descriptors in frames frame0 .. frame0 + n_frames - 1 of the current output set, where an
 * extraction would have left them: n[f] keypoints from row f of kps / desc (rows of `cap` entries).  Host code only -- copies
 * on the handle's stream, which the call waits for.  To a tracker it is an extraction into those slots: the results it holds
 * from before are refused afterwards.  The frames of the set that the call does not name keep what they hold; the pyramid is
 * not touched.  Refused: a handle that has not extracted yet (no geometry), a distortion with k1 != 0 (mvKeysUn would be a
 * second array), n[f] above the keypoint capacity or `cap`, frame0 + n_frames above max_batch. */
int sd_debug_orb_set_keypoints(sd_orb* h, int frame0, int n_frames, const int32_t* n, const sd_keypoint* kps,
                               const uint8_t* desc, int cap);

/* Stream / timing plumbing (bench + rocprof).  sd_orb_set_stream: run on a caller-owned
 * hipStream_t (NULL restores the handle's own stream); it first waits for the work queued on the
 * previous stream.  On a caller's stream every extraction starts behind everything queued on that
 * stream before the call (the early level-0 FAST launch is the own stream's alone).  With profiling on, every extract call
 * brackets each stage with HIP events on the launch stream; sd_orb_stage_ms returns the mean
 * elapsed ms per stage over the calls made since profiling was switched on (last 128 at most;
 * names from sd_orb_stage_name). */
int sd_orb_set_stream(sd_orb* h, void* hip_stream);
/* Ordering against a caller-owned hipStream_t (e.g. the stream that uploads the NEXT batch's frames while this batch is being
 * processed): direction 0 = that stream waits for the extractions queued so far (their input frames may then be overwritten),
 * 1 = the extractions queued from now on -- on all of the handle's streams -- wait for everything queued on that stream so far
 * (the upload of their frames).  Every fence holds: fences on several streams order the extractions behind all of them. */
int sd_orb_stream_fence(sd_orb* h, void* hip_stream, int direction);
int sd_orb_sync(sd_orb* h);
int sd_orb_set_profiling(sd_orb* h, int on);
int sd_orb_num_stages(void);
const char* sd_orb_stage_name(int stage);
int sd_orb_stage_ms(sd_orb* h, float* ms_out, int cap);
/* algorithmic bytes per frame of each stage for the current geometry */
int sd_orb_stage_bytes(const sd_orb* h, double* bytes_out, int cap);

/* device memory helpers for harnesses that have no HIP binding of their own */
int sd_dev_alloc(size_t bytes, void** out);
/* page-locked host buffers (hipHostMalloc): frames handed to sd_orb_extract / sd_orb_extract_batch from such a buffer
 * are copied at the PCIe rate instead of through the driver's pageable-memory staging */
int sd_host_alloc(size_t bytes, void** out);
int sd_host_free(void* p);
int sd_dev_free(void* p);
int sd_dev_upload(void* dst, const void* src, size_t bytes);
int sd_dev_download(void* dst, const void* src, size_t bytes);

/* ------------------------------------------------------------------------------------------
 * Batched TrackWithMotionModel context -- the per-frame sequence of src/Tracking.cc:654-718
 * over two resident extractor handles: `cur` holds the current frames of the batch, `ref` the
 * last frames (same geometry, frame f of one pairs with frame f of the other).
 *
 *   sd_track_align   ImageAlign::ComputePose            src/ImageAlign.h:36-42, src/ImageAlign.cc:45-232
 *                    mode 0 (Frame,Frame) / 1 (Frame,KeyFrame) / 2 (Frame,KeyFrame,fast) / 3 (KF,KF)
 *   sd_track_match   ORBmatcher::SearchByProjection(Frame&, const Frame&, th, bMono)
 *                                                       src/ORBmatcher.h:46, src/ORBmatcher.cc:946-1075
 *                    (+ Frame::AssignFeaturesToGrid / GetFeaturesInArea, src/Frame.cc:179-192,271-332)
 *   sd_track_pnp     PnPsolver ctor + SetRansacParameters + iterate
 *                                                       src/PnPsolver.h:67-76, src/PnPsolver.cc:71-315
 *
 * Last-frame data (sd_track_set_last) flattens LastFrame.mvpMapPoints: for last-frame keypoint
 * i, valid[i] = (pMP != NULL && !mvbOutlier[i]), Xw = pMP->GetWorldPos(), desc =
 * pMP->GetDescriptor(), octave = mvKeys[i].octave, angle = mvKeysUn[i].angle, obs =
 * pMP->Observations().  Arrays are [n_frames][max_points(...)] in host memory.  Poses are 16
 * doubles column-major (Eigen::Matrix4d::data()).  All launches are asynchronous on the `cur`
 * extractor's stream; the sd_track_get_* calls synchronise.
 * ------------------------------------------------------------------------------------------ */
typedef struct sd_track sd_track;

int sd_track_create(sd_orb* cur, sd_orb* ref, int max_points, int max_batch, int pnp_max_iterations,
                    sd_track** out);
void sd_track_destroy(sd_track* h);
/* Frame statics: fx, fy, cx, cy, mbf, mnMinX, mnMaxX, mnMinY, mnMaxY (src/Frame.cc:158-174) */
int sd_track_set_camera(sd_track* h, float fx, float fy, float cx, float cy, float bf,
                        float min_x, float max_x, float min_y, float max_y);
int sd_track_set_last(sd_track* h, int frame0, int n_frames, const int32_t* n_last,
                      const uint8_t* valid, const double* Xw, const uint8_t* desc,
                      const int32_t* octave, const float* angle, const int32_t* obs);
int sd_track_set_poses(sd_track* h, int frame0, int n_frames, const double* Tref_cm,
                       const double* Tcur_cm);
/* raw rand() values consumed by SD_SLAM::Random, 4 per RANSAC iteration (src/extra/utils.cc:23-26,
 * src/PnPsolver.cc:185-194); rand_values is [n_frames][per_frame] */
int sd_track_set_rand(sd_track* h, int frame0, int n_frames, const int32_t* rand_values, int per_frame);

/* Stereo / RGB-D information of the current frames: either mvuRight directly, or
 * Frame::ComputeStereoFromRGBD (src/Frame.cc:399-417) from CV_32F depth images in host memory
 * (mvDepth, mvuRight = kpU.x - mbf / d); bf comes from sd_track_set_camera. */
int sd_track_set_uright(sd_track* h, int frame0, int n_frames, const float* uright, int cap);
int sd_track_stereo_from_depth(sd_track* h, int n_frames, const float* depth, int w, int hgt,
                               int stride_elems, size_t frame_stride_elems);
int sd_track_get_stereo(sd_track* h, int frame0, int n_frames, float* uright, float* depth, int cap);
/* sd_track_stereo_from_depth_device: the same mvuRight / mvDepth from depth maps already in DEVICE memory, converted as
 * Tracking::GrabImageRGBD does (src/Tracking.cc:113-117, 147-148).  d_depth holds n_frames maps of w x hgt elements of
 * `dtype`, rows stride_elems apart, frames frame_stride_elems apart (both in elements), aligned to the element size.
 * depth_map_factor = Config::DepthMapFactor(): scale = 1 if |factor| < 1e-5, else 1.0f / factor; the depth is
 * (float)raw * scale, one float product, when |scale - 1| > 1e-5 or dtype is SD_DEPTH_U16, raw otherwise (raw 0: no depth).
 * Queued on the tracking stream (the one sd_track_stream_fence orders) behind the current extraction and the tracking calls
 * queued before it: no host wait, no allocation, no copy of the maps.  A producer on another stream S is ordered with
 * sd_track_stream_fence(h, S, 1) before the call; the maps may be rewritten or freed after sd_track_stream_fence(h, S, 0)
 * (S then waits for the call) or after any synchronising getter.  Slots >= n_frames are left alone; in broadcast mode the
 * call walks the frames of the cur extractor, as sd_track_stereo_from_depth does.  SD_ERR_INVALID_ARG: NULL pointer, unknown
 * dtype, w / hgt < 1, stride < w, a misaligned pointer, no camera, no extraction; SD_ERR_CAPACITY: n_frames > max_batch. */
#define SD_DEPTH_F32 0  /* float    */
#define SD_DEPTH_U16 1  /* uint16_t */
int sd_track_stereo_from_depth_device(sd_track* h, int n_frames, const void* d_depth, int dtype, int w, int hgt,
                                      int stride_elems, size_t frame_stride_elems, float depth_map_factor);

/* TrackLocalMap's search (reference src/Tracking.cc:898-939): Frame::isInFrustum (src/Frame.cc:215-269, incl.
 * MapPoint::PredictScale src/MapPoint.cc:371-385) for every local map point with cand != 0, then
 * ORBmatcher::SearchByProjection(Frame&, const vector<MapPoint*>&, th) (src/ORBmatcher.cc:43-126) with
 * mfNNratio = nnratio, at the frames' current poses.  Per-point arrays are [n_frames][max_points]:
 * min_dist / max_dist = GetMin/MaxDistanceInvariance(), mf_max_dist = mfMaxDistance, normal = GetNormal(),
 * obs = Observations(); kp_claimed [n_frames][kp_cap] (may be NULL) marks keypoints that already hold a map
 * point with Observations() > 0.  Results: local_match[kp] = index of the assigned local point or -1,
 * in_view = mbTrackInView, proj3 = {mTrackProjX, mTrackProjY, mTrackProjXR}, level = mnTrackScaleLevel. */
int sd_track_set_local(sd_track* h, int frame0, int n_frames, const int32_t* n_local, const uint8_t* cand, const double* Xw,
                       const double* normal, const float* min_dist, const float* max_dist, const float* mf_max_dist,
                       const uint8_t* desc, const int32_t* obs, const uint8_t* kp_claimed);
int sd_track_match_local(sd_track* h, int n_frames, float th, float nnratio, float viewing_cos_limit);
/* The same search on the CALLER's isInFrustum results -- what ORBmatcher::SearchByProjection(Frame&, const vector<MapPoint*>&, th)
 * itself reads from the map points (src/ORBmatcher.cc:48-60): in_view = mbTrackInView && !isBad(), proj3 = {mTrackProjX,
 * mTrackProjY, mTrackProjXR}, level = mnTrackScaleLevel, view_cos = mTrackViewCos; [n_frames][max_points] arrays.  Results
 * through sd_track_get_local. */
int sd_track_set_local_view(sd_track* h, int frame0, int n_frames, const int32_t* n_local, const uint8_t* in_view, const float* proj3,
                            const int32_t* level, const float* view_cos, const uint8_t* desc, const int32_t* obs, const uint8_t* kp_claimed);
int sd_track_match_local_view(sd_track* h, int n_frames, float th, float nnratio);
int sd_track_get_local(sd_track* h, int frame0, int n_frames, int32_t* local_match, int cap, int32_t* n_matches,
                       uint8_t* in_view, float* proj3, int32_t* level, float* view_cos);

/* Optimizer::PoseOptimization(Frame*) (reference src/Optimizer.cc:221-415: g2o Levenberg, Huber kernel, 4 rounds of
 * 10 iterations with outlier re-classification), the pose solve the reference runs after SearchByProjection
 * (src/Tracking.cc:693) and after the local-map search (:729).  Input pose = the frames' current poses; map points =
 * the matches of sd_track_match (source 0) or sd_track_match_local (source 1); stereo observations where
 * mvuRight >= 0.  Results: optimised Tcw (16 doubles column-major), mvbOutlier flags, info8 = {nInitialCorrespondences,
 * nBad, rounds, g2o iterations, LM trials, return value (nInitial - nBad), 0, 0}. */
int sd_track_pose_opt(sd_track* h, int n_frames, int source);
int sd_track_get_pose_opt(sd_track* h, int frame0, int n_frames, double* Tcw_cm, uint8_t* outlier, int cap, int32_t* info8);

/* One current frame against many keyframes.  After sd_track_set_current_broadcast(h, c) with c >= 0, slot f of every
 * later sd_track_align / _match / _pnp / _pose_opt pairs its own map points, poses and ref-extractor frame f with frame c
 * of the cur extractor (and with row c of mvuRight); -1 restores slot f <-> current frame f.  The cur extractor may then
 * hold fewer frames than the tracker has slots.
 *
 * sd_track_relocalize: Tracking::Relocalization (src/Tracking.cc:1064-1097) with every keyframe attempt of its loop run
 * as one batch slot: ImageAlign::ComputePose(frame, kf, fast) -> SearchByProjection(frame, kf, th, mono) with orientation
 * check -> PoseOptimization.  Slots are in the order the reference tries them (newest keyframe first); *winner = first
 * slot with align ok, nmatches >= min_matches (20) and nGood >= min_good (10), or -1 (= Relocalization returns false).
 * stage3 (may be NULL): [n][3] = {align ok, nmatches, nGood} of every slot.
 *
 * sd_track_detect_loop: the candidate search of LoopClosing::DetectLoop (src/LoopClosing.cc:115-149):
 * ImageAlign::ComputePose(mpCurrentKF, kfs[i]) for all i as one batch, then the reference's loop replayed over the
 * results (skip excluded[i] != 0; a failed alignment also skips slot i+1; best error; keep error < 1.5 * best).
 * candidates: slot indices in ascending order (the reference's std::map<KeyFrame*,...> order is pointer order). */
int sd_track_set_current_broadcast(sd_track* h, int cur_frame);
int sd_track_relocalize(sd_track* h, int n_keyframes, int cur_frame, float th, int mono, int min_matches, int min_good,
                        int32_t* winner, int32_t* stage3);
int sd_track_detect_loop(sd_track* h, int n_keyframes, int cur_frame, const uint8_t* excluded, int32_t* candidates, int cap,
                         int32_t* n_candidates, double* best_error, double* errors);

/* Tracking::TrackWithMotionModel (src/Tracking.cc:654-718) for the batch in one call: ImageAlign (align_mode 0: against the
 * last frame; 1: ComputePose(frame, reference keyframe) as in TrackReferenceKeyFrame :583-644; -1: align_image_ off) ->
 * SearchByProjection(th) -> if nmatches < min_matches: pose := predicted and SearchByProjection(2 th) -> if still
 * < min_matches: failed -> PoseOptimization -> outliers discarded, nmatchesMap counted -> tracked iff nmatchesMap >=
 * min_inliers.  The reference's constants are min_matches = 20, min_inliers = 10.  All per-frame decisions are taken on the
 * device.  Afterwards: sd_track_get_tracked (info4 = status 0 few matches / 1 few inliers / 2 tracked, nmatches, nmatchesMap,
 * retried), sd_track_get_pose_opt (the frame's pose; mvbOutlier all false after the discard), sd_track_get_matches
 * (mvpMapPoints after the discard). */
int sd_track_with_motion_model(sd_track* h, int n_frames, int align_mode, float th, int mono, int min_matches, int min_inliers);
int sd_track_get_tracked(sd_track* h, int frame0, int n_frames, int32_t* info4);

/* Tracking::TrackLocalMap (src/Tracking.cc:720-751) for the batch, on top of the frame-to-frame matches and pose that
 * sd_track_with_motion_model (or sd_track_match) left: SearchLocalPoints (:898-939) over the local map of sd_track_set_local
 * (a keypoint is closed to the search where its frame match has Observations() > 0; kp_claimed of sd_track_set_local is not
 * used) -> PoseOptimization over all of mvpMapPoints -> mnMatchesInliers -> tracked iff >= min_inliers (reference: 30).
 * th = 1 (3 for RGB-D, 5 right after a relocalisation), nnratio = 0.8, viewing_cos_limit = 0.5 in the reference.
 * sd_track_get_local_map: map_match[i] = -1 | v < max_points: last-frame point v | v >= max_points: local point v - max_points;
 * info4 = {status 1 failed / 2 tracked, points in mvpMapPoints, mnMatchesInliers, local matches}.  Pose and mvbOutlier:
 * sd_track_get_pose_opt; isInFrustum outputs: sd_track_get_local.  sd_track_pose_opt(h, n, 2) runs the optimisation alone
 * on the same union. */
int sd_track_local_map(sd_track* h, int n_frames, float th, float nnratio, float viewing_cos_limit, int min_inliers);
int sd_track_get_local_map(sd_track* h, int frame0, int n_frames, int32_t* map_match, int cap, int32_t* info4);

/* ORBmatcher::SearchByPoints(KeyFrame* currentKF, KeyFrame* pKF, vector<MapPoint*>& matches)
 *   src/ORBmatcher.h:56, src/ORBmatcher.cc:1209-1301 (caller: LoopClosing::ComputeSim3, src/LoopClosing.cc:255)
 * Brute-force Hamming matching between the map points of two keyframes, for the whole batch: slot f pairs frame f (or the
 * broadcast frame) of the cur extractor with frame f of the ref extractor.  has_mp_cur / has_mp_ref [n_frames][cap]:
 * GetMapPointMatches()[i] != NULL && !isBad().  nnratio = mfNNratio (0.75 in ComputeSim3), check_ori = mbCheckOrientation.
 * matches12[i] = index of the pKF keypoint whose map point the reference stores in matches[i], or -1; *n_matches = return value. */
int sd_track_set_point_flags(sd_track* h, int frame0, int n_frames, const uint8_t* has_mp_cur, const uint8_t* has_mp_ref, int cap);
int sd_track_search_by_points(sd_track* h, int n_frames, float nnratio, int check_ori);
int sd_track_get_point_matches(sd_track* h, int frame0, int n_frames, int32_t* matches12, int cap, int32_t* n_matches);

/* Sim3Solver(KeyFrame* pKF1, KeyFrame* pKF2, const vector<MapPoint*>& vpMatched12, bool bFixScale)
 *   src/Sim3Solver.h, src/Sim3Solver.cc:36-393 (caller: LoopClosing::ComputeSim3, src/LoopClosing.cc:255-283, right after
 *   SearchByPoints: SetRansacParameters(0.99, 20, 300), then iterate(5) round-robin over the candidates)
 * for the whole batch, one solver per slot: KF1 = the slot's cur frame (or the broadcast frame) with pose Tcur, KF2 = frame f
 * of the ref extractor with pose Tref (sd_track_set_poses).  vpMatched12 is the matches12 buffer: what sd_track_search_by_points
 * left there (no host copy), or any vector given to sd_track_set_point_matches (cap entries per slot, the rest NULL; entries
 * in [-1, keypoint capacity)), as sd_track_set_matches does for PnPsolver.  A correspondence needs both map points valid:
 * has_mp_cur[i1] and has_mp_ref[matches12[i1]] of sd_track_set_point_flags, i.e. != NULL && !isBad(), the constructor's test
 * (:65-69).  GetIndexInKeyFrame is taken as the identity: indexKF1 = i1, indexKF2 = matches12[i1] (:71-72); an index beyond
 * the keypoints the extraction produced is no correspondence.  K, the keypoint octaves and mvLevelSigma2 are the tracker's and
 * the extractors' own.
 * sd_track_set_sim3_points: pMP->GetWorldPos() of the two keyframes' map points, [n_frames][cap][3] doubles each, indexed by
 *   that keyframe's keypoint index (:90-96).
 * sd_track_sim3 = constructor (:36-110) + SetRansacParameters(probability, min_inliers, max_iterations) (:112-135) +
 *   iterate(n_iterations) (:137-198; n_iterations = max_iterations is find(), :200-203) for slots 0 .. n_frames - 1.
 *   probability in (0, 1), min_inliers >= 3, max_iterations >= 1, n_iterations >= 1.
 * sd_track_sim3_iterate = a further iterate(n_iterations): mnIterations, mnBestInliers, mvbBestInliers, mBestT12, the best
 *   R / t / scale and the position in the rand() stream persist on the device.  The lifetime rule is sd_track_pnp_iterate's:
 *   a new extraction on `cur` or `ref`, sd_track_search_by_points, sd_track_set_point_matches / _set_sim3_points /
 *   _set_point_flags / _set_poses / _set_rand, or another broadcast setting end the solvers' life, and the next
 *   sd_track_sim3_iterate fails with SD_ERR_INVALID_ARG until sd_track_sim3 constructs new ones.
 * Both are queued on the tracking stream: no host wait, no allocation.  Draws use the stream of sd_track_set_rand, 3 values
 * per iteration (Random(0, size - 1) with size N, N - 1, N - 2; src/extra/utils.cc:23-26); a call that could run past the
 * supplied values fails with SD_ERR_INVALID_ARG before anything is launched.
 * sd_track_get_sim3 (synchronises; NULL outputs are skipped): T12_cm = the matrix iterate() returned, 16 doubles
 *   column-major, all zero when none was returned; R12_cm (9, column-major) / t12 (3) / scale (1; a float value) =
 *   GetEstimatedRotation / Translation / Scale (:344-354), the best so far whether returned or not (zeros before the first
 *   iteration); inliers[i1] = vbInliers over KF1's keypoints (mN1 = the keypoint capacity; cap >= it);
 *   info8 = {returned (0/1), nInliers, bNoMore, mnIterations, N, mRansacMaxIts, mnBestInliers, 0}. */
int sd_track_set_sim3_points(sd_track* h, int frame0, int n_frames, const double* Xw_cur, const double* Xw_ref, int cap);
int sd_track_set_point_matches(sd_track* h, int frame0, int n_frames, const int32_t* matches12, int cap);
int sd_track_sim3(sd_track* h, int n_frames, int fix_scale, double probability, int min_inliers, int max_iterations, int n_iterations);
int sd_track_sim3_iterate(sd_track* h, int n_frames, int n_iterations);
int sd_track_get_sim3(sd_track* h, int frame0, int n_frames, double* T12_cm, double* R12_cm, double* t12, double* scale,
                      uint8_t* inliers, int cap, int32_t* info8);

/* ORBmatcher::SearchForTriangulation(KeyFrame* pKF1, KeyFrame* pKF2, const Eigen::Matrix3d& F12, vMatchedPairs)
 *   src/ORBmatcher.cc:359-475 with CheckDistEpipolarLine (:128-144), and LocalMapping::ComputeF12 (src/LocalMapping.cc:494-511);
 *   caller LocalMapping::CreateNewMapPoints, once per neighbour keyframe
 * for the whole batch on the SearchByPoints pairing: KF1 = the slot's cur frame (or the broadcast frame) with pose Tcur and
 * mvuRight row sd_track_set_uright (in broadcast mode the broadcast frame's row), KF2 = frame f of the ref extractor with pose
 * Tref and mvuRight row sd_track_set_uright_ref.  Poses are per slot: in broadcast mode every slot's Tcur holds KF1's pose.  Keypoints are the undistorted ones, K, mvScaleFactors and mvLevelSigma2 the
 * tracker's and the extractors' own.
 * Map-point flags are the buffers of sd_track_set_point_flags, read as "the keypoint holds a map point": for this call pass
 *   GetMapPointMatches()[i] != NULL -- bad points count, as in the reference (:385-389, :399-403).
 * sd_track_set_uright_ref: mvuRight of the ref extractor's frames, [n_frames][cap], rows shorter than the keypoint capacity
 *   leave the rest; -1 everywhere for a new handle, as the cur rows are.  Ordered on the tracking stream; returns once the rows are read.
 * sd_track_set_f12: the caller's own F12 for use_set_f12 = 1, 9 doubles row-major per slot.  Queued on the tracking stream.
 * sd_track_search_for_triangulation: use_set_f12 = 0 computes F12 from Tcur / Tref on the device, which is ComputeF12 (in
 *   double; operation order: sdslam_amd/csrc/track_tri.hip); the epipole is always computed from the poses.  check_ori =
 *   mbCheckOrientation (CreateNewMapPoints: off).  With check_ori = 0 the rows are independent, so one broadcast call over all
 *   neighbours followed by an in-order walk that skips the idx1 already turned into points equals the reference's sequential loop.
 *   Queued on the tracking stream: no host wait, no allocation.  The result lives in a buffer of its own: matches12 of
 *   sd_track_search_by_points and live Sim3 solvers are untouched.
 * sd_track_get_triangulation_matches (synchronises; NULL outputs are skipped): matches12[idx1] = the KF2 keypoint index of
 *   vMatchedPairs or -1 ([n_frames][cap], cap >= keypoint capacity), *n_matches = the return value, F12_rm9 = the F12 used,
 *   epipole2 = (ex, ey).  A result ends with a new extraction on `cur` or `ref`, sd_track_set_point_flags / _set_poses /
 *   _set_uright / _set_uright_ref / _set_f12 or another broadcast setting: the getter then fails with SD_ERR_INVALID_ARG until
 *   the search has run again.
 * Errors: SD_ERR_INVALID_ARG for use_set_f12 = 1 on a slot sd_track_set_f12 has not covered, missing extractions or camera;
 *   SD_ERR_CAPACITY for n_frames > max_batch or a keypoint capacity above 2048.
 * sd_debug_search_for_triangulation: one keyframe pair from host arrays through the same kernel, synchronous, with buffers of
 *   its own (no extractor, no tracker): n1 / n2 <= 2048 keypoints, has_mp / uright per keypoint, tables of nlevels entries;
 *   matches12 has n1 entries. */
int sd_track_set_uright_ref(sd_track* h, int frame0, int n_frames, const float* uright, int cap);
int sd_track_set_f12(sd_track* h, int frame0, int n_frames, const double* F12_rm9);
int sd_track_search_for_triangulation(sd_track* h, int n_frames, int use_set_f12, int check_ori);
int sd_track_get_triangulation_matches(sd_track* h, int frame0, int n_frames, int32_t* matches12, int cap, int32_t* n_matches,
                                       double* F12_rm9, float* epipole2);
int sd_debug_search_for_triangulation(int n1, int n2, const sd_keypoint* kps1, const uint8_t* desc1, const uint8_t* has_mp1,
                                      const float* uright1, const sd_keypoint* kps2, const uint8_t* desc2, const uint8_t* has_mp2,
                                      const float* uright2, const double* F12_rm9, const float* epipole2, const float* scale_factors,
                                      const float* level_sigma2, int nlevels, int check_ori, int32_t* matches12, int32_t* n_matches);

/* LocalMapping::CreateNewMapPoints after the search (src/LocalMapping.cc:219-419 with KeyFrame::UnprojectStereo
 *   src/KeyFrame.cc:572-585 and MapPoint::UpdateNormalAndDepth src/MapPoint.cc:304-343)
 * on the live result of sd_track_search_for_triangulation, same pairing, poses, mvuRight rows and camera: every match is
 * triangulated and tested as :268-399 does (operand widths and operation order: sdslam_amd/csrc/track_newpoints_tri.hip), and
 * the accepted ones become map point rows.  Nothing is downloaded in between.
 * sd_track_set_tri_depth: mvDepth rows, [n_frames][cap], rows shorter than the keypoint capacity leave the rest.  side 0: the
 *   frames of `cur` (frame0 counts cur frames: in broadcast mode KF1's row is the broadcast frame's) -- the row
 *   sd_track_stereo_from_depth / _device fill, so an RGB-D caller needs side 1 only; side 1: the frames of `ref`.  -1 everywhere
 *   for a new handle.  Only rows of keypoints with mvuRight >= 0 are read.  Ordered on the tracking stream; returns once the
 *   rows are read.
 * sd_track_set_tri_median_depth: ComputeSceneMedianDepth(2) of KF2 per slot for the monocular baseline gate (:234-238); a
 *   negative entry (the value of a new handle) switches the slot's gate off.  Queued on the tracking stream.
 * sd_track_triangulate: monocular = mbMonocular (it selects the baseline gate of :230-239 only).  Queued on the tracking
 *   stream: no host wait, no allocation.  SD_ERR_INVALID_ARG when no live search result covers the slots, and under the
 *   broadcast when that search ran with check_ori = 1 (its rows are then not independent; the reference's matcher has it off).  Under
 *   sd_track_set_current_broadcast a KF1 keypoint becomes a point of the FIRST slot that accepts it, which is the reference's
 *   loop over the neighbours; ids count from slot 0's sd_track_set_next_map_id value, which advances.  Paired: every accepted
 *   row is a point of its slot, ids count from the slot's own counter, which advances.
 * sd_track_get_triangulated (synchronises; NULL outputs are skipped): verdict / branch [n_frames][cap], Xw [n_frames][cap][3],
 *   cap >= keypoint capacity; n_accepted[f] = rows with verdict SD_TRI_ACCEPTED.  Xw is x3D of every row that chose a branch.
 * sd_track_get_new_points (synchronises; NULL outputs are skipped): info4 = points, the broadcast setting, slots, the next id
 *   (-1 when paired: the slots' counters); then per point in (slot, idx1) order, arrays of cap >= info4[0] entries: the KF1
 *   keypoint, the slot, the KF2 keypoint, the id, Xw[3], mNormalVector[3], mfMaxDistance, mfMinDistance (sd_track_set_local
 *   takes 1.2f * and 0.8f * these) and the descriptor (KF1's keypoint's: of two observations the reference returns the first
 *   in pointer order).  SD_ERR_CAPACITY when cap is smaller; info4 is filled first.
 * A result ends with whatever ends the search's result, and with sd_track_set_tri_depth / _set_tri_median_depth /
 *   _set_camera / sd_track_stereo_from_depth / _device (they rewrite KF1's mvuRight and mvDepth, and end the search's result
 *   too): the getters then fail with SD_ERR_INVALID_ARG until sd_track_triangulate has run again.
 * sd_debug_triangulate: one keyframe pair and an explicit matches12 row (n1 entries, -1 or < n2) from host arrays through the
 *   same kernel, synchronous, with buffers of its own.  kps*_un = mvKeysUn, kps* = mvKeys; cam5 = fx, fy, cx, cy, mbf;
 *   scale_factor = mfScaleFactor; verdict / branch [n1], Xw [n1][3]. */
#define SD_TRI_NO_MATCH 0
#define SD_TRI_ACCEPTED 1
#define SD_TRI_LOW_PARALLAX 2   /* no stereo and low parallax (:322) */
#define SD_TRI_W_ZERO 3         /* x3D[3] == 0 (:311) */
#define SD_TRI_Z1 4             /* z1 <= 0 */
#define SD_TRI_Z2 5
#define SD_TRI_REPROJ1 6        /* reprojection error in KF1 */
#define SD_TRI_REPROJ2 7
#define SD_TRI_DIST_ZERO 8      /* dist1 == 0 || dist2 == 0 */
#define SD_TRI_SCALE 9          /* scale consistency (:398) */
#define SD_TRI_SLOT_GATED 10    /* the neighbour's baseline is too short (:225-239) */
#define SD_TRI_BRANCH_SVD 1
#define SD_TRI_BRANCH_UNPROJECT1 2
#define SD_TRI_BRANCH_UNPROJECT2 3
int sd_track_set_tri_depth(sd_track* h, int side, int frame0, int n_frames, const float* depth, int cap);
int sd_track_set_tri_median_depth(sd_track* h, int frame0, int n_frames, const float* median_depth);
int sd_track_triangulate(sd_track* h, int n_frames, int monocular);
int sd_track_get_triangulated(sd_track* h, int frame0, int n_frames, uint8_t* verdict, uint8_t* branch, double* Xw, int cap,
                              int32_t* n_accepted);
int sd_track_get_new_points(sd_track* h, int32_t* info4, int32_t* kp1, int32_t* slot, int32_t* idx2, int32_t* ids, double* Xw,
                            double* normal, float* max_dist, float* min_dist, uint8_t* desc, int cap);
int sd_debug_triangulate(int n1, int n2, const sd_keypoint* kps1_un, const sd_keypoint* kps1, const float* uright1, const float* depth1,
                         const sd_keypoint* kps2_un, const sd_keypoint* kps2, const float* uright2, const float* depth2,
                         const int32_t* matches12, const double* Tcw1_cm16, const double* Tcw2_cm16, const float* cam5,
                         const float* scale_factors, const float* level_sigma2, int nlevels, float scale_factor, int monocular,
                         float median_depth, uint8_t* verdict, uint8_t* branch, double* Xw);

/* The new points become local-map rows on the device (sdslam_amd/csrc/track_append.hip): between sd_track_triangulate and
 *   sd_track_fuse / sd_track_match_local / sd_track_refresh_points nothing has to be downloaded, rebuilt and uploaded.
 * sd_track_append_new_points copies the points of the live sd_track_triangulate result, in creation order g = 0 .. info4[0] - 1,
 *   behind the n_local points a local row holds, and advances n_local.  Queued on the tracking stream: no host wait, no allocation.
 *   Per point: Xw, normal, mf_max_dist = mfMaxDistance, max_dist = 1.2f * mfMaxDistance, min_dist = 0.8f * mfMinDistance, desc, and
 *   obs = nObs after CreateNewMapPoints' two AddObservation calls (src/MapPoint.cc:98-108): (mvuRight1[kp1] >= 0 ? 2 : 1) +
 *   (mvuRight2[idx2] >= 0 ? 2 : 1) on the sd_track_set_uright / _set_uright_ref rows the triangulation read.  kp_claimed keeps its bytes.
 *   point_row = r >= 0 (the broadcast CreateNewMapPoints feeding the first loop of SearchInNeighbors, or any result): all points go
 *     to row r, point g to position base + g with base = n_local[r].  For every f < n_cand_rows, cand[f][base + g] = (f != slot of
 *     g) = !IsInKeyFrame(ref frame f): the Fuse targets are a superset of the triangulation's neighbours, which the caller keeps in
 *     the first ref frames; rows beyond the triangulation's slots get 1.
 *   point_row = -1 (a paired result only): the points of slot b go to row b behind n_local[b], in order, with cand = 1 -- local
 *     points for the stream's next TrackLocalMap.
 *   A row takes only the first max_points - base points that arrive, in order; the rest are dropped and counted.
 *   mark_flags = 1 also sets the "holds a map point" flags of sd_track_set_point_flags for the appended points, as AddMapPoint does
 *     to mvpMapPoints: the ref flag of row slot at idx2, and the cur flag at kp1 in the row of every slot that stands for KF1 -- row
 *     slot when paired, rows 0 .. slots - 1 under the broadcast -- so that a second sd_track_search_for_triangulation passes over them.
 *   It ends the cached results sd_track_set_local ends (sd_track_get_fuse, _get_refreshed), and with mark_flags those
 *   sd_track_set_point_flags ends (the search's result and its triangulation, the Sim3 solvers).  sd_track_get_new_points keeps
 *   working until the append's own result ends: the caller's objects need kp1, slot, idx2 and id, and point g stands at base + g
 *   (paired: at base of its slot + its rank within the slot).
 *   SD_ERR_INVALID_ARG: no live sd_track_triangulate result; its points have been appended already; point_row outside
 *   [-1, max_batch); point_row = -1 under the broadcast; n_cand_rows outside [0, max_batch]; mark_flags outside {0, 1}.
 * sd_track_get_appended (synchronises; NULL outputs are skipped): per local row frame0 .. frame0 + n_rows - 1 of the last append,
 *   base = n_local before it, appended, dropped (rows that received nothing: n_local, 0, 0).  The result ends with the next
 *   sd_track_set_local / _set_local_view, a write-through sd_track_refresh_points, sd_track_triangulate or the next append.
 * sd_track_get_local_points (synchronises; NULL outputs are skipped): local row `row` as it is on the device, whoever wrote it
 *   last (sd_track_set_local, this append, a write-through refresh): n_local and the arrays of sd_track_set_local, max_points
 *   entries each, cap >= max_points. */
int sd_track_append_new_points(sd_track* h, int point_row, int n_cand_rows, int mark_flags);
int sd_track_get_appended(sd_track* h, int frame0, int n_rows, int32_t* base, int32_t* appended, int32_t* dropped);
int sd_track_get_local_points(sd_track* h, int row, int32_t* n_local, uint8_t* cand, double* Xw, double* normal, float* min_dist,
                              float* max_dist, float* mf_max_dist, uint8_t* desc, int32_t* obs, int cap);

/* ORBmatcher::Fuse, both overloads: the search (src/ORBmatcher.cc:493-594 with a keyframe pose, :639-715 with a Sim3 Scw;
 *   KeyFrame::GetFeaturesInArea / IsInImage src/KeyFrame.cc:529-570; MapPoint::PredictScale src/MapPoint.cc:355-369; callers
 *   LocalMapping::SearchInNeighbors src/LocalMapping.cc:422-492 and LoopClosing::SearchAndFuse src/LoopClosing.cc:535-560)
 * for the whole batch: slot f projects a list of map points into one keyframe and returns, per point i, best_idx[i] = the keypoint
 * the reference reaches :597 / :718 with (bestDist <= TH_LOW = 50), else -1, and best_dist[i] = bestDist (256: no candidate).
 * The search reads nothing the reference's fusing changes (no observations, no mvpMapPoints), so all keyframes of a
 * SearchInNeighbors or SearchAndFuse go in one call; Replace / AddObservation / AddMapPoint stay with the caller, who walks the
 * results in the reference's order (ORBmatcher::Fuse of include/sdslam/sdslam.hpp does).
 * Points: the local-map buffers of sd_track_set_local, same fields and layout (obs and kp_claimed are not read); here
 *   cand[f][i] = pMP != NULL && !isBad() && !IsInKeyFrame(KF of slot f) at upload time.  sd_track_set_local is shared with
 *   TrackLocalMap's search: like relocalisation and loop detection, Fuse is meant for a tracker handle of its own.
 * kf_side 0: KF = the slot's cur frame (or the broadcast frame), pose Tcur of the slot, mvuRight row sd_track_set_uright.  Under
 *   sd_track_set_current_broadcast this is the second Fuse of SearchInNeighbors (all candidates against the current keyframe),
 *   split over as many slots as the list needs.
 * kf_side 1: KF = frame f of the ref extractor, pose Tref, mvuRight row sd_track_set_uright_ref: over n target keyframes the
 *   first loop of SearchInNeighbors.
 * point_row -1: slot f reads point row f.  r >= 0: every slot reads n_local, Xw, normal, the distances and desc of row r and only
 *   cand of its own row -- one upload of the current keyframe's points for all neighbours.
 * sim3 0: the keyframe-pose overload, with its chi-square gate (7.8 for keypoints with mvuRight >= 0, 5.99 otherwise).
 * sim3 1: the Scw overload: the slot's Scw (sd_track_set_fuse_scw, 16 doubles column-major, queued on the tracking stream) is
 *   decomposed on the device as :625-629 does (operation order: sdslam_amd/csrc/track_fuse.hip); no chi-square gate.
 * th: the search radius factor (3.0 in SearchInNeighbors, 4 in SearchAndFuse).  Keypoints are the undistorted ones; K, the image
 *   bounds, mvScaleFactors and mvInvLevelSigma2 are the tracker's and the extractor's own (sd_track_create requires both extractors
 *   to share nlevels and scaleFactor, so PredictScale is the same on either side).
 * sd_track_fuse is queued on the tracking stream: no host wait, no allocation.  The result lives in buffers of its own: the results
 *   of sd_track_match_local, sd_track_search_by_points and sd_track_search_for_triangulation are untouched.
 * sd_track_get_fuse (synchronises; NULL outputs are skipped): best_idx / best_dist [n_frames][cap], cap >= max_points, entries
 *   beyond n_local read -1 / 256; n_found[f] = points with best_idx >= 0 (= nFused when the walk skips none).  A result ends with
 *   a new extraction on the side in use, sd_track_set_local / _set_local_view / _set_poses / _set_uright / _set_uright_ref /
 *   _set_fuse_scw / _set_camera or another broadcast setting: the getter then fails with SD_ERR_INVALID_ARG until the search
 *   has run again.
 * Errors: SD_ERR_INVALID_ARG for a NULL handle, th <= 0 or not finite, point_row outside [-1, max_batch), kf_side / sim3 outside
 *   {0, 1}, sim3 = 1 on a slot sd_track_set_fuse_scw has not covered, a missing extraction or camera; SD_ERR_CAPACITY for
 *   n_frames > max_batch.
 * sd_debug_fuse: one keyframe and one point list from host arrays through the same kernel, synchronous, with buffers of its own
 *   (no extractor, no tracker).  n_kp <= kp_cap <= 2048 keypoints, n_pts <= max_points <= 2048 points (the capacities shape the
 *   launch as a tracker's would); T_cm16 = Tcw or Scw, column-major; cam9 = fx, fy, cx, cy, bf, mnMinX, mnMaxX, mnMinY, mnMaxY;
 *   tables of nlevels entries, scale_factor = mfScaleFactor (for PredictScale).  best_idx / best_dist have max_points entries;
 *   pose15 (may be NULL) = Rcw row-major | tcw | Ow as projected with (also sd_track_debug_read, which = 2, bytes <= 120). */
int sd_track_set_fuse_scw(sd_track* h, int frame0, int n_frames, const double* Scw_cm16);
int sd_track_fuse(sd_track* h, int n_frames, int kf_side, int point_row, float th, int sim3);
int sd_track_get_fuse(sd_track* h, int frame0, int n_frames, int32_t* best_idx, int32_t* best_dist, int cap, int32_t* n_found);
int sd_debug_fuse(int n_kp, const sd_keypoint* kps, const uint8_t* desc, const float* uright, int n_pts, const uint8_t* cand,
                  const double* Xw, const double* normal, const float* min_dist, const float* max_dist, const float* mf_max_dist,
                  const uint8_t* pt_desc, const double* T_cm16, int sim3, const float* cam9, const float* scale_factors,
                  const float* inv_level_sigma2, int nlevels, float scale_factor, float th, int kp_cap, int max_points,
                  int32_t* best_idx, int32_t* best_dist, int32_t* n_found, double* pose15);

/* MapPoint::ComputeDistinctiveDescriptors (src/MapPoint.cc:225-284) and MapPoint::UpdateNormalAndDepth (:304-343) for a list of map
 *   points: what LocalMapping::SearchInNeighbors (src/LocalMapping.cc:478-488), CreateNewMapPoints' recent points (:140-147),
 *   LoopClosing::SearchAndFuse (src/LoopClosing.cc:457-484) and Tracking::CreateNewKeyFrame (src/Tracking.cc:874-875) call per point.
 *   Their outputs are the desc, normal, min_dist, max_dist and mf_max_dist fields of sd_track_set_local.
 * Keyframes are frames of the extractors.  An observation is (obs_frame, obs_kp): obs_frame >= 0 is a frame of the ref extractor,
 *   with pose Tref of that slot (sd_track_set_poses); -1 is the current keyframe: the broadcast frame of the cur extractor
 *   (sd_track_set_current_broadcast), or its frame 0 without a broadcast, with pose Tcur of slot 0; -2 is a keyframe that is not
 *   resident on the device.  obs_kp indexes that frame's keypoints.
 * sd_track_set_observations: the observations of n_points <= max_points points as CSR -- point i owns entries obs_off[i] ..
 *   obs_off[i + 1] - 1 of obs_frame / obs_kp / obs_kf_bad, obs_off[0] = 0 -- IN THE ORDER IN WHICH THE CALLER ITERATES mObservations.
 *   The reference's order is that of a std::map keyed by pointer; it decides ties of the least median (strict <: the first wins)
 *   and the order of the normal's sum, so the result is defined as the reference's loops run over the list as given.
 *   ref_obs[i] = the position of mpRefKF in point i's own list.  obs_kf_bad (may be NULL) marks observations whose keyframe
 *   isBad(): ComputeDistinctiveDescriptors skips them (:246), UpdateNormalAndDepth does not and counts them in n (:323-329).
 *   point_bad (may be NULL) marks points that are bad.  The host arrays are copied before the call returns; the upload itself is
 *   queued on the tracking stream.  The device block for the lists is allocated by sd_track_create for max_points points of 16
 *   observations each; a call that needs more replaces it by a larger one (this, and only this, waits for the tracking stream and
 *   allocates), and it never shrinks.
 *   SD_ERR_INVALID_ARG: obs_off[0] != 0 or not monotone, obs_frame outside [-2, max_batch), ref_obs outside its (non-empty) list;
 *   SD_ERR_CAPACITY: n_points > max_points.  Keypoint indices are checked on the device against the frame's keypoint count.
 * sd_track_refresh_points: both functions for every point of the list; world positions are Xw of row point_row of the
 *   sd_track_set_local buffers, point i of the list = entry i of the row.  Queued on the tracking stream: no host wait, no
 *   allocation.  write_local = 1 also writes desc, normal, mf_max_dist = mfMaxDistance, max_dist = 1.2f * mfMaxDistance and
 *   min_dist = 0.8f * mfMinDistance (GetMaxDistanceInvariance / GetMinDistanceInvariance) into that row, for the parts the status
 *   says were written; everything else keeps its bytes.  A later sd_track_fuse / sd_track_match_local sees the refreshed points
 *   without an upload.  A write-through ends the cached results sd_track_set_local ends (sd_track_get_fuse); write_local = 0 ends none.
 * sd_track_get_refreshed (synchronises; NULL outputs are skipped; cap >= n_points entries each): status[i] = SD_REFRESH_DESC |
 *   SD_REFRESH_NORMAL for what was written, or one reason and nothing written: SD_REFRESH_SKIPPED (point bad or no observations:
 *   both functions return early), SD_REFRESH_NOT_RESIDENT (an observation with frame -2), SD_REFRESH_TOO_MANY (more than
 *   SD_REFRESH_MAX_OBS observations) -- these two leave the point to the caller -- or SD_REFRESH_BAD_INDEX (a keypoint index
 *   outside its frame; nothing is read through it).  A point whose observing keyframes are all bad has SD_REFRESH_NORMAL alone.
 *   best_obs = BestIdx as a position in the caller's list, best_median = BestMedian, desc [.][32], normal [.][3],
 *   max_dist = mfMaxDistance, min_dist = mfMinDistance.  Entries that were not written hold what an earlier call left.
 *   The result ends with a new extraction on either side, sd_track_set_poses, _set_local, _set_observations or another broadcast
 *   setting: the getter then fails with SD_ERR_INVALID_ARG until sd_track_refresh_points has run again.
 * sd_debug_refresh_points: the same kernel from host arrays, synchronous, with buffers of its own (no extractor, no tracker):
 *   per observation its descriptor [32], its keyframe's camera centre [3] (double) and its keypoint's octave; the CSR offsets, flags
 *   and ref_obs as above; Xw [n_points][3]; mvScaleFactors [nlevels].  The outputs are read AND written: entries the kernel does
 *   not write come back as they went in.
 * Arithmetic (operation order: sdslam_amd/csrc/track_refresh.hip): double where the reference has double, float where it has
 *   float, every operation rounded on its own; distances are sd_hamming's. */
#define SD_REFRESH_MAX_OBS 256
#define SD_REFRESH_DESC 1
#define SD_REFRESH_NORMAL 2
#define SD_REFRESH_SKIPPED 16
#define SD_REFRESH_NOT_RESIDENT 32
#define SD_REFRESH_TOO_MANY 64
#define SD_REFRESH_BAD_INDEX 128
int sd_track_set_observations(sd_track* h, int n_points, const int32_t* obs_off, const int32_t* obs_frame, const int32_t* obs_kp,
                              const uint8_t* obs_kf_bad, const int32_t* ref_obs, const uint8_t* point_bad);
int sd_track_refresh_points(sd_track* h, int point_row, int write_local);
int sd_track_get_refreshed(sd_track* h, uint8_t* status, int32_t* best_obs, int32_t* best_median, uint8_t* desc, double* normal,
                           float* max_dist, float* min_dist, int cap);
int sd_debug_refresh_points(int n_points, const int32_t* obs_off, const uint8_t* obs_desc, const double* obs_centre,
                            const int32_t* obs_octave, const uint8_t* obs_kf_bad, const int32_t* ref_obs, const uint8_t* point_bad,
                            const double* Xw, const float* scale_factors, int nlevels, uint8_t* status, int32_t* best_obs,
                            int32_t* best_median, uint8_t* desc, double* normal, float* max_dist, float* min_dist);

/* Optimizer::LocalBundleAdjustment (src/Optimizer.cc:417-714) on the lists of sd_track_set_observations: the step of the
 *   LocalMapping chain behind sd_track_append_new_points / _fuse / _refresh_points and before sd_track_cull_keyframes, without
 *   taking the map to the host.
 * The problem.  Points: point i of the list = entry i of row point_row of the sd_track_set_local buffers; the caller builds
 *   lLocalMapPoints in the reference's order (:432-445).  A point with point_bad set is not in the problem; an observation with
 *   obs_kf_bad set gives no edge (:541).  Keyframes: obs_frame >= 0 is a frame of the ref extractor with pose Tref, -1 the current
 *   keyframe with Tcur of slot 0 (as for the refresh).  sd_track_set_ba_keyframes gives their roles: kf_role[f], f < n_ref_frames,
 *   is 1 for a local keyframe, 2 for a local keyframe that is fixed (mnId == 0, :484), 0 otherwise; cur_role is 1 or 2.  Every
 *   other resident frame that a point of the list observes is a fixed camera (:447-460, :496).  A local keyframe that no point
 *   observes is a vertex without edges and keeps its pose.  Edges, in CSR order: mono where mvuRight < 0, else stereo; the
 *   measurement is the undistorted keypoint (and mvuRight), the information mvInvLevelSigma2[octave] * I, the Huber deltas
 *   (float)sqrt(5.991) and (float)sqrt(7.815), camera and bf the handle's (sd_track_set_camera).
 * The run (:608-683): optimize(5) with the robust kernel on every edge; every edge with chi2 > 5.991 (mono) / 7.815 (stereo) or
 *   !isDepthPositive goes to level 1 and the robust kernel comes off every edge; initializeOptimization(0) and optimize(10)
 *   (vertices without a level-0 edge leave the active set); the same test again gives obs_erase, one byte per CSR entry: 1 =
 *   vToErase would hold it.  g2o's Levenberg driver and Schur-complement block solver are restated
 *   (sdslam_amd/csrc/track_ba.hip, tests/ba_ref.py), three quirks included: lambda is re-initialised at iteration 0 of each
 *   optimize(); Terminate on rho == 0, after ten trials, and at _nBad >= 3; chi2() in both classifications is the error of the LAST
 *   computeActiveErrors (after a rejected last trial that of the rejected step; for a level-1 edge in round 2 round 1's last).
 *   pbStopFlag is not modelled: the caller checks it before the call, the device runs both rounds.  Double throughout; no
 *   floating-point atomics, every sum has one owner and a fixed order: two runs of one problem give the same bytes.
 * sd_track_local_ba is queued on the tracking stream: no host wait, no allocation (its scratch is allocated by sd_track_create for
 *   max_points points of 16 observations and max_batch + 1 cameras, and grows where sd_track_set_observations grows its block).
 *   write_back = 1, and only on SD_BA_OK: the optimised poses of the local keyframes with role 1 that some point observes go to
 *   Tref / Tcur, the positions of the SD_BA_POINT_OPTIMISED points to Xw of the row; everything else keeps its bytes.  It ends
 *   the cached results that sd_track_set_poses and a write-through refresh end; write_back = 0 ends none.  A
 *   sd_track_refresh_points queued behind it is the UpdateNormalAndDepth of :712, provided no observation was erased (otherwise
 *   behind sd_track_erase_observations(h, SD_ERASE_LOCAL_BA)).
 *   SD_ERR_INVALID_ARG: no sd_track_set_observations / sd_track_set_ba_keyframes / sd_track_set_camera before it.
 * sd_track_get_local_ba (synchronises; NULL outputs are skipped): T_ref_cm16 [n_ref_frames][16] and T_cur_cm16 [16] column-major,
 *   Xw [cap_points][3], point_status [cap_points] = SD_BA_POINT_OPTIMISED, _SKIPPED (bad, or no edge) or _BAD_INDEX (a keypoint
 *   index outside its frame; nothing is read through it), obs_erase [cap_obs], info16 = {status, n_local_free, n_fixed, n_points,
 *   n_edges_mono, n_edges_stereo, round-1 iterations, trials, exit, round-2 iterations, trials, exit, n_level1 after round 1,
 *   n_erase, 0, 0}; exits: 0 optimize() did not iterate, 1 _nBad >= 3, 2 ten trials rejected, 3 rho == 0, 4 the iterations were
 *   used.  status is SD_BA_OK or a refusal -- the problem is not run, nothing is written, poses and points are the inputs:
 *   SD_BA_NOT_RESIDENT (an observation of a live point with frame -2), SD_BA_TOO_MANY_KF (more than SD_BA_MAX_FREE_KF keyframes
 *   with role 1), SD_BA_BAD_INDEX (a keypoint index outside its frame).  The number of fixed cameras is bounded by max_batch only.
 * sd_debug_local_ba: the same kernels from host arrays, synchronous, with buffers of its own: per observation its keyframe
 *   obs_kf (an index into the n_kf poses and roles; -2: not resident; anything else outside [0, n_kf): a bad index), obs_uv [.][2],
 *   obs_ur and obs_inv_sigma2; the CSR offsets and flags; T_cm16 [n_kf][16]; kf_role [n_kf]; Xw; cam9 as for sd_debug_fuse
 *   (fx, fy, cx, cy, bf, ...).  T_out_cm16 [n_kf][16], Xw_out, point_status, obs_erase and info16 as the getter's. */
#define SD_BA_MAX_FREE_KF 32
#define SD_BA_OK 0
#define SD_BA_NOT_RESIDENT 1
#define SD_BA_TOO_MANY_KF 2
#define SD_BA_BAD_INDEX 3
#define SD_BA_POINT_SKIPPED 0
#define SD_BA_POINT_OPTIMISED 1
#define SD_BA_POINT_BAD_INDEX 2
int sd_track_set_ba_keyframes(sd_track* h, int n_ref_frames, const uint8_t* kf_role, int cur_role);
int sd_track_local_ba(sd_track* h, int point_row, int write_back);
int sd_track_get_local_ba(sd_track* h, double* T_ref_cm16, double* T_cur_cm16, double* Xw, uint8_t* point_status, uint8_t* obs_erase,
                          int32_t* info16, int cap_points, int cap_obs);
int sd_debug_local_ba(int n_points, const int32_t* obs_off, const int32_t* obs_kf, const float* obs_uv, const float* obs_ur,
                      const float* obs_inv_sigma2, const uint8_t* obs_kf_bad, const uint8_t* point_bad, int n_kf, const double* T_cm16,
                      const uint8_t* kf_role, const double* Xw, const float* cam9, double* T_out_cm16, double* Xw_out,
                      uint8_t* point_status, uint8_t* obs_erase, int32_t* info16);

/* Optimizer::BundleAdjustment / GlobalBundleAdjustemnt (src/Optimizer.cc:46-219) on the same lists: points, observations and
 *   keyframes are those of sd_track_set_observations / sd_track_set_ba_keyframes, point i is entry i of row point_row, obs_frame
 *   >= 0 is a ref frame with Tref, -1 the current keyframe with Tcur of slot 0.  The roles are read for this call as 1 = a free
 *   vertex, 2 = a fixed vertex (mnId == 0, :81), 0 = not a keyframe of vpKFs.  A live observation (point not bad, obs_kf_bad clear)
 *   whose camera has role 0 would be an edge to a vertex that does not exist: the call refuses with SD_BA_NO_VERTEX.  The other
 *   refusals are local BA's, in its order, SD_BA_NO_VERTEX last; SD_BA_TOO_MANY_KF: more than min(SD_GBA_MAX_FREE_KF,
 *   max_batch + 1) cameras with role 1.  A point that is bad or has no edge is vbNotIncludedMP (:170-175): SD_BA_POINT_SKIPPED,
 *   its position kept; a free keyframe without an edge keeps its pose.
 * Edges as in local BA; with robust = 1 Huber with (float)sqrt(5.99) (sic, :87) for mono and (float)sqrt(7.815) for stereo edges,
 *   with robust = 0 no kernel.  The run: initializeOptimization() and ONE optimize(n_iterations), 1 <= n_iterations <=
 *   SD_GBA_MAX_ITERATIONS, by the Levenberg driver local BA restates (lambda from computeLambdaInit, at most ten trials an
 *   iteration, the exits on rho == 0, ten rejected trials and _nBad >= 3, a zero pivot fails the trial with x = 0); no
 *   classification.  pbStopFlag is not modelled.  The reduced system of up to SD_BA_MAX_FREE_KF free cameras is factorised in LDS
 *   as in local BA, a larger one by a blocked LDL^T in global memory (panels of 48 columns, no pivoting, index order).
 * sd_track_global_ba is queued on the tracking stream: no host wait, no allocation.  write_back = 1 (the nLoopKF == 0 branch), only
 *   on SD_BA_OK: poses of the observed free cameras to Tref / Tcur, the optimised points to Xw of the row; it ends the cached
 *   results local BA's write-back ends.  write_back = 0 (nLoopKF != 0) writes nothing: mTcwGBA / mPosGBA are read through
 *   sd_track_get_global_ba (synchronises; NULL outputs are skipped), which answers a global run only (as sd_track_get_local_ba a
 *   local one) and not after sd_track_set_poses.  info16 = {status, n_free, n_fixed, n_points, n_edges_mono, n_edges_stereo,
 *   iterations, trials, exit, 0...}, exits numbered as in local BA.
 * sd_debug_global_ba: sd_debug_local_ba's inputs, n_iterations and robust; no obs_erase.
 * sd_debug_ldlt: only the blocked factorisation and both substitutions on a host matrix, synchronous, with buffers of its own:
 *   A_packed_lower is the lower triangle in row order (entry (r, c), c <= r, at r (r + 1) / 2 + c), 1 <= n <= 6 *
 *   SD_GBA_MAX_FREE_KF.  *ok = 0 and x = 0 on a zero pivot. */
#define SD_GBA_MAX_FREE_KF 256
#define SD_GBA_MAX_ITERATIONS 20
#define SD_BA_NO_VERTEX 4
int sd_track_global_ba(sd_track* h, int point_row, int n_iterations, int robust, int write_back);
int sd_track_get_global_ba(sd_track* h, double* T_ref_cm16, double* T_cur_cm16, double* Xw, uint8_t* point_status, int32_t* info16,
                           int cap_points);
int sd_debug_global_ba(int n_points, const int32_t* obs_off, const int32_t* obs_kf, const float* obs_uv, const float* obs_ur,
                       const float* obs_inv_sigma2, const uint8_t* obs_kf_bad, const uint8_t* point_bad, int n_kf, const double* T_cm16,
                       const uint8_t* kf_role, const double* Xw, const float* cam9, int n_iterations, int robust, double* T_out_cm16,
                       double* Xw_out, uint8_t* point_status, int32_t* info16);
int sd_debug_ldlt(int n, const double* A_packed_lower, const double* b, double* x, int32_t* ok);

/* LocalMapping::KeyFrameCulling (src/LocalMapping.cc:580-634), the last step of LocalMapping::Run, and the erasure of
 *   observations (MapPoint::EraseObservation, src/MapPoint.cc:110-134, with MapPoint::SetBadFlag, :146-161) on the lists of
 *   sd_track_set_observations.  A keyframe appears at most once in a point's list.  A point with point_bad set has neither
 *   observations nor matches in the reference: its entries are not read, counted or killed by either call.
 * sd_track_cull_keyframes is queued on the tracking stream: no host wait, no allocation (its scratch is allocated by
 *   sd_track_create and grows where sd_track_set_observations grows its block).  cand_frame[c] >= 0 is candidate c of
 *   mpCurrentKeyFrame->GetVectorCovisibleKeyFrames(), in that order, as a frame of the ref extractor; cand_flags[c] bit 0: mnId
 *   == 0 (the `continue` of :589), bit 1: mbNotErase (SetBadFlag only sets mbToBeErased).  SD_ERR_INVALID_ARG: a candidate outside
 *   [0, max_batch) or named twice, n_cand < 0, no observations set.  For each candidate in order, on the lists as the earlier
 *   candidates left them (:591-632): its points are those with a live entry in that frame that are not bad and have not gone bad
 *   in this run; with monocular == 0 a point whose mvDepth (the ref side's row of sd_track_set_tri_depth; -1 on a new handle) is
 *   > th_depth or < 0 is skipped; nMPs counts the others; one is redundant if Observations() > 3 -- the sum over its live entries
 *   of 2 where mvuRight >= 0 and 1 otherwise, obs_kf_bad entries included -- and at least 3 OTHER live entries have octave_i <=
 *   octave + 1 (the resident keypoints' octaves).  The keyframe is culled iff (double)nRedundant > 0.9 * (double)nMPs.  Verdicts:
 *   SD_CULL_SKIPPED_ID0, _KEPT, _CULLED, _TO_BE_ERASED (the test passed but bit 1 is set: nothing is erased).  Only _CULLED
 *   cascades: every live entry in that frame dies, its point's nObs falls by the entry's weight, a ref_obs that died moves to the
 *   first surviving entry in list order (-1: none), and at nObs <= 2 the point goes bad and all its entries die.
 *   The resident lists themselves are not changed.
 * sd_track_get_culled (synchronises; NULL outputs are skipped): verdict [n_cand], counts2 [n_cand][2] = {nRedundant, nMPs},
 *   obs_dead [n entries] = 0 live, 1 culled with its keyframe, 2 cleared because its point went bad, point_bad [n_points] = 1 iff
 *   the point went bad in this run, ref_obs (a position in the list as uploaded), n_obs = nObs, info8 = {status, n_culled,
 *   n_to_be_erased, n_entries_dead, n_points_bad, 0, 0, 0}.  status is SD_CULL_OK or a refusal, made before anything but info8 is
 *   written: SD_CULL_NOT_RESIDENT (a point that is not bad has an entry with frame -2), SD_CULL_BAD_INDEX (a frame or keypoint
 *   index that names nothing; nothing is read through it).
 * sd_track_erase_observations is queued on the tracking stream as well.  source SD_ERASE_LOCAL_BA: the obs_erase of the last
 *   sd_track_local_ba (EraseMapPointMatch + EraseObservation per flagged entry); SD_ERASE_CULL: the non-zero obs_dead of the last
 *   cull.  Either must have run on the lists as they stand (SD_ERR_INVALID_ARG otherwise); a run that refused erases nothing.
 *   nObs falls by the weight of every erased entry; a point with an erased entry and nObs <= 2 goes bad and loses every entry.
 *   The survivors are compacted stably into the list block's twin and the two are swapped: obs_off, obs_frame, obs_kp,
 *   obs_kf_bad and ref_obs hold the survivors in the caller's order (a ref_obs that died becomes the first survivor), point_bad
 *   gains the points that went bad, such a point has an empty list and ref_obs 0.  The call ends every cached result that
 *   sd_track_set_observations ends; a following sd_track_refresh_points, _local_ba, _global_ba or _cull_keyframes sees the lists
 *   as if the caller had rebuilt and uploaded them.  The getters of runs on the old lists (sd_track_get_local_ba, _get_culled)
 *   keep answering / refuse as after a sd_track_set_observations.
 * sd_track_get_erased (synchronises; NULL outputs are skipped): obs_off_new [n_points + 1], obs_map [n old entries] = the new
 *   position or -1, point_bad (the resident flags), ref_obs, n_obs (0 for a point that went bad), info8 = {0, n_entries_erased,
 *   n_points_bad, n_entries_left, 0, 0, 0, 0}.
 * sd_debug_cull_keyframes / sd_debug_erase_observations: the same kernels from host arrays, synchronous, with buffers of their
 *   own.  Per observation its keyframe obs_kf (an index into n_kf keyframes; -1: the current keyframe, -2: not resident,
 *   anything else outside [0, n_kf): a bad index), octave, stereo flag (mvuRight >= 0) and mvDepth; the CSR offsets, ref_obs and
 *   point_bad (or NULL); candidates as indices into the n_kf keyframes.  Outputs as the getters'. */
#define SD_ERASE_LOCAL_BA 0
#define SD_ERASE_CULL 1
#define SD_CULL_OK 0
#define SD_CULL_NOT_RESIDENT 1
#define SD_CULL_BAD_INDEX 2
#define SD_CULL_SKIPPED_ID0 0
#define SD_CULL_KEPT 1
#define SD_CULL_CULLED 2
#define SD_CULL_TO_BE_ERASED 3
int sd_track_cull_keyframes(sd_track* h, int n_cand, const int32_t* cand_frame, const uint8_t* cand_flags, int monocular, float th_depth);
int sd_track_get_culled(sd_track* h, uint8_t* verdict, int32_t* counts2, uint8_t* obs_dead, uint8_t* point_bad, int32_t* ref_obs,
                        int32_t* n_obs, int32_t* info8, int cap_cand, int cap_points, int cap_obs);
int sd_track_erase_observations(sd_track* h, int source);
int sd_track_get_erased(sd_track* h, int32_t* obs_off_new, int32_t* obs_map, uint8_t* point_bad, int32_t* ref_obs, int32_t* n_obs,
                        int32_t* info8, int cap_points, int cap_obs);
int sd_debug_cull_keyframes(int n_points, const int32_t* obs_off, const int32_t* obs_kf, const int32_t* obs_octave,
                            const uint8_t* obs_stereo, const float* obs_depth, const int32_t* ref_obs, const uint8_t* point_bad,
                            int n_kf, int n_cand, const int32_t* cand_kf, const uint8_t* cand_flags, int monocular, float th_depth,
                            uint8_t* verdict, int32_t* counts2, uint8_t* obs_dead, uint8_t* point_bad_out, int32_t* ref_obs_out,
                            int32_t* n_obs, int32_t* info8);
int sd_debug_erase_observations(int n_points, const int32_t* obs_off, const uint8_t* obs_stereo, const uint8_t* obs_erase,
                                const int32_t* ref_obs, const uint8_t* point_bad, int32_t* obs_off_new, int32_t* obs_map,
                                uint8_t* point_bad_out, int32_t* ref_obs_out, int32_t* n_obs, int32_t* info8);

int sd_track_align(sd_track* h, int n_frames, int mode);
int sd_track_match(sd_track* h, int n_frames, float th, int mono, int check_ori);
/* sd_track_pnp = PnPsolver(CurrentFrame, CurrentFrame.mvpMapPoints) + SetRansacParameters(...) + iterate(n_iterations)
 * (src/PnPsolver.cc:71-244); min_set 4 is the reference's default (src/PnPsolver.h:74); 3..64 are accepted (1 and 2: SD_ERR_INVALID_ARG --
 * EPnP on fewer than 3 points is pinned by nothing; 3 is pinned only as "no hypothesis is ever accepted").
 * sd_track_pnp_iterate = a further iterate(n_iterations) on those solvers: mnIterations, the best hypothesis so far and the
 * position in the rand() stream carry over (src/PnPsolver.cc:177).  The reference's solver owns copies of its inputs; here they
 * stay in the tracker, so anything that replaces them -- a new extraction on `cur`, sd_track_match / _with_motion_model /
 * _relocalize, sd_track_set_matches / _set_last / _set_rand -- ends the solvers' life: the next sd_track_pnp_iterate fails with
 * SD_ERR_INVALID_ARG until sd_track_pnp constructs new ones.  Each RANSAC iteration consumes min_set values of the
 * stream given to sd_track_set_rand; a call that could run past the supplied values fails with SD_ERR_INVALID_ARG.
 * sd_track_set_matches replaces CurrentFrame.mvpMapPoints of the slots by the caller's vector (indices into the
 * last-frame arrays, -1 = NULL; cap entries per frame, the rest NULL): PnPsolver and Optimizer::PoseOptimization take any
 * match vector, not only the one sd_track_match leaves (src/PnPsolver.cc:71-110, src/Optimizer.cc:240-330). */
int sd_track_pnp(sd_track* h, int n_frames, double probability, int min_inliers, int max_iterations,
                 int min_set, float epsilon, float th2, int n_iterations);
int sd_track_pnp_iterate(sd_track* h, int n_frames, int n_iterations);
int sd_track_set_matches(sd_track* h, int frame0, int n_frames, const int32_t* cur_match, int cap);

/* sd_track_set_poses: LastFrame.GetPose() and the current frame's prior pose (motion-model
 * prediction); sd_track_align reads the prior and leaves the aligned pose for the later stages.
 * ImageAlign results: pose written by CurrentFrame.SetPose (= the prior when ok == 0 or mode 3),
 * GetError(), the bool return, iterations per pyramid level (n x 16) and chi2_ */
int sd_track_get_align(sd_track* h, int frame0, int n_frames, double* Tcur_cm, double* error,
                       int32_t* ok, int32_t* iters, double* chi2);
/* CurrentFrame.mvpMapPoints as indices into the last-frame arrays (-1 = NULL), return value */
int sd_track_get_matches(sd_track* h, int frame0, int n_frames, int32_t* cur_match, int cap,
                         int32_t* n_matches);
/* iterate(): Tcw (4x4 CV_32F row-major; all zeros = empty Mat), vbInliers, and per frame
 * info8 = {returned(0/1), nInliers, bNoMore, iterations, N, minInliers, maxIts, refined} */
int sd_track_get_pnp(sd_track* h, int frame0, int n_frames, float* Tcw_rowmajor, uint8_t* inliers,
                     int cap, int32_t* info8);
/* diagnostics: device EPnP (PnPsolver::compute_pose, src/PnPsolver.cc:445-492) on n explicit
 * correspondences; R9 row-major, returns the mean reprojection error in *reproj_err */
/* Stage cycle counters of k_pnp (only in a library built with -DSD_PNP_PROF; tools/prof_pnp.py) */
int sd_debug_pnp_prof(unsigned long long* out32, int reset);
int sd_debug_align_prof(unsigned long long* out16, int reset); /* k_align phases */
int sd_debug_sel_prof(unsigned long long* out64, int reset);   /* out64[8 * i + 7] = k_fast_cells phase i (cycles), rest 0 */
int sd_debug_epnp(int n, const double* Xw, const double* uv, double fx, double fy, double cx, double cy,
                  double* R9, double* t3, double* reproj_err);
int sd_track_debug_read(sd_track* h, int which, int frame, void* out, size_t bytes);
/* Frame::GetFeaturesInArea(x, y, r, minLevel, maxLevel) (src/Frame.cc:271-321) answered by the device-side bucket grid of
 * current frame `frame` (Frame::AssignFeaturesToGrid, src/Frame.cc:179-192 -- the grid the matchers build): keypoint
 * indices in the reference's vIndices order; grid_counts (may be NULL) = mGrid[x][y].size(), [64][48]. */
int sd_track_debug_features_in_area(sd_track* h, int frame, float x, float y, float r, int min_level, int max_level,
                                    int32_t* indices, int cap, int32_t* n_out, int32_t* grid_counts);
/* Batched-frames mode across GPUs: the fixed-size per-frame result records -- the only data that leaves a GPU.
 * sd_track_pack_records queues, behind the tracking stages, a kernel that writes n_frames x 20 doubles {pose 4x4
 * column-major, ImageAlign ok, nmatches, pose-solver inliers, pose-solver ok} into a caller-owned DEVICE buffer; source =
 * 0 PnPsolver / 1 PoseOptimization / 2 TrackWithMotionModel / 3 TrackLocalMap / 4 ImageAlign only.
 * sd_track_stream_fence orders the tracking stream against a caller's hipStream_t (the stream of its RCCL collective):
 * direction 0 = that stream waits for the tracking stream, 1 = the tracking stream waits for that stream. */
int sd_track_pack_records(sd_track* h, int n_frames, int source, void* d_records);

/* ------------------------------------------------------------------------------------------
 * Sequential tracking: B camera streams tracked frame after frame, the hand-off on the device
 *   mLastFrame = Frame(mCurrentFrame)             src/Tracking.cc:292, after
 *     "Clean VO matches" (Observations() < 1)     src/Tracking.cc:250-257
 *     outliers discarded                          src/Tracking.cc:272-275
 *   mnLastFrameSeen skip of SearchLocalPoints     src/Tracking.cc:703, :900-918
 *   ConstantVelocity::GetPose  Exp(vel) * last_pose_ (the prior: from the caller through sd_track_set_prior, or from the
 *     device's own motion model, below)
 * One frame per call on every slot:
 *   extract into sd_track_get_extractors' cur -> sd_track_set_prior | sd_track_motion_predict -> sd_track_with_motion_model ->
 *   [sd_track_local_map] -> [sd_track_motion_update] -> sd_track_advance.
 * sd_track_set_map_ids: the caller's identity of every map point, which = 0 last-frame arrays, 1 local-map arrays, [n][cap]
 *   rows (cap <= max_points, the rest -1), -1 = none.  sd_track_set_last resets the last-frame ids of its slots to -1.  Once ids
 *   are set, sd_track_local_map skips a local point whose id equals the id of a last-frame point that the final search of
 *   sd_track_with_motion_model (run on this extraction) matched, before or after its outlier discard: the `cand` flags no
 *   longer have to exclude them.  Points without ids (-1) are never skipped, so without ids nothing changes.
 * sd_track_advance: for every slot < n_frames and current keypoint i < N, the last frame's point i becomes mvpMapPoints[i]
 *   (source 0: after sd_track_with_motion_model's discard; 1: after sd_track_local_map, local points included, mvbOutlier
 *   dropped; 2: after sd_track_stereo_init, the created points only, Tref = the identity), kept iff it has Observations()
 *   >= 1, with its Xw / descriptor / obs / id; octave = mvKeys[i].octave, angle =
 *   mvKeysUn[i].angle; n_last = N; Tref = the frame's final pose (the prior when no pose solve ran).  Slots >= n_frames keep
 *   their last frame.  Then the cur / ref extractors swap roles (this frame's pyramid and keypoints are the next reference):
 *   extract the next frame into the new cur.  Queued on the tracking stream; that extraction waits for the kernels that
 *   still read the set it overwrites.  SD_ERR_CAPACITY: keypoint capacity > max_points; SD_ERR_INVALID_ARG: the call named
 *   by `source` has not run since the last extraction, or broadcast mode is on.
 * sd_track_set_prior: Tprior = Tcur = T (relative 0) or T * Tref computed on the device (relative 1; each entry sums k = 0..3
 *   in order, without FMA contraction), column-major, queued on the tracking stream without a host wait.  Tref is left alone.
 * sd_track_get_last: the last-frame arrays in [n][max_points] layout; any pointer may be NULL.
 * sd_track_get_extractors: the handles in the cur / ref roles now.
 * sd_track_close_points: the RGB-D counts of Tracking::NeedNewKeyFrame (src/Tracking.cc:776-789) for slots < n_frames, queued
 *   on the tracking stream without a host wait.  Over keypoints i < N with 0 < mvDepth[i] < th_depth (mThDepth = mbf * ThDepth
 *   / fx, passed in), a keypoint is tracked when sd_track_advance with the same
 *   `source` would keep its map point (after "Clean VO matches": present, Observations() >= 1, not an outlier), non-tracked
 *   otherwise.  SD_ERR_CAPACITY: n_frames > max_batch; SD_ERR_INVALID_ARG: a bad source, the call named by `source` has not
 *   run on these slots since the last extraction, or broadcast mode is on.  Slots >= n_frames keep their counts.
 *   Precondition (not checked): mvDepth of this extraction has been computed by sd_track_stereo_from_depth(_device) before
 *   the call; otherwise the counts read whatever depth the slots last received (-1 everywhere for a new handle).
 * sd_track_get_close_points: out2 = [n_frames][2] {nTrackedClose, nNonTrackedClose}; synchronises. */
int sd_track_set_map_ids(sd_track* h, int frame0, int n_frames, int which, const int32_t* ids, int cap);
int sd_track_advance(sd_track* h, int n_frames, int source);
int sd_track_set_prior(sd_track* h, int frame0, int n_frames, const double* T_cm, int relative);
int sd_track_get_last(sd_track* h, int frame0, int n_frames, int32_t* n_last, uint8_t* valid, double* Xw, uint8_t* desc, int32_t* octave,
                      float* angle, int32_t* obs, int32_t* ids);
int sd_track_get_extractors(sd_track* h, sd_orb** cur, sd_orb** ref);
int sd_track_close_points(sd_track* h, int n_frames, int source, float th_depth);
int sd_track_get_close_points(sd_track* h, int frame0, int n_frames, int32_t* out2);

/* Motion model on the device: EKF + ConstantVelocity as per-slot state of the tracker, so the prior needs no host pose
 *   EKF::Predict / Update / Restart               src/sensors/EKF.cc:44-66, :68-104, :106-109
 *   ConstantVelocity (Init, Q, R, Z, Exp, Log)    src/sensors/ConstantVelocity.cc:34-46, :83-122, :151-263
 *   COV_V_2, COV_W_2, SIGMA_V, SIGMA_W            src/sensors/Sensor.cc:24-32
 *   motion_model_->Predict(mLastFrame.GetPose())  src/Tracking.cc:661
 *   motion_model_->Update / Restart               src/Tracking.cc:243-247, :221, :226
 * Per slot: X (v, w), the diagonal of P (jF = jH = G = I and Q, R, the initial P are diagonal, so the reference's dense P, S and
 *   K stay exactly diagonal: six scalar filters), started (EKF::Started()), it_time, last_pose (Sensor::SetLastPose) and the
 *   last E = Exp(X).  A new handle: started 0, X = 0, P = diag(COV_V_2 x3, COV_W_2 x3).
 * sd_track_motion_predict: for slots < n_frames, it_time = started ? dt : 0; last_pose = Tref; P += Q(it_time);
 *   Tprior = Tcur = Exp(X) * Tref through the product of sd_track_set_prior (k = 0..3 in order, no FMA contraction).  Tref is
 *   left alone.  dt stands for the reference's wall-clock timer: one value for all slots of the step, which advance in
 *   lock-step; per-slot timestamps are not supported.  A slot that is not started has X = 0, Exp(0) = I and so Tprior = Tref
 *   bit for bit: the pose TrackReferenceKeyFrame starts from, which keeps the batch uniform.
 * sd_track_motion_update: for slots < n_frames; a slot is tracked when source 0: sd_track_with_motion_model left status 2,
 *   1: sd_track_local_map left status 2, -1: always (the caller vouches: its own pose solve).  Tracked and last_pose not zero
 *   (Matrix4d::isZero(): every |entry| <= 1e-12): EKF::Update with the frame's final pose Tcur, Z = Log(Tcur *
 *   inverse(last_pose)); the first update after a start only sets started (InitState: X = 0).  Otherwise EKF::Restart
 *   (started 0, X = 0, the diagonal of P to its initial values).  Call it before sd_track_advance.
 * sd_track_motion_restart: EKF::Restart for slots frame0 .. frame0 + n_frames - 1.
 *   These three are queued on the tracking stream behind the calls whose results they read: no host wait, no allocation.
 * sd_track_get_motion: [n][6] X, [n][6] diagonal of P, [n] started, [n] it_time, [n][16] E and last_pose column-major; any
 *   pointer may be NULL; synchronises.  sd_track_set_motion: restores X / P / started / it_time of a stream's filter (NULL:
 *   left alone); synchronises.
 * Slots >= n_frames keep their state and prior.  sd_track_set_prior stays: either call may set the prior of a frame.
 * Errors: SD_ERR_CAPACITY for n_frames > max_batch; SD_ERR_INVALID_ARG for a source outside -1..1, a dt that is negative or not
 *   finite, broadcast mode, or when the call named by `source` (0 / 1) has not run on these slots since the last extraction.
 * Not covered (the caller's, with the statuses that name the slots): running TrackReferenceKeyFrame's (Frame, KeyFrame)
 *   overloads for slots that are not started or just relocalised (src/Tracking.cc:215-216), its retry after a failed
 *   TrackWithMotionModel (:219-222), and Relocalization.  The IMU sensor model is the other value of
 *   sd_track_set_sensor_model, below; everything in this comment describes SD_SENSOR_CONSTANT_VELOCITY, the default. */
int sd_track_motion_predict(sd_track* h, int n_frames, double dt);
int sd_track_motion_update(sd_track* h, int n_frames, int source);
int sd_track_motion_restart(sd_track* h, int frame0, int n_frames);
int sd_track_get_motion(sd_track* h, int frame0, int n_frames, double* X6, double* Pdiag6, int32_t* started, double* it_time,
                        double* E_cm, double* last_pose_cm);
int sd_track_set_motion(sd_track* h, int frame0, int n_frames, const double* X6, const double* Pdiag6, const int32_t* started,
                        const double* it_time);

/* IMU sensor model on the device: the 16-state EKF of Monocular-IMU tracking (System::MONOCULAR_IMU, System::TrackFusion,
 * Tracking::SetMeasurements) as per-slot state, chosen per handle as Tracking chooses its Sensor (src/Tracking.cc:134-138)
 *   EKF::Predict / Update / Restart               src/sensors/EKF.cc:44-109
 *   IMU (Init, InitState, F, jF, Q, Z, H, jH, R, UpdateGravity)   src/sensors/IMU.cc:26-240
 *   Sensor (GetPose, PoseToVector, QuaternionFromAngularVelocity, QuaternionJacobian(Right), dq_by_dw)   src/sensors/Sensor.cc:24-159
 * Per slot: X[16] = (x, q as w x y z, v, w, a), the dense P[16][16] row-major, gravity_[3], started, it_time, last_pose and
 *   the last measurements [6] = (gyro xyz, accelerometer xyz); about 2.3 KB, allocated with the tracker.  A new handle: model
 *   SD_SENSOR_CONSTANT_VELOCITY; IMU state started 0, X = (0, 1 0 0 0, 0, 0, 0), P = diag(COV_X_2 x3, COV_Q_2 x4, COV_V_2 x3,
 *   COV_W_2 x3, COV_A_2 x3), gravity_ = 0.
 * sd_track_set_sensor_model: the filter that sd_track_motion_predict / _update / _restart run from now on.  Every slot's
 *   filter of the chosen model restarts (a new Tracking constructs a new EKF), and under SD_SENSOR_IMU every slot's
 *   measurements count as not set.  With SD_SENSOR_CONSTANT_VELOCITY every call behaves as described above.
 * Under SD_SENSOR_IMU:
 *   sd_track_motion_predict, slots < n_frames: last_pose = Tref.  A started slot: it_time = dt; jF and Q on the old X, then
 *     X = F(X), P = jF P jF^T + Q, Tprior = Tcur = Sensor::GetPose(X) -- the filter's own absolute pose (the rotation of a
 *     normalised copy of q, and x), not a product with Tref.  A slot that is not started is not predicted: the reference never
 *     calls Predict for it (it runs TrackReferenceKeyFrame from the last pose), so Tprior = Tcur = Tref bit for bit, X and P
 *     are left alone and it_time = 0 -- the same convention as the constant-velocity model.
 *   sd_track_motion_update, slots < n_frames: tracked (source as above) and last_pose not zero: EKF::Update with the pose in
 *     Tcur and the slot's stored measurements -- Z = (x, normalised q of the pose, gyro, accelerometer - gravity_) after
 *     UpdateGravity(it_time); the first update after a start is InitState (X = the pose part of Z, zeros elsewhere, gravity_ =
 *     0, P left alone).  Otherwise EKF::Restart = IMU::Init, gravity_ = 0 included; IMU::Init assigns the five diagonal
 *     blocks of P (x, q, v, w, a) and leaves the off-diagonal blocks as they are, so only a filter that never updated, or
 *     one sd_track_set_sensor_model rebuilt, has all of them zero.  The reference's quirks are kept: P = P -
 *     K S K^T without symmetrisation, quaternions subtracted componentwise in Y = Z - h(X), R = sigma^2 it_time^2 (zero for dt
 *     = 0), the state's q never normalised.  S^-1 is a Gauss-Jordan inverse with partial pivoting.
 *   sd_track_motion_restart: EKF::Restart for its range.  Measurements, it_time and last_pose stay.
 *   sd_track_set_measurements: Tracking::SetMeasurements for slots frame0 .. frame0 + n_frames - 1, [n][6] doubles (gyro xyz,
 *     accelerometer xyz); they persist until replaced, as the reference's vector does.  Queued on the tracking stream through
 *     the pinned ring of sd_track_set_prior: no host wait, no allocation.
 *   sd_track_get_imu: [n][16] X, [n][256] P, [n][3] gravity_, [n] started, [n] it_time, [n][16] last_pose column-major, [n][6]
 *     measurements; any pointer may be NULL; synchronises.  sd_track_set_imu restores X / P / gravity_ / started / it_time
 *     (NULL: left alone); synchronises.
 * Slots >= n_frames keep everything.  Errors, all leaving state untouched: SD_ERR_INVALID_ARG for an unknown model;
 *   sd_track_set_measurements or sd_track_set_imu under SD_SENSOR_CONSTANT_VELOCITY; sd_track_get_motion / _set_motion under
 *   SD_SENSOR_IMU; measurements that are not finite; sd_track_motion_update under SD_SENSOR_IMU for slots whose measurements
 *   have not been set since the model was chosen (the reference asserts there); and everything the motion calls refuse above.
 * Not covered: per-slot timestamps, orientation filters (Madgwick), and what the constant-velocity model leaves to the caller. */
#define SD_SENSOR_CONSTANT_VELOCITY 0
#define SD_SENSOR_IMU 1
int sd_track_set_sensor_model(sd_track* h, int model);
int sd_track_get_sensor_model(sd_track* h, int* model);
int sd_track_set_measurements(sd_track* h, int frame0, int n_frames, const double* wa6);
int sd_track_get_imu(sd_track* h, int frame0, int n_frames, double* X16, double* P256, double* gravity3, int32_t* started, double* it_time,
                     double* last_pose_cm, double* measurements6);
int sd_track_set_imu(sd_track* h, int frame0, int n_frames, const double* X16, const double* P256, const double* gravity3,
                     const int32_t* started, const double* it_time);
int sd_track_stream_fence(sd_track* h, void* hip_stream, int direction);
int sd_track_set_profiling(sd_track* h, int on);
int sd_track_stage_ms(sd_track* h, float* ms_out /* [0]=align, [1]=match, [2]=pnp */, int cap);

/* ------------------------------------------------------------------------------------------
 * RGB-D map points created on the device, so B streams bootstrap, track, decide and refill their points without a host wait
 *   Tracking::StereoInitialization                src/Tracking.cc:302-349
 *   Tracking::NeedNewKeyFrame                     src/Tracking.cc:753-826
 *   Tracking::CreateNewKeyFrame, RGB-D part       src/Tracking.cc:837-888, mnLastKeyFrameId :894
 *   Frame::UnprojectStereo                        src/Frame.cc:419-431
 * Per frame:  ... -> sd_track_local_map -> sd_track_close_points -> sd_track_need_keyframe ->
 *   sd_track_create_keyframe_points(use_flags = 1) -> sd_track_advance; frame 0: extract, depth, sd_track_stereo_init,
 *   sd_track_advance(source = 2).  All calls but the two getters are queued on the tracking stream without a host wait; the
 *   small host arrays travel through a ring of pinned buffers like sd_track_set_prior's.
 * sd_track_set_next_map_id: MapPoint::nNextId per slot; created points get next_id, next_id + 1, ... in creation order and the
 *   device advances it (0 for a new handle).
 * sd_track_stereo_init: a slot with N = min(keypoints, capacity) > min_keypoints (reference: 500) sets its pose (Tcur) to the
 *   identity and gives every keypoint with mvDepth > 0 a point, ids in keypoint order.  Other slots create nothing (info mode 0)
 *   and sd_track_advance(source 2) leaves their last frame alone.
 * sd_track_set_keyframe_state: state8 = [n][8] int32 {nKFs = KeyFramesInMap(), nRefMatches = mpReferenceKF->
 *   TrackedMapPoints(nMinObs), mnLastKeyFrameId, mnLastRelocFrameId, flags, 3 reserved}; flags bit 0 AcceptKeyFrames() (mapper
 *   idle), bit 1 isStopped() || stopRequested(), bit 2 KeyframesInQueue() < 3, bit 3 usePattern (enters nMinObs, which the caller
 *   applied to nRefMatches: not read).  An entry equal to SD_KF_KEEP leaves the device's value: sd_track_create_keyframe_points
 *   writes mnLastKeyFrameId itself.  nKFs and nRefMatches come from the KeyFrame graph and stay the caller's.
 * sd_track_need_keyframe: the decision for slots < n_frames as one byte per slot: bit 0 insert a keyframe, bit 1 the conditions
 *   held but the mapper is busy (where the reference calls InterruptBA; bit 0 is then KeyframesInQueue() < 3 for RGB-D).  Reads
 *   mnMatchesInliers of sd_track_local_map and, for rgbd, the counts of sd_track_close_points(source 1): both must have run on
 *   this extraction.  mnMatchesInliers < nRefMatches * 0.25 compares in double, < nRefMatches * thRefRatio in float (0.75f, 0.4f
 *   for nKFs < 2, 0.9f when not rgbd).  A slot that is not tracked gets 0.
 * sd_track_set_keyframe_flags / sd_track_get_keyframe_flags: the same bytes from / to the host (the getter synchronises).
 * sd_track_create_keyframe_points: for every slot < n_frames that the call named by `source` (as in sd_track_advance) left
 *   tracked and, with use_flags, whose flag bit 0 is set: keypoints with mvDepth > 0 sorted by (depth, index); the prefix up to
 *   and including the first entry beyond th_depth (mThDepth) past the 100th is processed, and each of its keypoints that holds no
 *   map point with Observations() >= 1 -- outlier flags not consulted, :861-867 -- gets a new point: Xw = UnprojectStereo from
 *   the frame's final pose, Observations() = 1, the keypoint's descriptor, the next id.  mnLastKeyFrameId of the slot = frame_id.
 *   The depth sort holds 2048 keys: SD_ERR_CAPACITY for a larger keypoint capacity.  UnprojectStereo: x = (u - cx) * z * invfx
 *   in float, then Xw[r] = ((Rwc[r][0] * x + Rwc[r][1] * y) + Rwc[r][2] * z) + Ow[r], Ow[r] = -((Rwc[r][0] * t0 + Rwc[r][1] *
 *   t1) + Rwc[r][2] * t2) in double, every operation rounded on its own.
 *   A following sd_track_advance(source) hands each created point to the next frame in place of whatever the keypoint held.
 *   The depth precondition is sd_track_close_points'.  A second creation call on one extraction replaces the first one's
 *   record but has already advanced the ids.
 * sd_track_get_created: per slot info4 = {mode (0 nothing created on the slot, 1 keyframe, 2 initialisation), created, P =
 *   processed prefix (candidates for mode 2), candidates}, and [n][cap] rows in creation order: keypoint index, Xw ([n][cap][3]),
 *   id; any of the three may be NULL.  Synchronises.  info4 is written even when the call returns SD_ERR_CAPACITY.  KeyFrame construction, InsertKeyFrame and later observations stay with
 *   the caller.
 * Errors: SD_ERR_INVALID_ARG for a bad source, when the call named by `source` (sd_track_need_keyframe: sd_track_local_map and
 *   sd_track_close_points) has not run since the extraction, or in broadcast mode; SD_ERR_CAPACITY for n_frames > max_batch or
 *   a cap smaller than a slot's number of created points. */
#define SD_KF_KEEP INT32_MIN
int sd_track_set_next_map_id(sd_track* h, int frame0, int n_frames, const int32_t* next_id);
int sd_track_stereo_init(sd_track* h, int n_frames, int min_keypoints);
int sd_track_set_keyframe_state(sd_track* h, int frame0, int n_frames, const int32_t* state8);
int sd_track_need_keyframe(sd_track* h, int n_frames, int rgbd, int frame_id, int min_frames, int max_frames);
int sd_track_set_keyframe_flags(sd_track* h, int frame0, int n_frames, const uint8_t* flags);
int sd_track_get_keyframe_flags(sd_track* h, int frame0, int n_frames, uint8_t* flags);
int sd_track_create_keyframe_points(sd_track* h, int n_frames, int source, float th_depth, int use_flags, int frame_id);
int sd_track_get_created(sd_track* h, int frame0, int n_frames, int32_t* info4, int32_t* kp_index, double* Xw, int32_t* ids, int cap);

/* ------------------------------------------------------------------------------------------
 * ORBmatcher::DescriptorDistance -- src/ORBmatcher.h:44, src/ORBmatcher.cc:1459-1473
 * (pure host function; kept in the ABI so callers need no second library)
 * ------------------------------------------------------------------------------------------ */
int sd_hamming(const uint8_t* a32, const uint8_t* b32);

#ifdef __cplusplus
}
#endif
#endif /* SDSLAM_HIP_H_ */
