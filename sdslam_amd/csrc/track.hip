// sd_track_*: batched TrackWithMotionModel context (ImageAlign -> SearchByProjection -> pose solve)
// over two resident extractor handles (current frames, last frames).  Host side only; the
// kernels live in track_align.hip / track_match.hip / track_pnp.hip / track_poseopt.hip.
// Besides the stage calls: whole-function calls that keep the reference's per-frame decisions on
// the device (sd_track_with_motion_model, sd_track_local_map) and the one-frame-against-all-
// keyframes calls (sd_track_relocalize, sd_track_detect_loop) built on the broadcast current frame.
// The sequential loop around them (hand-off, keyframes, new points, motion models) is track_seq.hip; the handle itself and the
// helpers both files share are track_handle.h.
//
// Call sequence of the reference this mirrors (src/Tracking.cc:654-718):
//   ImageAlign::ComputePose(cur, last)            -> sd_track_align
//   ORBmatcher(0.9,true).SearchByProjection(...)  -> sd_track_match
//   pose solve (PnPsolver per BASELINE; the reference calls Optimizer::PoseOptimization, D1)
//                                                 -> sd_track_pnp
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "track_handle.h"

using namespace sd;

// Per-frame result record (the only data that crosses xGMI in the batched-frames mode), 20 doubles:
// pose 4x4 column-major | ImageAlign ok | nmatches | pose-solver inliers | pose-solver ok
//   source 0: PnPsolver (pose = Tcw it returned, zeros for an empty Mat)   1: PoseOptimization (ok = nGood >= 10)
//   source 2: TrackWithMotionModel (inliers = nmatchesMap, ok = tracked)   3: TrackLocalMap (mnMatchesInliers, tracked)
//   source 4: ImageAlign only (pose = the aligned pose)
__global__ void k_pack_records(TrackBuffers tb, int source, int n_frames, double* __restrict__ out) {
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= n_frames) return;
  double* r = out + (size_t)f * 20;
  if (source == 0) {
    const float* T = tb.pnp_T + (size_t)f * 16;   // row-major CV_32F
    for (int c = 0; c < 4; c++)
      for (int rr = 0; rr < 4; rr++) r[c * 4 + rr] = (double)T[rr * 4 + c];
  } else {
    const double* T = (source == 4 ? tb.Tcur : tb.po_T) + (size_t)f * 16;
    for (int i = 0; i < 16; i++) r[i] = T[i];
  }
  r[16] = (double)tb.al_ok[f];
  r[17] = (double)tb.n_matches[f];
  double inl = 0, ok = 0;
  if (source == 0) { inl = tb.pnp_info[(size_t)f * 8 + 1]; ok = tb.pnp_info[(size_t)f * 8]; }
  else if (source == 1) { inl = tb.po_info[(size_t)f * 8 + 5]; ok = inl >= 10; }
  else if (source == 2) { inl = tb.tw_info[(size_t)f * 4 + 2]; ok = tb.tw_info[(size_t)f * 4] == 2; }
  else if (source == 3) { inl = tb.tl_info[(size_t)f * 4 + 2]; ok = tb.tl_info[(size_t)f * 4] == 2; }
  else { ok = tb.al_ok[f]; }
  r[18] = inl;
  r[19] = ok;
}

// What a buffer holds when sd_track_create returns: zeros | 0xFF bytes (-1 in an int32) | -1.f in every float
enum Fill { FILL_ZERO, FILL_FF, FILL_MINUS_ONE };

// The fill runs on the null stream: sd_track_create waits for it before it queues anything that reads a buffer
template <Fill F = FILL_ZERO, typename T>
static int dalloc(sd_track* h, T** p, size_t count) {
  static_assert(F != FILL_MINUS_ONE || std::is_same<T, float>::value, "FILL_MINUS_ONE is a float value");
  const size_t n = std::max<size_t>(count, 1);
  void* q = nullptr;
  SD_HIP_CHECK(hipMalloc(&q, n * sizeof(T)));
  h->allocs.push_back(q);
  if (F == FILL_MINUS_ONE) SD_HIP_CHECK(hipMemsetD32(q, (int)0xBF800000u /* -1.f */, n));
  else SD_HIP_CHECK(hipMemset(q, F == FILL_FF ? 0xFF : 0, n * sizeof(T)));
  *p = (T*)q;
  return SD_OK;
}

// Run `stages` with every slot paired to frame `cur_frame` of the cur extractor (sd_track_set_current_broadcast), and put the
// caller's pairing back whatever they return
template <typename Stages>
static int with_broadcast(sd_track* h, int cur_frame, Stages&& stages) {
  const int saved = h->tb.cur_bcast;
  SD_TRY(sd_track_set_current_broadcast(h, cur_frame));
  const int rc = stages();
  h->tb.cur_bcast = saved;
  return rc;
}

extern "C" {

int sd_track_create(sd_orb* cur, sd_orb* ref, int max_points, int max_batch, int pnp_max_iterations, sd_track** out) {
  SD_REQUIRE(out, SD_ERR_INVALID_ARG, "out is NULL");
  *out = nullptr;
  SD_REQUIRE(cur && ref, SD_ERR_INVALID_ARG, "extractor handle is NULL");
  SD_REQUIRE(cur->device == ref->device && cur->nlevels == ref->nlevels && cur->scaleFactor == ref->scaleFactor,
             SD_ERR_INVALID_ARG, "cur/ref extractors must share device and pyramid parameters");
  // `cur` may hold fewer frames than the tracker has slots: one current frame against many keyframes
  // (sd_track_set_current_broadcast); slot-paired calls then check their n_frames against what `cur` extracted
  SD_REQUIRE(max_points >= 1 && max_points <= 2048 && max_batch >= 1 && max_batch <= ref->max_batch, SD_ERR_INVALID_ARG,
             "bad capacities (max_points <= 2048, max_batch <= the ref extractor's max_batch)");
  SD_REQUIRE(pnp_max_iterations >= 1 && pnp_max_iterations <= 4096, SD_ERR_INVALID_ARG, "bad pnp_max_iterations");
  const int nsel = keypoint_capacity(cur);
  SD_REQUIRE(nsel >= 1 && nsel <= 2048, SD_ERR_INVALID_ARG, "tracking supports at most 2048 keypoints per frame");
  SD_HIP_CHECK(hipSetDevice(cur->device));
  sd_track* h = new sd_track();
  h->cur = cur;
  h->ref = ref;
  h->max_points = max_points;
  h->max_batch = max_batch;
  h->kp_cap = nsel;
  h->device = cur->device;
  h->rand_per_frame = 4 * pnp_max_iterations;
  h->rand_len.assign((size_t)max_batch, 0);
  h->meas_set.assign((size_t)max_batch, 0);
  h->f12_set.assign((size_t)max_batch, 0);
  h->scw_set.assign((size_t)max_batch, 0);
  const size_t B = max_batch, M = max_points, K = nsel;
  TrackBuffers& tb = h->tb;
  tb.max_points = max_points;
  tb.kp_cap = nsel;
  tb.cur_bcast = -1;
  // FILL_FF on the match / seen arrays: "no map point" until a search has run (a TrackLocalMap / PoseOptimization called first
  // must not see index 0 everywhere); on the id arrays: no ids, the seen-point exclusion never fires and the hand-off carries -1
  int rc = SD_OK;
  auto A = [&](int r) { if (rc == SD_OK) rc = r; };
  A(dalloc(h, &tb.valid, B * M));
  A(dalloc(h, &tb.Xw, B * M * 3));
  A(dalloc(h, &tb.mp_desc, B * M * 32));
  A(dalloc(h, &tb.octave, B * M));
  A(dalloc(h, &tb.angle, B * M));
  A(dalloc(h, &tb.obs, B * M));
  A(dalloc(h, &tb.n_last, B));
  A(dalloc<FILL_FF>(h, &tb.last_id, B * M));
  A(dalloc(h, &tb.valid2, B * M));
  A(dalloc(h, &tb.Xw2, B * M * 3));
  A(dalloc(h, &tb.mp_desc2, B * M * 32));
  A(dalloc(h, &tb.octave2, B * M));
  A(dalloc(h, &tb.angle2, B * M));
  A(dalloc(h, &tb.obs2, B * M));
  A(dalloc<FILL_FF>(h, &tb.last_id2, B * M));
  A(dalloc<FILL_FF>(h, &tb.tw_seen, B * K));
  A(dalloc(h, &tb.tw_seen_ids, B * K));
  A(dalloc<FILL_FF>(h, &tb.lm_id, B * M));
  A(dalloc(h, &h->d_prior, B * 16));
  A(dalloc(h, &h->d_close, B * 2));
  A(dalloc(h, &tb.np_flag, B * K));
  A(dalloc(h, &tb.np_Xw, B * K * 3));
  A(dalloc(h, &tb.np_id, B * K));
  A(dalloc(h, &tb.np_list, B * K));
  A(dalloc(h, &tb.np_info, B * 4));
  A(dalloc(h, &tb.next_id, B));
  A(dalloc(h, &tb.kf_state, B * 8));
  A(dalloc(h, &tb.kf_flags, B));
  A(dalloc(h, &h->d_kf_stage, B * 8));
  A(dalloc(h, &tb.mo_X, B * 6));
  A(dalloc(h, &tb.mo_P, B * 6));
  A(dalloc(h, &tb.mo_started, B));
  A(dalloc(h, &tb.mo_it, B));
  A(dalloc(h, &tb.mo_last, B * 16));
  A(dalloc(h, &tb.mo_E, B * 16));
  A(dalloc(h, &tb.im_X, B * 16));
  A(dalloc(h, &tb.im_P, B * 256));
  A(dalloc(h, &tb.im_g, B * 3));
  A(dalloc(h, &tb.im_started, B));
  A(dalloc(h, &tb.im_it, B));
  A(dalloc(h, &tb.im_last, B * 16));
  A(dalloc(h, &tb.im_meas, B * 6));
  A(dalloc(h, &tb.Tref, B * 16));
  A(dalloc(h, &tb.Tprior, B * 16));
  A(dalloc(h, &tb.Tcur, B * 16));
  A(dalloc(h, &tb.al_ok, B));
  A(dalloc(h, &tb.al_err, B));
  A(dalloc(h, &tb.al_chi2, B));
  A(dalloc(h, &tb.al_iters, B * 16));
  A(dalloc<FILL_FF>(h, &tb.cur_match, B * K));
  A(dalloc(h, &tb.n_matches, B));
  A(dalloc(h, &tb.mt_list, B * 8192));
  A(dalloc(h, &tb.mt_pt, B * M));
  A(dalloc(h, &tb.mt_key, B * 2048));
  A(dalloc(h, &tb.mt_cstart, B * (64 * 48 + 4)));
  A(dalloc(h, &tb.retry_list, B + 1));
  A(dalloc<FILL_MINUS_ONE>(h, &tb.uright, B * K));
  A(dalloc<FILL_MINUS_ONE>(h, &tb.depth, B * K));
  A(dalloc(h, &tb.rand_stream, B * (size_t)h->rand_per_frame));
  A(dalloc(h, &tb.pnp_T, B * 16));
  A(dalloc(h, &tb.pnp_inliers, B * K));
  A(dalloc(h, &tb.pnp_info, B * 8));
  A(dalloc(h, &tb.pnp_scratch, B * K * 5));
  A(dalloc(h, &tb.pnp_pts, B * K * 6));
  A(dalloc(h, &tb.pnp_kpidx, B * K));
  A(dalloc(h, &tb.pnp_state, B * 4));
  A(dalloc(h, &tb.pnp_best_mask, B * 32));
  A(dalloc(h, &tb.pnp_best_T, B * 12));
  A(dalloc(h, &tb.sp_valid1, B * K));
  A(dalloc(h, &tb.sp_valid2, B * K));
  A(dalloc(h, &tb.sp_match, B * K));
  A(dalloc(h, &tb.sp_n, B));
  A(dalloc<FILL_MINUS_ONE>(h, &tb.uright_ref, B * K));
  A(dalloc(h, &tb.tri_F12_set, B * 9));
  A(dalloc(h, &tb.tri_F12, B * 9));
  A(dalloc(h, &tb.tri_epi, B * 2));
  A(dalloc<FILL_FF>(h, &tb.tri_match, B * K));
  A(dalloc(h, &tb.tri_n, B));
  A(dalloc<FILL_MINUS_ONE>(h, &h->nb.depth_ref, B * K));
  A(dalloc<FILL_MINUS_ONE>(h, &h->nb.median, B));
  A(dalloc(h, &h->nb.verdict, B * K));
  A(dalloc(h, &h->nb.branch, B * K));
  A(dalloc(h, &h->nb.Xw, B * K * 3));
  A(dalloc(h, &h->nb.count, B * 2));
  A(dalloc(h, &h->nb.info, 4));
  A(dalloc(h, &h->nb.pt, B * K * 4));
  A(dalloc(h, &h->nb.geo, B * K * 6));
  A(dalloc(h, &h->nb.dist, B * K * 2));
  A(dalloc(h, &h->nb.desc, B * K * 32));
  A(dalloc(h, &h->nb.appended, B * 3));
  A(dalloc(h, &h->fu.Scw, B * 16));
  A(dalloc(h, &h->fu.pose, B * 15));
  A(dalloc<FILL_FF>(h, &h->fu.idx, B * M));
  A(dalloc(h, &h->fu.dist, B * M));
  A(dalloc(h, &h->fu.n, B));
  A(dalloc(h, &h->rf.centre, (B + 1) * 3));
  A(dalloc(h, &h->rf.status, M));
  A(dalloc(h, &h->rf.best_obs, M));
  A(dalloc(h, &h->rf.best_median, M));
  A(dalloc(h, &h->rf.desc, M * 32));
  A(dalloc(h, &h->rf.normal, M * 3));
  A(dalloc(h, &h->rf.max_dist, M));
  A(dalloc(h, &h->rf.min_dist, M));
  A(refresh_create(h));
  A(ba_create(h));
  A(cull_create(h));
  A(dalloc(h, &tb.s3_Xw1, B * K * 3));
  A(dalloc(h, &tb.s3_Xw2, B * K * 3));
  A(dalloc(h, &tb.s3_X, B * K * 6));
  A(dalloc(h, &tb.s3_F, B * K * 6));
  A(dalloc(h, &tb.s3_idx, B * K));
  A(dalloc(h, &tb.s3_state, B * 8));
  A(dalloc(h, &tb.s3_best_mask, B * 32));
  A(dalloc(h, &tb.s3_bestT, B * 16));
  A(dalloc(h, &tb.s3_R, B * 9));
  A(dalloc(h, &tb.s3_t, B * 3));
  A(dalloc(h, &tb.s3_s, B));
  A(dalloc(h, &tb.s3_T, B * 16));
  A(dalloc(h, &tb.s3_inliers, B * K));
  A(dalloc(h, &tb.s3_info, B * 8));
  A(dalloc(h, &h->d_sim3_max_its, K + 1));
  A(dalloc(h, &tb.lm_cand, B * M));
  A(dalloc(h, &tb.lm_Xw, B * M * 3));
  A(dalloc(h, &tb.lm_normal, B * M * 3));
  A(dalloc(h, &tb.lm_min, B * M));
  A(dalloc(h, &tb.lm_max, B * M));
  A(dalloc(h, &tb.lm_mfmax, B * M));
  A(dalloc(h, &tb.lm_desc, B * M * 32));
  A(dalloc(h, &tb.lm_obs, B * M));
  A(dalloc(h, &tb.lm_n, B));
  A(dalloc(h, &tb.lm_kclaim, B * K));
  A(dalloc(h, &tb.lm_inview, B * M));
  A(dalloc(h, &tb.lm_proj, B * M * 3));
  A(dalloc(h, &tb.lm_level, B * M));
  A(dalloc(h, &tb.lm_cos, B * M));
  A(dalloc<FILL_FF>(h, &tb.lm_match, B * K));
  A(dalloc(h, &tb.lm_nmatch, B));
  A(dalloc(h, &tb.po_T, B * 16));
  A(dalloc(h, &tb.po_outlier, B * K));
  A(dalloc(h, &tb.po_info, B * 8));
  A(dalloc(h, &tb.tw_info, B * 4));
  A(dalloc<FILL_FF>(h, &tb.un_match, B * K));
  A(dalloc(h, &tb.tl_info, B * 4));
  A(dalloc(h, &h->d_inv_sigma2, (size_t)cur->nlevels));
  A(dalloc(h, &h->d_scale_thr, (size_t)SD_MAX_LEVELS));
  A(dalloc(h, &h->d_sf, (size_t)cur->nlevels));
  A(dalloc(h, &h->d_inv_sf, (size_t)cur->nlevels));
  A(dalloc(h, &h->d_sigma2, (size_t)cur->nlevels));
  if (rc == SD_OK) {
    hipError_t e = hipSuccess;
    auto table = [&](float* dst, const float* src) {
      if (e == hipSuccess) e = hipMemcpy(dst, src, cur->nlevels * sizeof(float), hipMemcpyHostToDevice);
    };
    table(h->d_sf, cur->hp.sf.data());
    table(h->d_inv_sf, cur->hp.inv_sf.data());
    table(h->d_sigma2, cur->hp.sigma2.data());
    table(h->d_inv_sigma2, cur->hp.inv_sigma2.data());
    if (e == hipSuccess) {
      float thr[SD_MAX_LEVELS];   // MapPoint::PredictScale breakpoints (track_handle.h)
      predict_scale_thresholds(cur->scaleFactor, thr);
      e = hipMemcpy(h->d_scale_thr, thr, sizeof(thr), hipMemcpyHostToDevice);
    }
    for (int r = 0; r < sd_track::kRing && e == hipSuccess; r++)
      for (int i = 0; i < 6 && e == hipSuccess; i++) e = hipEventCreate(&h->ev[r][i]);
    if (e == hipSuccess) e = h->pose_ring.create(B * 16 * sizeof(double));
    if (e == hipSuccess) e = h->small_ring.create(B * 8 * sizeof(int32_t));
    if (e == hipSuccess) e = h->sim3_ring.create((K + 1) * sizeof(int32_t));
    if (e == hipSuccess) {
      // Priority of the tracking stream.  Round 1 (extraction kernels at 6-7 waves per SIMD): lowest was best (122.3 k vs
      // 119.2 k frames/s at highest) -- the few, long-running, latency-bound tracking workgroups filled what the extraction
      // left free.  Round 2 (FAST / select at 8 waves per SIMD leave nothing free): the chain of tracking kernels starves at
      // the lowest priority and becomes the longest path of the step when it is long (TrackWithMotionModel + TrackLocalMap:
      // low 107.3 k, normal 108.3 k, HIGH 113.3 k frames/s); with the PnP step all three are within 0.5 % (145.7 / 145.4 /
      // 146.1 k).  Default: highest.
      int lo = 0, hi = 0;
      e = hipDeviceGetStreamPriorityRange(&lo, &hi);
      const int pe = opt(OPT_TRACK_PRIORITY);   // option "track.stream_priority": 0 low | 1 normal | 2 high (default)
      const int prio = pe == 0 ? lo : (pe == 1 ? (lo + hi) / 2 : hi);
      if (e == hipSuccess) e = hipStreamCreateWithPriority(&h->pnp_stream, hipStreamNonBlocking, prio);
    }
    if (e != hipSuccess) {
      set_error(std::string("sd_track_create: ") + hipGetErrorString(e));
      rc = SD_ERR_HIP;
    }
    // both motion models as their constructors leave them (ConstantVelocity::Init, IMU::Init on a zeroed P).  These kernels
    // must stay behind the blocking hipMemcpy calls of the tables above (d_scale_thr's is the last), which drain the null stream
    // of dalloc's fills (the tracking stream does not wait for it); every reader of the filters runs on the tracking stream or
    // waits for it (TRACK_RANGE)
    if (rc == SD_OK) rc = launch_motion_init(tb, 0, max_batch, h->pnp_stream);
    if (rc == SD_OK) rc = launch_imu_init(tb, 0, max_batch, /*full*/ 1, h->pnp_stream);
    if (rc == SD_OK) rc = orb_enable_double_buffer(cur);
  }
  if (rc != SD_OK) {
    sd_track_destroy(h);
    return rc;
  }
  *out = h;
  return SD_OK;
}

void sd_track_destroy(sd_track* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  if (h->pnp_stream) (void)hipStreamSynchronize(h->pnp_stream);
  if (h->cur && h->cur->stream) (void)hipStreamSynchronize(h->cur->stream);
  if (h->pnp_stream) (void)hipStreamDestroy(h->pnp_stream);
  for (void* p : h->allocs) (void)hipFree(p);
  refresh_destroy(h);
  ba_destroy(h);
  cull_destroy(h);
  if (h->ev_fence) (void)hipEventDestroy(h->ev_fence);
  h->pose_ring.destroy();
  h->small_ring.destroy();
  h->sim3_ring.destroy();
  for (int r = 0; r < sd_track::kRing; r++)
    for (int i = 0; i < 6; i++)
      if (h->ev[r][i]) (void)hipEventDestroy(h->ev[r][i]);
  delete h;
}

int sd_track_set_camera(sd_track* h, float fx, float fy, float cx, float cy, float bf, float min_x, float max_x, float min_y,
                        float max_y) {
  SD_REQUIRE(h, SD_ERR_INVALID_ARG, "handle is NULL");
  SD_REQUIRE(fx > 0 && fy > 0 && max_x > min_x && max_y > min_y, SD_ERR_INVALID_ARG, "bad camera parameters");
  h->cam = make_cam(fx, fy, cx, cy, bf, min_x, max_x, min_y, max_y);
  h->have_cam = true;
  END_RESULTS(h, "sd_track_set_camera");
  return SD_OK;
}

int sd_track_set_last(sd_track* h, int frame0, int n_frames, const int32_t* n_last, const uint8_t* valid, const double* Xw,
                      const uint8_t* desc, const int32_t* octave, const float* angle, const int32_t* obs) {
  TRACK_RANGE(h, frame0, n_frames);
  SD_REQUIRE(n_last && valid && Xw && desc && octave && angle && obs, SD_ERR_INVALID_ARG, "NULL argument");
  END_RESULTS(h, "sd_track_set_last");
  const size_t M = h->max_points, o = (size_t)frame0, n = (size_t)n_frames;
  for (int f = 0; f < n_frames; f++) SD_REQUIRE(n_last[f] >= 0 && n_last[f] <= h->max_points, SD_ERR_CAPACITY, "n_last exceeds max_points");
  // the octave indexes mvScaleFactors / mvLevelSigma2 on the device (search radius, level window)
  for (int f = 0; f < n_frames; f++)
    for (int i = 0; i < n_last[f]; i++)
      SD_REQUIRE(!valid[(size_t)f * M + i] || (octave[(size_t)f * M + i] >= 0 && octave[(size_t)f * M + i] < h->cur->nlevels),
                 SD_ERR_INVALID_ARG, "octave of a valid last-frame point outside [0, nlevels)");
  hipStream_t s = h->cur->stream;
  const TrackBuffers& tb = h->tb;
  SD_TRY(upload(tb.n_last, n_last, o, n, 1, s));
  SD_TRY(upload(tb.valid, valid, o, n, M, s));
  SD_TRY(upload(tb.Xw, Xw, o, n, M * 3, s));
  SD_TRY(upload(tb.mp_desc, desc, o, n, M * 32, s));
  SD_TRY(upload(tb.octave, octave, o, n, M, s));
  SD_TRY(upload(tb.angle, angle, o, n, M, s));
  SD_TRY(upload(tb.obs, obs, o, n, M, s));
  SD_HIP_CHECK(hipMemsetAsync(tb.last_id + o * M, 0xFF, n * M * sizeof(int32_t), s));   // new points: no ids until sd_track_set_map_ids
  return wait_for(s);
}

int sd_track_set_poses(sd_track* h, int frame0, int n_frames, const double* Tref_cm, const double* Tcur_cm) {
  TRACK_RANGE(h, frame0, n_frames);
  SD_REQUIRE(Tref_cm && Tcur_cm, SD_ERR_INVALID_ARG, "NULL argument");
  END_RESULTS(h, "sd_track_set_poses");
  // a global bundle adjustment's result is kept aside for poses that are being replaced (mTcwGBA is applied relative to them);
  // a local one's is a record of its run and stays (track_results.h, kEndsBa)
  if (h->ba.ran_global) h->ba.ran_points = -1;
  hipStream_t s = h->cur->stream;
  SD_TRY(upload(h->tb.Tref, Tref_cm, frame0, n_frames, 16, s));
  SD_TRY(upload(h->tb.Tprior, Tcur_cm, frame0, n_frames, 16, s));
  SD_TRY(upload(h->tb.Tcur, Tcur_cm, frame0, n_frames, 16, s));
  return wait_for(s);
}

int sd_track_set_rand(sd_track* h, int frame0, int n_frames, const int32_t* rand_values, int per_frame) {
  TRACK_RANGE(h, frame0, n_frames);
  SD_REQUIRE(rand_values && per_frame >= 1 && per_frame <= h->rand_per_frame, SD_ERR_INVALID_ARG, "bad rand stream");
  END_RESULTS(h, "sd_track_set_rand");
  SD_TRY(upload_rows(h->tb.rand_stream, h->rand_per_frame, rand_values, per_frame, frame0, n_frames, h->cur->stream));
  SD_HIP_CHECK(hipStreamSynchronize(h->cur->stream));
  for (int f = 0; f < n_frames; f++) h->rand_len[(size_t)frame0 + f] = per_frame;
  return SD_OK;
}

// One current frame against n keyframes (Tracking::Relocalization, LoopClosing::DetectLoop): slot f of the tracker
// (its map points, Tref/Tprior, the ref extractor's frame f) pairs with frame `cur_frame` of the cur extractor and with
// that frame's mvuRight row.  -1 restores slot f <-> current frame f.
int sd_track_set_current_broadcast(sd_track* h, int cur_frame) {
  SD_REQUIRE(h, SD_ERR_INVALID_ARG, "handle is NULL");
  SD_REQUIRE(cur_frame >= -1 && cur_frame < h->cur->max_batch && cur_frame < h->max_batch, SD_ERR_INVALID_ARG,
             "cur_frame outside the cur extractor / tracker batch");
  h->tb.cur_bcast = cur_frame;   // TrackBuffers travels by value with every launch: queued kernels keep the old setting
  return SD_OK;
}

int sd_track_align(sd_track* h, int n_frames, int mode) {
  SD_TRY(check_ready(h, n_frames));
  SD_REQUIRE(mode >= 0 && mode <= 3, SD_ERR_INVALID_ARG, "bad mode");
  SD_TRY(require_ref_frames(h, n_frames, true));
  return run_stage(h, true, true, STAGE_ALIGN, [&](hipStream_t s) {
    return launch_align(h->cur, h->ref, h->tb, h->cam, h->d_inv_sf, h->d_sf, n_frames, mode, s);
  });
}

int sd_track_match(sd_track* h, int n_frames, float th, int mono, int check_ori) {
  SD_TRY(check_ready(h, n_frames));
  END_RESULTS(h, "sd_track_match");
  return run_stage(h, false, false, STAGE_MATCH, [&](hipStream_t s) {
    return launch_match(h->cur, h->tb, h->cam, h->d_sf, n_frames, th, mono, check_ori, s);
  });
}

// TrackLocalMap's search.  Local map points of every frame, flattened in mvpLocalMapPoints order.
int sd_track_set_local(sd_track* h, int frame0, int n_frames, const int32_t* n_local, const uint8_t* cand, const double* Xw,
                       const double* normal, const float* min_dist, const float* max_dist, const float* mf_max_dist, const uint8_t* desc,
                       const int32_t* obs, const uint8_t* kp_claimed) {
  TRACK_RANGE(h, frame0, n_frames);
  SD_REQUIRE(n_local && cand && Xw && normal && min_dist && max_dist && mf_max_dist && desc && obs, SD_ERR_INVALID_ARG, "NULL argument");
  const size_t M = h->max_points, K = h->kp_cap, o = (size_t)frame0, n = (size_t)n_frames;
  for (int f = 0; f < n_frames; f++) SD_REQUIRE(n_local[f] >= 0 && n_local[f] <= h->max_points, SD_ERR_CAPACITY, "n_local exceeds max_points");
  END_RESULTS(h, "sd_track_set_local");
  hipStream_t s = h->cur->stream;
  const TrackBuffers& tb = h->tb;
  SD_TRY(upload(tb.lm_n, n_local, o, n, 1, s));
  SD_TRY(upload(tb.lm_cand, cand, o, n, M, s));
  SD_TRY(upload(tb.lm_Xw, Xw, o, n, M * 3, s));
  SD_TRY(upload(tb.lm_normal, normal, o, n, M * 3, s));
  SD_TRY(upload(tb.lm_min, min_dist, o, n, M, s));
  SD_TRY(upload(tb.lm_max, max_dist, o, n, M, s));
  SD_TRY(upload(tb.lm_mfmax, mf_max_dist, o, n, M, s));
  SD_TRY(upload(tb.lm_desc, desc, o, n, M * 32, s));
  SD_TRY(upload(tb.lm_obs, obs, o, n, M, s));
  if (kp_claimed) SD_TRY(upload(tb.lm_kclaim, kp_claimed, o, n, K, s));
  else SD_HIP_CHECK(hipMemsetAsync(tb.lm_kclaim + o * K, 0, n * K, s));
  return wait_for(s);
}

// ORBmatcher::SearchByProjection(Frame& F, const vector<MapPoint*>& vpMapPoints, th) on the caller's OWN isInFrustum results
// (reference src/ORBmatcher.cc:43-119 reads pMP->mbTrackInView, mTrackProjX / Y / XR, mnTrackScaleLevel, mTrackViewCos, which
// Frame::isInFrustum left in the MapPoint): sd_track_set_local_view uploads them, sd_track_match_local_view searches.
// in_view[i] = mbTrackInView && !isBad().
int sd_track_set_local_view(sd_track* h, int frame0, int n_frames, const int32_t* n_local, const uint8_t* in_view, const float* proj3,
                            const int32_t* level, const float* view_cos, const uint8_t* desc, const int32_t* obs, const uint8_t* kp_claimed) {
  TRACK_RANGE(h, frame0, n_frames);
  SD_REQUIRE(n_local && in_view && proj3 && level && view_cos && desc && obs, SD_ERR_INVALID_ARG, "NULL argument");
  const size_t M = h->max_points, K = h->kp_cap, o = (size_t)frame0, n = (size_t)n_frames;
  for (int f = 0; f < n_frames; f++) {
    SD_REQUIRE(n_local[f] >= 0 && n_local[f] <= h->max_points, SD_ERR_CAPACITY, "n_local exceeds max_points");
    for (int i = 0; i < n_local[f]; i++)
      SD_REQUIRE(!in_view[(size_t)f * M + i] || (level[(size_t)f * M + i] >= 0 && level[(size_t)f * M + i] < h->cur->nlevels), SD_ERR_INVALID_ARG,
                 "mnTrackScaleLevel of an in-view point outside [0, nlevels)");
  }
  END_RESULTS(h, "sd_track_set_local_view");
  hipStream_t s = h->cur->stream;
  const TrackBuffers& tb = h->tb;
  SD_TRY(upload(tb.lm_n, n_local, o, n, 1, s));
  SD_TRY(upload(tb.lm_inview, in_view, o, n, M, s));
  SD_TRY(upload(tb.lm_proj, proj3, o, n, M * 3, s));
  SD_TRY(upload(tb.lm_level, level, o, n, M, s));
  SD_TRY(upload(tb.lm_cos, view_cos, o, n, M, s));
  SD_TRY(upload(tb.lm_desc, desc, o, n, M * 32, s));
  SD_TRY(upload(tb.lm_obs, obs, o, n, M, s));
  if (kp_claimed) SD_TRY(upload(tb.lm_kclaim, kp_claimed, o, n, K, s));
  else SD_HIP_CHECK(hipMemsetAsync(tb.lm_kclaim + o * K, 0, n * K, s));
  return wait_for(s);
}

int sd_track_match_local_view(sd_track* h, int n_frames, float th, float nnratio) {
  SD_TRY(check_ready(h, n_frames));
  return run_stage(h, false, false, STAGE_NONE, [&](hipStream_t s) {
    return launch_match_local(h->cur, h->tb, h->cam, h->d_sf, h->d_scale_thr, h->cur->nlevels, n_frames, th, nnratio, 0.f, s, 0, 1);
  });
}

// Frame::isInFrustum for every candidate + ORBmatcher::SearchByProjection(F, vpMapPoints, th) with mfNNratio = nnratio,
// at the frames' current poses (sd_track_set_poses / the ImageAlign result)
int sd_track_match_local(sd_track* h, int n_frames, float th, float nnratio, float viewing_cos_limit) {
  SD_TRY(check_ready(h, n_frames));
  return run_stage(h, false, false, STAGE_NONE, [&](hipStream_t s) {
    return launch_match_local(h->cur, h->tb, h->cam, h->d_sf, h->d_scale_thr, h->cur->nlevels, n_frames, th, nnratio, viewing_cos_limit, s);
  });
}

int sd_track_get_local(sd_track* h, int frame0, int n_frames, int32_t* local_match, int cap, int32_t* n_matches, uint8_t* in_view,
                       float* proj3, int32_t* level, float* view_cos) {
  TRACK_RANGE(h, frame0, n_frames);
  SD_REQUIRE(!local_match || cap >= h->kp_cap, SD_ERR_CAPACITY, "cap smaller than the keypoint capacity");
  hipStream_t s = h->cur->stream;
  const size_t M = h->max_points, o = frame0, n = n_frames;
  const TrackBuffers& tb = h->tb;
  SD_TRY(download_rows(local_match, cap, tb.lm_match, o, n, h->kp_cap, s));
  SD_TRY(download(n_matches, tb.lm_nmatch, o, n, 1, s));
  SD_TRY(download(in_view, tb.lm_inview, o, n, M, s));
  SD_TRY(download(proj3, tb.lm_proj, o, n, M * 3, s));
  SD_TRY(download(level, tb.lm_level, o, n, M, s));
  SD_TRY(download(view_cos, tb.lm_cos, o, n, M, s));
  return wait_for(s);
}

// Optimizer::PoseOptimization(&CurrentFrame) at the frames' current poses (tb.Tcur: sd_track_set_poses / ImageAlign result).
// source 0: mvpMapPoints = the frame-to-frame matches (sd_track_match); 1: the local-map matches (sd_track_match_local).
int sd_track_pose_opt(sd_track* h, int n_frames, int source) {
  SD_TRY(check_ready(h, n_frames));
  SD_REQUIRE(source >= 0 && source <= 2, SD_ERR_INVALID_ARG, "source must be 0 (frame matches), 1 (local-map matches) or 2 (both, as after SearchLocalPoints)");
  return run_stage(h, false, false, STAGE_SOLVE, [&](hipStream_t s) {   // timed in the pose-solve slot, like sd_track_pnp
    return launch_pose_opt(h->cur, h->tb, h->cam, h->d_inv_sigma2, source, n_frames, s);
  });
}

// Tracking::TrackWithMotionModel (reference src/Tracking.cc:654-718) / TrackReferenceKeyFrame (:583-644) for the batch, as
// one queue of launches with the reference's per-frame decisions taken on the device (no host round trip):
//   ImageAlign::ComputePose(cur, last)  [align_mode 0; 1 = (cur, reference keyframe); -1 = align_image_ off]; a failed
//     alignment leaves the predicted pose
//   SearchByProjection(cur, last, th, mono) with orientation check
//   nmatches < min_matches (20): pose := predicted, SearchByProjection again with 2 * th       (k_match, retry_below)
//   nmatches < min_matches: tracking failed (status 0), PoseOptimization is not run             (k_pose_opt gate)
//   PoseOptimization; outliers lose their map point and flag; nmatchesMap = survivors with Observations() > 0;
//   status 2 iff nmatchesMap >= min_inliers (10), else 1
// The frame's pose (sd_track_get_pose_opt / the tracker's current pose), mvpMapPoints (sd_track_get_matches) and the
// counts (sd_track_get_tracked) are what the reference leaves in mCurrentFrame.  TrackReferenceKeyFrame's second search
// goes to mLastFrame, not to the keyframe (src/Tracking.cc:610): with align_mode 1 it equals the reference when the slot's
// points serve both, otherwise run the stages separately.
int sd_track_with_motion_model(sd_track* h, int n_frames, int align_mode, float th, int mono, int min_matches, int min_inliers) {
  SD_TRY(check_ready(h, n_frames));
  SD_REQUIRE(align_mode >= -1 && align_mode <= 1, SD_ERR_INVALID_ARG, "align_mode must be -1 (off), 0 (last frame) or 1 (reference keyframe)");
  SD_REQUIRE(min_matches >= 3 && min_inliers >= 0, SD_ERR_INVALID_ARG, "bad gates (reference: 20 matches, 10 inliers)");
  hipStream_t s = h->pnp_stream;
  const TrackBuffers& tb = h->tb;
  END_RESULTS(h, "sd_track_with_motion_model");
  const bool use_ref = align_mode >= 0;
  if (use_ref) SD_TRY(require_ref_frames(h, n_frames, true));
  SD_TRY(wait_inputs(h, use_ref, use_ref));
  SD_HIP_CHECK(hipMemsetAsync(tb.tw_info, 0, (size_t)n_frames * 4 * sizeof(int32_t), s));
  SD_TRY(stage_begin(h, STAGE_ALIGN));
  int rc = SD_OK;
  if (use_ref) rc = launch_align(h->cur, h->ref, tb, h->cam, h->d_inv_sf, h->d_sf, n_frames, align_mode, s);
  else SD_HIP_CHECK(hipMemcpyAsync(tb.Tcur, tb.Tprior, (size_t)n_frames * 16 * sizeof(double), hipMemcpyDeviceToDevice, s));
  SD_TRY(stage_end(h, STAGE_ALIGN));
  SD_TRY(rc);
  if (use_ref) {
    SD_TRY(mark_reads(h, true));
    SD_TRY(wait_inputs(h, false));   // the matcher needs the keypoints, not only the pyramid
  }
  SD_TRY(stage_begin(h, STAGE_MATCH));
  rc = launch_match(h->cur, tb, h->cam, h->d_sf, n_frames, th, mono, 1, s, 0, min_matches);   // (lists the frames that need the retry)
  if (rc == SD_OK) rc = launch_match(h->cur, tb, h->cam, h->d_sf, n_frames, 2.f * th, mono, 1, s, min_matches);
  SD_TRY(stage_end(h, STAGE_MATCH));
  SD_TRY(rc);
  SD_TRY(stage_begin(h, STAGE_SOLVE));
  rc = launch_pose_opt(h->cur, tb, h->cam, h->d_inv_sigma2, 0, n_frames, s, min_matches, min_inliers);
  SD_TRY(stage_end(h, STAGE_SOLVE));
  SD_TRY(rc);
  SD_TRY(mark_reads(h, false));
  h->ran[0].set(h, n_frames);
  return SD_OK;
}

// Tracking::TrackLocalMap (reference src/Tracking.cc:720-751) for the batch, after sd_track_with_motion_model (or any
// sd_track_match) left the frame-to-frame matches and the pose: SearchLocalPoints (:898-939: isInFrustum + the local-map
// SearchByProjection; a keypoint is closed to the search where its frame match has observations) -> PoseOptimization over
// ALL of mvpMapPoints (frame matches and local matches) -> mnMatchesInliers -> tracked iff >= min_inliers (30).
// The local map (sd_track_set_local) is the caller's UpdateLocalMap(); its `cand` flags carry the "already matched in this
// frame / isBad" skips of :916-921, kp_claimed is ignored here.  th: 1, 3 for RGB-D, 5 after a relocalisation (:929-934).
int sd_track_local_map(sd_track* h, int n_frames, float th, float nnratio, float viewing_cos_limit, int min_inliers) {
  SD_TRY(check_ready(h, n_frames));
  SD_REQUIRE(min_inliers >= 0, SD_ERR_INVALID_ARG, "bad min_inliers (reference: 30)");
  hipStream_t s = h->pnp_stream;
  SD_TRY(wait_inputs(h, false));
  SD_TRY(stage_begin(h, STAGE_MATCH));
  // seen-point exclusion: ids given, and tw_seen holds this extraction's TrackWithMotionModel result for these slots
  const int exclude = h->ids_on && h->ran[0].covers(h, n_frames) ? 1 : 0;
  int rc = launch_match_local(h->cur, h->tb, h->cam, h->d_sf, h->d_scale_thr, h->cur->nlevels, n_frames, th, nnratio, viewing_cos_limit, s, 1, 0,
                              exclude);
  SD_TRY(stage_end(h, STAGE_MATCH));
  SD_TRY(rc);
  SD_TRY(stage_begin(h, STAGE_SOLVE));
  rc = launch_pose_opt(h->cur, h->tb, h->cam, h->d_inv_sigma2, 2, n_frames, s, 0, min_inliers);
  SD_TRY(stage_end(h, STAGE_SOLVE));
  SD_TRY(rc);
  SD_TRY(mark_reads(h, false));
  h->ran[1].set(h, n_frames);
  return SD_OK;
}

// map_match (may be NULL): mvpMapPoints after SearchLocalPoints, -1 | v < max_points: last-frame point v | v >= max_points:
// local map point v - max_points.  info4: status (1 failed, 2 tracked), points in mvpMapPoints, mnMatchesInliers, local matches
int sd_track_get_local_map(sd_track* h, int frame0, int n_frames, int32_t* map_match, int cap, int32_t* info4) {
  TRACK_RANGE(h, frame0, n_frames);
  SD_REQUIRE(!map_match || cap >= h->kp_cap, SD_ERR_CAPACITY, "cap smaller than the keypoint capacity");
  hipStream_t s = h->cur->stream;
  SD_TRY(download_rows(map_match, cap, h->tb.un_match, frame0, n_frames, h->kp_cap, s));
  SD_TRY(download(info4, h->tb.tl_info, frame0, n_frames, 4, s));
  return wait_for(s);
}

// info4 per frame: status (0 few matches, 1 few inliers, 2 tracked), nmatches after the discard, nmatchesMap, retried
int sd_track_get_tracked(sd_track* h, int frame0, int n_frames, int32_t* info4) {
  TRACK_RANGE(h, frame0, n_frames);
  SD_REQUIRE(info4, SD_ERR_INVALID_ARG, "NULL argument");
  SD_TRY(download(info4, h->tb.tw_info, frame0, n_frames, 4, h->cur->stream));
  return wait_for(h->cur->stream);
}

// Tracking::Relocalization (reference src/Tracking.cc:1064-1097) over all keyframes at once.  The reference walks the
// keyframes newest first and, for each: sets the frame's pose to the keyframe's, ImageAlign::ComputePose(frame, kf, fast)
// [continue on failure], clears mvpMapPoints, SearchByProjection(frame, kf, th, mono) [continue if < 20],
// PoseOptimization [continue if nGood < 10], else returns true.  Nothing an attempt leaves behind is read by the next one
// (pose and mvpMapPoints are reset, mvbOutlier is rewritten per edge), so the attempts are independent: slot i of the
// tracker holds the i-th keyframe TRIED (caller order = kfs.rbegin() ...), all slots run the three stages against the
// broadcast current frame, and the host returns the first slot that passes the three gates -- the keyframe at which the
// sequential loop would have stopped.  Its pose / matches / outlier flags are slot `winner`'s (sd_track_get_pose_opt,
// sd_track_get_matches).  Caller: sd_track_set_last (keyframe points), sd_track_set_poses(Tref = Tprior = kf pose).
int sd_track_relocalize(sd_track* h, int n_keyframes, int cur_frame, float th, int mono, int min_matches, int min_good,
                        int32_t* winner, int32_t* stage3 /* [n][3] align ok, nmatches, nGood; may be NULL */) {
  SD_REQUIRE(h && winner, SD_ERR_INVALID_ARG, "NULL argument");
  *winner = -1;
  SD_REQUIRE(cur_frame >= 0, SD_ERR_INVALID_ARG, "cur_frame must name a frame of the cur extractor");
  SD_TRY(with_broadcast(h, cur_frame, [&] {
    SD_TRY(sd_track_align(h, n_keyframes, 2));
    SD_TRY(sd_track_match(h, n_keyframes, th, mono, 1));   // ORBmatcher matcher(0.75, true)
    return sd_track_pose_opt(h, n_keyframes, 0);
  }));
  std::vector<int32_t> ok(n_keyframes), nm(n_keyframes), info((size_t)n_keyframes * 8);
  hipStream_t s = h->pnp_stream;
  SD_TRY(download(ok.data(), h->tb.al_ok, 0, n_keyframes, 1, s));
  SD_TRY(download(nm.data(), h->tb.n_matches, 0, n_keyframes, 1, s));
  SD_TRY(download(info.data(), h->tb.po_info, 0, n_keyframes, 8, s));
  SD_HIP_CHECK(hipStreamSynchronize(s));
  for (int i = 0; i < n_keyframes; i++) {
    const int good = info[(size_t)i * 8 + 5];
    if (stage3) { stage3[i * 3] = ok[i]; stage3[i * 3 + 1] = nm[i]; stage3[i * 3 + 2] = good; }
    if (*winner < 0 && ok[i] && nm[i] >= min_matches && good >= min_good) *winner = i;
  }
  return SD_OK;
}

// The candidate search of LoopClosing::DetectLoop (reference src/LoopClosing.cc:115-149): ImageAlign::ComputePose(
// mpCurrentKF, kf) -- level 4 only, identity start, rejected above 0.03 -- against every keyframe of the map.  Slot i holds
// kfs[i] (its GetMapPoints() in the caller's order, its pose as Tref, its pyramid in the ref extractor); the current
// keyframe is frame `cur_frame` of the cur extractor.  excluded[i] != 0 marks the keyframes the loop `continue`s over before
// aligning (the current keyframe itself, connected keyframes).  The reference's loop is replayed on the host over the batched
// results, including its `i++` after a failed alignment (the keyframe after a failure is never looked at), then the
// survivors with error < 1.5 * best are returned -- in slot order (the reference iterates a std::map<KeyFrame*, double>,
// i.e. pointer order; only the SET is defined).
int sd_track_detect_loop(sd_track* h, int n_keyframes, int cur_frame, const uint8_t* excluded, int32_t* candidates, int cap,
                         int32_t* n_candidates, double* best_error, double* errors /* [n], 1e10 where rejected; may be NULL */) {
  SD_REQUIRE(h && candidates && n_candidates && cap >= 0, SD_ERR_INVALID_ARG, "NULL argument");
  *n_candidates = 0;
  SD_REQUIRE(cur_frame >= 0, SD_ERR_INVALID_ARG, "cur_frame must name a frame of the cur extractor");
  SD_TRY(with_broadcast(h, cur_frame, [&] { return sd_track_align(h, n_keyframes, 3); }));
  std::vector<int32_t> ok(n_keyframes);
  std::vector<double> err(n_keyframes);
  hipStream_t s = h->pnp_stream;
  SD_TRY(download(ok.data(), h->tb.al_ok, 0, n_keyframes, 1, s));
  SD_TRY(download(err.data(), h->tb.al_err, 0, n_keyframes, 1, s));
  SD_HIP_CHECK(hipStreamSynchronize(s));
  if (errors) std::memcpy(errors, err.data(), (size_t)n_keyframes * sizeof(double));
  double best = 1e10;
  std::vector<int32_t> kept;
  for (int i = 0; i < n_keyframes; i++) {
    if (excluded && excluded[i]) continue;
    if (!ok[i]) { i++; continue; }   // "Skip some keyframes"
    kept.push_back(i);
    if (err[i] < best) best = err[i];
  }
  int n = 0;
  for (int32_t i : kept)
    if (err[i] < best * 1.5) {
      SD_REQUIRE(n < cap, SD_ERR_CAPACITY, "candidates array too small");
      candidates[n++] = i;
    }
  *n_candidates = n;
  if (best_error) *best_error = best;
  return SD_OK;
}

int sd_track_get_pose_opt(sd_track* h, int frame0, int n_frames, double* Tcw_cm, uint8_t* outlier, int cap, int32_t* info8) {
  TRACK_RANGE(h, frame0, n_frames);
  SD_REQUIRE(!outlier || cap >= h->kp_cap, SD_ERR_CAPACITY, "cap smaller than the keypoint capacity");
  hipStream_t s = h->cur->stream;
  SD_TRY(download(Tcw_cm, h->tb.po_T, frame0, n_frames, 16, s));
  SD_TRY(download_rows(outlier, cap, h->tb.po_outlier, frame0, n_frames, h->kp_cap, s));
  SD_TRY(download(info8, h->tb.po_info, frame0, n_frames, 8, s));
  return wait_for(s);
}

// CurrentFrame.mvuRight supplied by the caller (stereo) -- [n_frames][kp_cap] floats, -1 = none
int sd_track_set_uright(sd_track* h, int frame0, int n_frames, const float* uright, int cap) {
  TRACK_RANGE(h, frame0, n_frames);
  SD_REQUIRE(uright && cap >= 1 && cap <= h->kp_cap, SD_ERR_INVALID_ARG, "bad uright array");
  END_RESULTS(h, "sd_track_set_uright");
  SD_TRY(upload_rows(h->tb.uright, h->kp_cap, uright, cap, frame0, n_frames, h->cur->stream));
  return wait_for(h->cur->stream);
}

// Frame::ComputeStereoFromRGBD on the current frames of the batch: depth images (CV_32F, host memory)
int sd_track_stereo_from_depth(sd_track* h, int n_frames, const float* depth, int w, int hgt, int stride_elems, size_t frame_stride_elems) {
  SD_TRY(check_ready(h, n_frames, true));
  SD_REQUIRE(depth && w >= 1 && hgt >= 1 && stride_elems >= w, SD_ERR_INVALID_ARG, "bad depth image");
  END_RESULTS(h, "sd_track_stereo_from_depth");
  SD_HIP_CHECK(hipStreamSynchronize(h->pnp_stream));   // a queued match may still read the stereo arrays
  float* d_depth = nullptr;
  const size_t total = (size_t)n_frames * w * hgt;
  SD_HIP_CHECK(hipMalloc(&d_depth, total * sizeof(float)));
  hipStream_t s = h->cur->stream;
  hipError_t e = hipSuccess;
  int rc = SD_OK;
  for (int f = 0; f < n_frames && e == hipSuccess; f++)
    e = hipMemcpy2DAsync(d_depth + (size_t)f * w * hgt, w * sizeof(float), depth + (size_t)f * frame_stride_elems, stride_elems * sizeof(float),
                         w * sizeof(float), hgt, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) rc = launch_stereo_from_depth(h->cur, h->tb, h->cam, d_depth, w, hgt, w, (size_t)w * hgt, n_frames, s);
  hipError_t e2 = hipStreamSynchronize(s);
  (void)hipFree(d_depth);
  if (e != hipSuccess || e2 != hipSuccess) return hip_error("sd_track_stereo_from_depth", e != hipSuccess ? e : e2);
  return rc;
}

// The same on depth maps already in device memory, with Tracking::GrabImageRGBD's conversion (src/Tracking.cc:113-117,
// 147-148) applied to the pixels read.  Queued on the tracking stream behind the current extraction: no host wait, no
// allocation, no copy of the maps.
int sd_track_stereo_from_depth_device(sd_track* h, int n_frames, const void* d_depth, int dtype, int w, int hgt, int stride_elems,
                                      size_t frame_stride_elems, float depth_map_factor) {
  SD_TRY(check_ready(h, n_frames, true));
  SD_REQUIRE(d_depth && (dtype == SD_DEPTH_F32 || dtype == SD_DEPTH_U16) && w >= 1 && hgt >= 1 && stride_elems >= w, SD_ERR_INVALID_ARG,
             "bad depth image (NULL, unknown dtype, empty or stride < w)");
  SD_REQUIRE((uintptr_t)d_depth % (dtype == SD_DEPTH_U16 ? 2 : 4) == 0, SD_ERR_INVALID_ARG, "depth pointer not aligned to its element size");
  // mDepthMapFactor and the convertTo condition, in the reference's float arithmetic
  END_RESULTS(h, "sd_track_stereo_from_depth_device");
  const float scale = std::fabs(depth_map_factor) < 1e-5 ? 1.0f : 1.0f / depth_map_factor;
  const bool convert = std::fabs(scale - 1.0f) > 1e-5 || dtype != SD_DEPTH_F32;
  return run_stage(h, false, false, STAGE_NONE, [&](hipStream_t s) {
    return launch_stereo_from_depth_typed(h->cur, h->tb, h->cam, d_depth, dtype == SD_DEPTH_U16, convert, scale, w, hgt, stride_elems,
                                          frame_stride_elems, n_frames, s);
  });
}

int sd_track_get_stereo(sd_track* h, int frame0, int n_frames, float* uright, float* depth, int cap) {
  TRACK_RANGE(h, frame0, n_frames);
  SD_REQUIRE(cap >= h->kp_cap, SD_ERR_CAPACITY, "cap smaller than the keypoint capacity");
  hipStream_t s = h->cur->stream;
  SD_TRY(download_rows(uright, cap, h->tb.uright, frame0, n_frames, h->kp_cap, s));
  SD_TRY(download_rows(depth, cap, h->tb.depth, frame0, n_frames, h->kp_cap, s));
  return wait_for(s);
}

// ORBmatcher::SearchByPoints(currentKF, pKF, matches) (reference src/ORBmatcher.cc:1209-1301) for the batch: slot f matches
// the keypoints of current frame f (or the broadcast frame) that hold a map point against those of frame f of the ref
// extractor.  has_mp_* = "GetMapPointMatches()[i] != NULL && !isBad()", [n_frames][cap], rows shorter than the keypoint
// capacity are padded with 0.
int sd_track_set_point_flags(sd_track* h, int frame0, int n_frames, const uint8_t* has_mp_cur, const uint8_t* has_mp_ref, int cap) {
  TRACK_RANGE(h, frame0, n_frames);
  SD_REQUIRE(has_mp_cur && has_mp_ref && cap >= 1 && cap <= h->kp_cap, SD_ERR_INVALID_ARG, "bad flag arrays (cap must be 1..keypoint capacity)");
  END_RESULTS(h, "sd_track_set_point_flags");
  hipStream_t s = h->cur->stream;
  const size_t K = h->kp_cap, o = (size_t)frame0 * K;
  SD_HIP_CHECK(hipMemsetAsync(h->tb.sp_valid1 + o, 0, (size_t)n_frames * K, s));
  SD_HIP_CHECK(hipMemsetAsync(h->tb.sp_valid2 + o, 0, (size_t)n_frames * K, s));
  SD_TRY(upload_rows(h->tb.sp_valid1, K, has_mp_cur, cap, frame0, n_frames, s));
  SD_TRY(upload_rows(h->tb.sp_valid2, K, has_mp_ref, cap, frame0, n_frames, s));
  return wait_for(s);
}

int sd_track_search_by_points(sd_track* h, int n_frames, float nnratio, int check_ori) {
  SD_TRY(check_ready(h, n_frames));
  SD_TRY(require_ref_frames(h, n_frames, false, true));
  END_RESULTS(h, "sd_track_search_by_points");
  return run_stage(h, true, false, STAGE_MATCH, [&](hipStream_t s) {   // timed in the matcher's slot
    return launch_search_points(h->cur, h->ref, h->tb, n_frames, nnratio, check_ori, s);
  });
}

int sd_track_get_point_matches(sd_track* h, int frame0, int n_frames, int32_t* matches12, int cap, int32_t* n_matches) {
  TRACK_RANGE(h, frame0, n_frames);
  SD_REQUIRE(!matches12 || cap >= h->kp_cap, SD_ERR_CAPACITY, "cap smaller than the keypoint capacity");
  hipStream_t s = h->cur->stream;
  SD_TRY(download_rows(matches12, cap, h->tb.sp_match, frame0, n_frames, h->kp_cap, s));
  SD_TRY(download(n_matches, h->tb.sp_n, frame0, n_frames, 1, s));
  return wait_for(s);
}

// PnPsolver(F, vpMapPointMatches) accepts ANY match vector (reference src/PnPsolver.cc:71-110), and so does
// Optimizer::PoseOptimization through pFrame->mvpMapPoints: this replaces the slot's CurrentFrame.mvpMapPoints (indices into
// the last-frame arrays, -1 = NULL) with the caller's, as if a search had produced them.
int sd_track_set_matches(sd_track* h, int frame0, int n_frames, const int32_t* cur_match, int cap) {
  TRACK_RANGE(h, frame0, n_frames);
  SD_REQUIRE(cur_match && cap >= 1 && cap <= h->kp_cap, SD_ERR_INVALID_ARG, "bad match array (cap must be 1..keypoint capacity)");
  END_RESULTS(h, "sd_track_set_matches");
  std::vector<int32_t> full((size_t)n_frames * h->kp_cap, -1), cnt((size_t)n_frames, 0);
  for (int f = 0; f < n_frames; f++)
    for (int i = 0; i < cap; i++) {
      const int32_t m = cur_match[(size_t)f * cap + i];
      SD_REQUIRE(m >= -1 && m < h->max_points, SD_ERR_INVALID_ARG, "match index outside [-1, max_points)");
      full[(size_t)f * h->kp_cap + i] = m;
      cnt[f] += m >= 0;
    }
  hipStream_t s = h->cur->stream;
  SD_TRY(upload(h->tb.cur_match, full.data(), frame0, n_frames, h->kp_cap, s));
  SD_TRY(upload(h->tb.n_matches, cnt.data(), frame0, n_frames, 1, s));
  return wait_for(s);
}

static int run_pnp(sd_track* h, int n_frames, const PnpParams& pp) {
  return run_stage(h, false, false, STAGE_SOLVE, [&](hipStream_t s) { return launch_pnp(h->cur, h->tb, h->cam, h->d_sigma2, pp, n_frames, s); });
}

// every slot must have been given the rand() values the call can consume: minSet per RANSAC iteration
static int check_rand(sd_track* h, int n_frames, long long need) {
  SD_REQUIRE(need <= h->rand_per_frame, SD_ERR_CAPACITY, "iterations exceed the handle's pnp_max_iterations (x4 rand values per slot)");
  for (int f = 0; f < n_frames; f++)
    SD_REQUIRE(h->rand_len[f] >= need, SD_ERR_INVALID_ARG,
               "sd_track_set_rand supplied fewer rand() values than the iterations can consume (minSet per iteration)");
  return SD_OK;
}

// PnPsolver ctor + SetRansacParameters + iterate(n_iterations) (reference src/PnPsolver.cc:71-244)
int sd_track_pnp(sd_track* h, int n_frames, double probability, int min_inliers, int max_iterations, int min_set, float epsilon,
                 float th2, int n_iterations) {
  SD_TRY(check_ready(h, n_frames));
  // the reference's default is 4 (src/PnPsolver.h:74); other sizes go through the general (one hypothesis at a time) path.
  // Fewer than 4 correspondences leave EPnP's 12 x 12 system rank deficient beyond its 4-D null space: the reference's own
  // hypotheses are then rounding noise of its summation order.  minSet 3 is accepted because its OUTCOME is pinned against
  // the oracle (no hypothesis reaches minInliers: empty Mat + bNoMore, tests/pnp_cases.py "minset3_degenerate"); 1 and 2
  // are pinned by nothing and refused.
  SD_REQUIRE(min_set >= 3 && min_set <= 64, SD_ERR_INVALID_ARG, "minSet must be in [3, 64]");
  SD_REQUIRE(max_iterations >= 1 && n_iterations >= 0 && min_inliers >= 0, SD_ERR_INVALID_ARG, "bad RANSAC parameters");
  const long long upper = std::max(max_iterations, n_iterations);
  SD_TRY(check_rand(h, n_frames, (long long)min_set * upper));
  PnpParams pp;
  pp.probability = probability;
  pp.min_inliers = min_inliers;
  pp.max_iterations = max_iterations;
  pp.min_set = min_set;
  pp.epsilon = epsilon;
  pp.th2 = th2;
  pp.n_iterations = n_iterations;
  pp.rand_per_frame = h->rand_per_frame;
  pp.resume = 0;
  SD_TRY(run_pnp(h, n_frames, pp));
  h->res.pnp.set(n_frames, BIND_PNP, inputs_now(h));
  h->pnp_params = pp;
  h->pnp_iter_upper = (int)upper;
  return SD_OK;
}

// A further PnPsolver::iterate(n_iterations) on the solvers the last sd_track_pnp constructed: mnIterations, the best
// hypothesis so far and the position in the rand() stream carry over (src/PnPsolver.cc:177: the loop runs while
// mnIterations < mRansacMaxIts OR nCurrentIterations < nIterations, so after the first call every call adds exactly
// n_iterations).  The match vector must not have been changed in between (the reference's solver holds its own copy).
int sd_track_pnp_iterate(sd_track* h, int n_frames, int n_iterations) {
  SD_TRY(check_ready(h, n_frames));
  SD_REQUIRE(h->res.pnp.covers(n_frames), SD_ERR_INVALID_ARG,
             "sd_track_pnp has not constructed solvers for these slots (or their matches / map points / rand stream were replaced since)");
  SD_REQUIRE(h->res.pnp.live(n_frames, inputs_now(h)), SD_ERR_INVALID_ARG,
             "the current frames were re-extracted since sd_track_pnp: the solvers' keypoints are gone");
  SD_REQUIRE(n_iterations >= 0, SD_ERR_INVALID_ARG, "bad n_iterations");
  PnpParams pp = h->pnp_params;
  const long long upper = std::max<long long>(pp.max_iterations, (long long)h->pnp_iter_upper + n_iterations);
  SD_TRY(check_rand(h, n_frames, (long long)pp.min_set * upper));
  pp.n_iterations = n_iterations;
  pp.resume = 1;
  SD_TRY(run_pnp(h, n_frames, pp));
  h->pnp_iter_upper = (int)upper;
  return SD_OK;
}

int sd_track_get_align(sd_track* h, int frame0, int n_frames, double* Tcur_cm, double* error, int32_t* ok, int32_t* iters,
                       double* chi2) {
  TRACK_RANGE(h, frame0, n_frames);
  hipStream_t s = h->cur->stream;
  const size_t o = frame0, n = n_frames;
  SD_TRY(download(Tcur_cm, h->tb.Tcur, o, n, 16, s));
  SD_TRY(download(error, h->tb.al_err, o, n, 1, s));
  SD_TRY(download(ok, h->tb.al_ok, o, n, 1, s));
  SD_TRY(download(iters, h->tb.al_iters, o, n, 16, s));
  SD_TRY(download(chi2, h->tb.al_chi2, o, n, 1, s));
  return wait_for(s);
}

int sd_track_get_matches(sd_track* h, int frame0, int n_frames, int32_t* cur_match, int cap, int32_t* n_matches) {
  TRACK_RANGE(h, frame0, n_frames);
  SD_REQUIRE(!cur_match || cap >= h->kp_cap, SD_ERR_CAPACITY, "cap smaller than the keypoint capacity");
  hipStream_t s = h->cur->stream;
  SD_TRY(download_rows(cur_match, cap, h->tb.cur_match, frame0, n_frames, h->kp_cap, s));
  SD_TRY(download(n_matches, h->tb.n_matches, frame0, n_frames, 1, s));
  return wait_for(s);
}

int sd_track_get_pnp(sd_track* h, int frame0, int n_frames, float* Tcw_rowmajor, uint8_t* inliers, int cap, int32_t* info8) {
  TRACK_RANGE(h, frame0, n_frames);
  SD_REQUIRE(!inliers || cap >= h->kp_cap, SD_ERR_CAPACITY, "cap smaller than the keypoint capacity");
  hipStream_t s = h->cur->stream;
  SD_TRY(download(Tcw_rowmajor, h->tb.pnp_T, frame0, n_frames, 16, s));
  SD_TRY(download_rows(inliers, cap, h->tb.pnp_inliers, frame0, n_frames, h->kp_cap, s));
  SD_TRY(download(info8, h->tb.pnp_info, frame0, n_frames, 8, s));
  return wait_for(s);
}

// EPnP (compute_pose, src/PnPsolver.cc:445-492) alone on explicit correspondences -- parity diagnostics
int sd_debug_pnp_prof(unsigned long long* out32, int reset) {
  SD_REQUIRE(out32, SD_ERR_INVALID_ARG, "null output");
  return read_pnp_prof(out32, reset);
}

int sd_debug_sel_prof(unsigned long long* out64, int reset) {
  SD_REQUIRE(out64, SD_ERR_INVALID_ARG, "null output");
  return read_sel_prof(out64, reset);
}

int sd_debug_align_prof(unsigned long long* out16, int reset) {
  SD_REQUIRE(out16, SD_ERR_INVALID_ARG, "null output");
  return read_align_prof(out16, reset);
}

int sd_debug_epnp(int n, const double* Xw, const double* uv, double fx, double fy, double cx, double cy, double* R9, double* t3,
                  double* reproj_err) {
  SD_REQUIRE(n >= 4 && Xw && uv && R9 && t3, SD_ERR_INVALID_ARG, "bad arguments");
  return run_epnp_debug(n, Xw, uv, fx, fy, cx, cy, R9, t3, reproj_err);
}

// diagnostics: raw copy of an internal per-frame buffer (0: pnp correspondences f32[kp_cap*6], 1: pnp keypoint indices u16[kp_cap],
// 2: what the last sd_track_fuse projected the slot with, f64[15] = Rcw row-major | tcw | Ow; the local-map row of the slot as
// sd_track_set_local or a write-through of sd_track_refresh_points left it -- 3: desc u8[M*32], 4: normal f64[M*3], 5: min_dist
// f32[M], 6: max_dist f32[M], 7: mf_max_dist f32[M]; the slot's poses as sd_track_set_poses or a write-back of sd_track_local_ba left
// them -- 8: Tref f64[16], 9: Tcur f64[16], column-major)
int sd_track_debug_read(sd_track* h, int which, int frame, void* out, size_t bytes) {
  SD_REQUIRE(h && out && frame >= 0 && frame < h->max_batch, SD_ERR_INVALID_ARG, "bad arguments");
  SD_REQUIRE(which != 2 || bytes <= 15 * sizeof(double), SD_ERR_CAPACITY, "the Fuse pose of a slot is 15 doubles");
  const size_t M = (size_t)h->max_points, row = (size_t)frame * M;
  const size_t lm_bytes[5] = {M * 32, M * 24, M * 4, M * 4, M * 4};
  SD_REQUIRE(which < 3 || (which <= 7 && bytes <= lm_bytes[which - 3]) || ((which == 8 || which == 9) && bytes <= 16 * sizeof(double)),
             SD_ERR_CAPACITY, "unknown buffer or more bytes than a local-map row / a pose holds");
  SD_HIP_CHECK(hipSetDevice(h->device));
  SD_HIP_CHECK(hipStreamSynchronize(h->pnp_stream));
  SD_HIP_CHECK(hipStreamSynchronize(h->cur->stream));
  const void* src = which == 0   ? (const void*)(h->tb.pnp_pts + (size_t)frame * h->kp_cap * 6)
                    : which == 2 ? (const void*)(h->fu.pose + (size_t)frame * 15)
                    : which == 3 ? (const void*)(h->tb.lm_desc + row * 32)
                    : which == 4 ? (const void*)(h->tb.lm_normal + row * 3)
                    : which == 5 ? (const void*)(h->tb.lm_min + row)
                    : which == 6 ? (const void*)(h->tb.lm_max + row)
                    : which == 7 ? (const void*)(h->tb.lm_mfmax + row)
                    : which == 8 ? (const void*)(h->tb.Tref + (size_t)frame * 16)
                    : which == 9 ? (const void*)(h->tb.Tcur + (size_t)frame * 16)
                                 : (const void*)(h->tb.pnp_kpidx + (size_t)frame * h->kp_cap);
  SD_HIP_CHECK(hipMemcpy(out, src, bytes, hipMemcpyDeviceToHost));
  return SD_OK;
}

// Frame::GetFeaturesInArea (src/Frame.cc:271-321) on the device grid of current frame `frame` (the grid k_match builds):
// indices in the reference's order; grid_counts (may be NULL): mGrid[x][y].size() as [64][48] ints.
int sd_track_debug_features_in_area(sd_track* h, int frame, float x, float y, float r, int min_level, int max_level, int32_t* indices,
                                    int cap, int32_t* n_out, int32_t* grid_counts) {
  SD_TRY(check_ready(h, frame + 1, true));
  SD_REQUIRE(frame >= 0 && indices && n_out && cap >= 0, SD_ERR_INVALID_ARG, "bad arguments");
  hipStream_t s = h->pnp_stream;
  SD_TRY(wait_inputs(h, false));
  int32_t* d = nullptr;
  const size_t n_ints = (size_t)h->kp_cap + 1 + 64 * 48;
  SD_HIP_CHECK(hipMalloc(&d, n_ints * sizeof(int32_t)));
  const int rc = launch_features_in_area(h->cur, h->tb, h->cam, frame, x, y, r, min_level, max_level, d, h->kp_cap, d + h->kp_cap, d + h->kp_cap + 1, s);
  std::vector<int32_t> host(n_ints);
  hipError_t e = hipMemcpyAsync(host.data(), d, n_ints * sizeof(int32_t), hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  (void)hipFree(d);
  SD_TRY(rc);
  if (e != hipSuccess) return hip_error("sd_track_debug_features_in_area", e);
  const int n = host[h->kp_cap];
  *n_out = n;
  SD_REQUIRE(n <= cap, SD_ERR_CAPACITY, "indices array too small");
  std::memcpy(indices, host.data(), (size_t)n * sizeof(int32_t));
  if (grid_counts) std::memcpy(grid_counts, host.data() + h->kp_cap + 1, 64 * 48 * sizeof(int32_t));
  return SD_OK;
}

// The batch's result records into a caller-owned DEVICE buffer (n_frames x 20 doubles), queued on the tracking stream
// behind the stages that produce them: no host round trip between the last tracking kernel and the collective that
// gathers the records.
int sd_track_pack_records(sd_track* h, int n_frames, int source, void* d_records) {
  SD_REQUIRE(h && d_records, SD_ERR_INVALID_ARG, "NULL argument");
  SD_REQUIRE(n_frames >= 1 && n_frames <= h->max_batch && source >= 0 && source <= 4, SD_ERR_INVALID_ARG, "bad n_frames / source");
  SD_HIP_CHECK(hipSetDevice(h->device));
  hipLaunchKernelGGL(k_pack_records, dim3((n_frames + 255) / 256), dim3(256), 0, h->pnp_stream, h->tb, source, n_frames, (double*)d_records);
  SD_HIP_CHECK(hipGetLastError());
  return SD_OK;
}

// Ordering against a caller's HIP stream (the stream its RCCL collectives run on).  direction 0: `hip_stream` waits for
// everything queued on the tracking stream so far (collective after the records are packed); 1: the tracking stream waits
// for everything queued on `hip_stream` so far (the next pack must not overwrite a buffer a collective is still reading).
int sd_track_stream_fence(sd_track* h, void* hip_stream, int direction) {
  SD_REQUIRE(h && (direction == 0 || direction == 1), SD_ERR_INVALID_ARG, "bad arguments");
  SD_HIP_CHECK(hipSetDevice(h->device));
  hipStream_t ext = (hipStream_t)hip_stream;   // NULL = the legacy default stream
  if (!h->ev_fence) SD_HIP_CHECK(hipEventCreateWithFlags(&h->ev_fence, hipEventDisableTiming));
  if (direction == 0) {
    SD_HIP_CHECK(hipEventRecord(h->ev_fence, h->pnp_stream));
    SD_HIP_CHECK(hipStreamWaitEvent(ext, h->ev_fence, 0));
  } else {
    SD_HIP_CHECK(hipEventRecord(h->ev_fence, ext));
    SD_HIP_CHECK(hipStreamWaitEvent(h->pnp_stream, h->ev_fence, 0));
  }
  return SD_OK;
}

int sd_track_get_extractors(sd_track* h, sd_orb** cur, sd_orb** ref) {
  SD_REQUIRE(h, SD_ERR_INVALID_ARG, "handle is NULL");
  if (cur) *cur = h->cur;
  if (ref) *ref = h->ref;
  return SD_OK;
}

int sd_track_set_profiling(sd_track* h, int on) {
  SD_REQUIRE(h, SD_ERR_INVALID_ARG, "handle is NULL");
  h->profiling = on != 0;
  h->ev_calls[0] = h->ev_calls[1] = h->ev_calls[2] = 0;
  return SD_OK;
}

// mean ms of the align / match / pnp launches since profiling was switched on
int sd_track_stage_ms(sd_track* h, float* ms_out, int cap) {
  SD_REQUIRE(h && ms_out && cap >= 3, SD_ERR_INVALID_ARG, "bad arguments");
  SD_REQUIRE(h->profiling, SD_ERR_INVALID_ARG, "profiling is off");
  SD_HIP_CHECK(hipSetDevice(h->device));
  SD_HIP_CHECK(hipStreamSynchronize(h->pnp_stream));
  SD_HIP_CHECK(hipStreamSynchronize(h->cur->stream));
  for (int k = 0; k < 3; k++) {
    ms_out[k] = 0;
    const int n = std::min(h->ev_calls[k], (int)sd_track::kRing);
    for (int r = 0; r < n; r++) {
      float ms = 0;
      const hipEvent_t* ev = stage_events(h, k, h->ev_calls[k] - 1 - r);
      SD_HIP_CHECK(hipEventElapsedTime(&ms, ev[0], ev[1]));
      ms_out[k] += ms / n;
    }
  }
  return SD_OK;
}

}  // extern "C"
