// sd_track_*: the sequential loop around the batched tracking calls of track.hip, on the device, so a stream of frames is
// tracked without a host round trip per frame (Tracking::Track, reference src/Tracking.cc:215-349): the last-frame hand-off
// (sd_track_advance), the RGB-D close-point counts and the keyframe decision, map point creation, the prior of the next
// frame and the two motion models.  Host side and three small kernels; the others: track_newpoints / _motion / _imu.hip.
#include <cmath>
#include <utility>

#include "track_handle.h"

using namespace sd;

// Tracking::Track's hand-off to the next frame (reference src/Tracking.cc:250-292), one workgroup per slot, into the second
// last-frame SoA (the host swaps the two afterwards: what is read and what is written overlap).  Keypoint i < N of the current
// frame keeps map point m = mvpMapPoints[i] -- source 0: cur_match after TrackWithMotionModel's outlier discard; 1: un_match
// after TrackLocalMap, m >= M naming local point m - M -- iff it is there, not an outlier (mvbOutlier, source 1) and has
// Observations() >= 1 ("Clean VO matches" :250-257, outliers :272-275).  Kept points carry Xw / descriptor / obs / id; the
// others zeros and id -1.  octave = mvKeys[i].octave, angle = mvKeysUn[i].angle; n_last = N; Tref = the frame's final pose,
// which both tracking tails leave in Tcur.  Slots >= n_frames keep their last frame (copied across).
// created_n > 0: a creation call (track_newpoints.hip) ran on this extraction for slots < created_n; a keypoint it gave a new
// point carries that point -- np_Xw, the keypoint's own descriptor (ComputeDistinctiveDescriptors with one observation),
// Observations() = 1, np_id -- whatever mvbOutlier[i] says.  source 2: after StereoInitialization mvpMapPoints are the
// created points only and Tref = the identity it left in Tcur; slots that did not initialise keep their last frame.
__global__ __launch_bounds__(256) void k_advance(const sd_keypoint* __restrict__ kps_all, const sd_keypoint* __restrict__ kps_un_all,
                                                 const int32_t* __restrict__ nkp_all, TrackBuffers tb, int source, int n_frames,
                                                 const uint8_t* __restrict__ desc_all, int created_n) {
  const int f = blockIdx.x, tid = threadIdx.x, NT = blockDim.x;
  const int M = tb.max_points, cap = tb.kp_cap;
  const size_t o = (size_t)f * M;
  if (f >= n_frames || (source == 2 && tb.np_info[(size_t)f * 4] != 2)) {
    for (int i = tid; i < M; i += NT) {
      const size_t e = o + i;
      tb.valid2[e] = tb.valid[e];
      for (int k = 0; k < 3; k++) tb.Xw2[e * 3 + k] = tb.Xw[e * 3 + k];
      ((uint4*)tb.mp_desc2)[e * 2] = ((const uint4*)tb.mp_desc)[e * 2];
      ((uint4*)tb.mp_desc2)[e * 2 + 1] = ((const uint4*)tb.mp_desc)[e * 2 + 1];
      tb.octave2[e] = tb.octave[e];
      tb.angle2[e] = tb.angle[e];
      tb.obs2[e] = tb.obs[e];
      tb.last_id2[e] = tb.last_id[e];
    }
    return;
  }
  const int N = min(nkp_all[f], cap);   // cap <= M (sd_track_advance)
  const int32_t* match = (source == 0 ? tb.cur_match : tb.un_match) + (size_t)f * cap;
  const uint8_t* outl = tb.po_outlier + (size_t)f * cap;
  const uint8_t* made = f < created_n ? tb.np_flag + (size_t)f * cap : nullptr;
  for (int i = tid; i < M; i += NT) {
    uint8_t v = 0;
    double X0 = 0, X1 = 0, X2 = 0;
    int ob = 0, id = -1, oct = 0;
    float ang = 0.f;
    uint4 d0 = make_uint4(0, 0, 0, 0), d1 = d0;
    if (i < N) {
      oct = kps_all[(size_t)f * cap + i].octave;
      ang = kps_un_all[(size_t)f * cap + i].angle;
      bool loc = false;
      size_t e = 0;
      const bool is_new = made && made[i];
      const int n_obs = (is_new || source == 2) ? 0 : kept_point_obs(tb, source, match[i], outl + i, o, &e, &loc);
      if (is_new) {
        const size_t k = (size_t)f * cap + i;
        const uint4* d = (const uint4*)desc_all + k * 2;
        v = 1;
        X0 = tb.np_Xw[k * 3]; X1 = tb.np_Xw[k * 3 + 1]; X2 = tb.np_Xw[k * 3 + 2];
        d0 = d[0]; d1 = d[1];
        ob = 1;
        id = tb.np_id[k];
      } else if (n_obs >= 1) {
        const double* X = (loc ? tb.lm_Xw : tb.Xw) + e * 3;
        const uint4* d = (const uint4*)(loc ? tb.lm_desc : tb.mp_desc) + e * 2;
        v = 1;
        X0 = X[0]; X1 = X[1]; X2 = X[2];
        d0 = d[0]; d1 = d[1];
        ob = n_obs;
        id = loc ? tb.lm_id[e] : tb.last_id[e];
      }
    }
    const size_t e = o + i;
    tb.valid2[e] = v;
    tb.Xw2[e * 3] = X0;
    tb.Xw2[e * 3 + 1] = X1;
    tb.Xw2[e * 3 + 2] = X2;
    ((uint4*)tb.mp_desc2)[e * 2] = d0;
    ((uint4*)tb.mp_desc2)[e * 2 + 1] = d1;
    tb.octave2[e] = oct;
    tb.angle2[e] = ang;
    tb.obs2[e] = ob;
    tb.last_id2[e] = id;
  }
  if (tid == 0) tb.n_last[f] = N;
  if (tid < 16) tb.Tref[(size_t)f * 16 + tid] = tb.Tcur[(size_t)f * 16 + tid];
}

// Tracking::NeedNewKeyFrame's RGB-D counts (reference src/Tracking.cc:776-789), which run after "Clean VO matches"
// (:250-257): over keypoints i < N with 0 < mvDepth[i] < th_depth, nTrackedClose = those whose map point k_advance keeps
// (kept_point_obs) and nNonTrackedClose = the others.  One workgroup per slot; each wave counts with two ballots per 64
// keypoints, the four waves' sums meet in LDS.
__global__ __launch_bounds__(256) void k_close_points(const int32_t* __restrict__ nkp_all, TrackBuffers tb, int source, float th_depth,
                                                      int32_t* __restrict__ out) {
  __shared__ int s_n[2][4];
  const int f = blockIdx.x, tid = threadIdx.x, wave = tid >> 6;
  const int M = tb.max_points, cap = tb.kp_cap;
  const size_t o = (size_t)f * M;
  const int N = min(nkp_all[f], cap);
  const float* depth = tb.depth + (size_t)f * cap;
  const int32_t* match = (source == 0 ? tb.cur_match : tb.un_match) + (size_t)f * cap;
  const uint8_t* outl = tb.po_outlier + (size_t)f * cap;
  int tracked = 0, other = 0;
  for (int base = 0; base < N; base += 256) {   // trip count uniform over the workgroup: the ballots see every lane
    const int i = base + tid;
    bool close = false, kept = false;
    if (i < N) {
      const float d = depth[i];
      close = d > 0 && d < th_depth;
      bool loc;
      size_t e;
      if (close) kept = kept_point_obs(tb, source, match[i], outl + i, o, &e, &loc) >= 1;
    }
    const unsigned long long bc = __ballot(close), bk = __ballot(kept);
    tracked += __popcll(bk);
    other += __popcll(bc & ~bk);
  }
  if ((tid & 63) == 0) {
    s_n[0][wave] = tracked;
    s_n[1][wave] = other;
  }
  __syncthreads();
  if (tid < 2) out[(size_t)f * 2 + tid] = s_n[tid][0] + s_n[tid][1] + s_n[tid][2] + s_n[tid][3];
}

// sd_track_set_prior: Tprior = Tcur = T (relative 0) or T * Tref (relative 1: ConstantVelocity::GetPose, Exp(vel) * last_pose_),
// column-major; each entry sums k = 0..3 in order with explicit roundings (no FMA contraction), as a plain host loop does.
__global__ void k_set_prior(const double* __restrict__ Tin, TrackBuffers tb, int frame0, int n, int relative) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n * 16) return;
  const int f = frame0 + t / 16, e = t % 16, c = e / 4, r = e % 4;
  const double* T = Tin + (size_t)(t / 16) * 16;
  double v = T[e];
  if (relative) v = pose_product_entry(T, tb.Tref + (size_t)f * 16, r, c);
  tb.Tprior[(size_t)f * 16 + e] = v;
  tb.Tcur[(size_t)f * 16 + e] = v;
}

extern "C" {

// ---- sequential tracking: the last-frame hand-off on the device (Tracking::Track, src/Tracking.cc:250-292)

int sd_track_set_map_ids(sd_track* h, int frame0, int n_frames, int which, const int32_t* ids, int cap) {
  TRACK_RANGE(h, frame0, n_frames);
  SD_REQUIRE(which == 0 || which == 1, SD_ERR_INVALID_ARG, "which must be 0 (last-frame points) or 1 (local map points)");
  SD_REQUIRE(ids && cap >= 1 && cap <= h->max_points, SD_ERR_INVALID_ARG, "bad id array (cap must be 1..max_points)");
  const size_t M = h->max_points;
  int32_t* dst = which == 0 ? h->tb.last_id : h->tb.lm_id;
  hipStream_t s = h->cur->stream;
  SD_HIP_CHECK(hipMemsetAsync(dst + (size_t)frame0 * M, 0xFF, (size_t)n_frames * M * sizeof(int32_t), s));
  SD_TRY(upload_rows(dst, M, ids, cap, frame0, n_frames, s));
  SD_HIP_CHECK(hipStreamSynchronize(s));
  h->ids_on = true;
  return SD_OK;
}

int sd_track_advance(sd_track* h, int n_frames, int source) {
  SD_TRY(check_batch(h, n_frames));
  SD_REQUIRE(source >= 0 && source <= 2, SD_ERR_INVALID_ARG,
             "source must be 0 (sd_track_with_motion_model), 1 (sd_track_local_map) or 2 (sd_track_stereo_init)");
  SD_REQUIRE(h->kp_cap <= h->max_points, SD_ERR_CAPACITY, "the keypoint capacity exceeds max_points: a last frame would not fit");
  SD_TRY(check_paired(h));
  // a creation call on this extraction, whatever its slots: its points go with the keypoints that received them
  const bool made = h->made.covers(h, 0);
  if (source == 2) {
    SD_REQUIRE(made && h->made.mode == 2 && n_frames <= h->made.n, SD_ERR_INVALID_ARG, not_run_msg(2));
  } else {
    SD_REQUIRE(h->ran[source].covers(h, n_frames), SD_ERR_INVALID_ARG, not_run_msg(source));
    SD_REQUIRE(!made || (h->made.mode == 1 && h->made.source == source), SD_ERR_INVALID_ARG,
               "map points were created on this extraction from another source (sd_track_stereo_init: advance with source 2)");
  }
  const int created_n = made ? h->made.n : 0;
  SD_REQUIRE(keypoint_capacity(h->ref) == h->kp_cap && h->cur->max_batch >= h->max_batch, SD_ERR_INVALID_ARG,
             "cur / ref extractors must share the keypoint capacity and hold max_batch frames to swap roles");
  SD_HIP_CHECK(hipSetDevice(h->device));
  // the new `cur` is extracted into next while tracking kernels may still read its last output set: it needs two
  SD_TRY(orb_enable_double_buffer(h->ref));
  SD_TRY(wait_inputs(h, false));
  const sd_orb* c = h->cur;
  hipLaunchKernelGGL(k_advance, dim3(h->max_batch), dim3(256), 0, h->pnp_stream, c->d_kps, keys_un(c), c->d_nout, h->tb, source,
                     n_frames, c->d_desc, created_n);
  SD_HIP_CHECK(hipGetLastError());
  SD_TRY(mark_reads(h, false));
  TrackBuffers& tb = h->tb;   // launches queued from now on see the new last frame
  std::swap(tb.valid, tb.valid2);
  std::swap(tb.Xw, tb.Xw2);
  std::swap(tb.mp_desc, tb.mp_desc2);
  std::swap(tb.octave, tb.octave2);
  std::swap(tb.angle, tb.angle2);
  std::swap(tb.obs, tb.obs2);
  std::swap(tb.last_id, tb.last_id2);
  std::swap(h->cur, h->ref);   // this frame's pyramid and keypoints are the next ImageAlign / match reference
  if (h->cur != h->ref) h->res.swap_roles();
  END_RESULTS(h, "sd_track_advance");
  h->ran[0] = h->ran[1] = h->close = h->made = RunStamp{};   // nothing has run on the new `cur` yet
  return SD_OK;
}

int sd_track_close_points(sd_track* h, int n_frames, int source, float th_depth) {
  SD_TRY(check_batch(h, n_frames));
  SD_REQUIRE(source == 0 || source == 1, SD_ERR_INVALID_ARG, "source must be 0 (sd_track_with_motion_model) or 1 (sd_track_local_map)");
  SD_TRY(check_paired(h));
  // (a call that ran in broadcast mode may have covered more slots than `cur` holds frames: its keypoint counts end there)
  SD_REQUIRE(h->ran[source].covers(h, n_frames) && h->cur->last_frames >= n_frames, SD_ERR_INVALID_ARG, not_run_msg(source));
  SD_HIP_CHECK(hipSetDevice(h->device));
  SD_TRY(wait_inputs(h, false));
  hipLaunchKernelGGL(k_close_points, dim3(n_frames), dim3(256), 0, h->pnp_stream, h->cur->d_nout, h->tb, source, th_depth, h->d_close);
  SD_HIP_CHECK(hipGetLastError());
  h->close.set(h, n_frames, 0, source);
  return mark_reads(h, false);
}

int sd_track_get_close_points(sd_track* h, int frame0, int n_frames, int32_t* out2) {
  TRACK_RANGE(h, frame0, n_frames);
  SD_REQUIRE(out2, SD_ERR_INVALID_ARG, "NULL argument");
  SD_TRY(download(out2, h->d_close, frame0, n_frames, 2, h->cur->stream));
  return wait_for(h->cur->stream);
}

// ---- RGB-D map point creation and the keyframe decision on the device (kernels: track_newpoints.hip)

int sd_track_set_next_map_id(sd_track* h, int frame0, int n_frames, const int32_t* next_id) {
  SD_REQUIRE(h && next_id, SD_ERR_INVALID_ARG, "NULL argument");
  QUEUE_RANGE(h, frame0, n_frames);
  return h->small_ring.upload(h->tb.next_id + frame0, next_id, (size_t)n_frames, h->pnp_stream);
}

int sd_track_set_keyframe_state(sd_track* h, int frame0, int n_frames, const int32_t* state8) {
  SD_REQUIRE(h && state8, SD_ERR_INVALID_ARG, "NULL argument");
  QUEUE_RANGE(h, frame0, n_frames);
  SD_TRY(h->small_ring.upload(h->d_kf_stage, state8, (size_t)n_frames * 8, h->pnp_stream));
  return launch_set_keyframe_state(h->tb, h->d_kf_stage, frame0, n_frames, h->pnp_stream);
}

int sd_track_set_keyframe_flags(sd_track* h, int frame0, int n_frames, const uint8_t* flags) {
  SD_REQUIRE(h && flags, SD_ERR_INVALID_ARG, "NULL argument");
  QUEUE_RANGE(h, frame0, n_frames);
  return h->small_ring.upload(h->tb.kf_flags + frame0, flags, (size_t)n_frames, h->pnp_stream);
}

int sd_track_get_keyframe_flags(sd_track* h, int frame0, int n_frames, uint8_t* flags) {
  TRACK_RANGE(h, frame0, n_frames);
  SD_REQUIRE(flags, SD_ERR_INVALID_ARG, "NULL argument");
  SD_TRY(download(flags, h->tb.kf_flags, frame0, n_frames, 1, h->cur->stream));
  return wait_for(h->cur->stream);
}

int sd_track_need_keyframe(sd_track* h, int n_frames, int rgbd, int frame_id, int min_frames, int max_frames) {
  SD_TRY(check_batch(h, n_frames));
  SD_TRY(check_paired(h));
  SD_REQUIRE(h->ran[1].covers(h, n_frames), SD_ERR_INVALID_ARG, not_run_msg(1));
  SD_REQUIRE(!rgbd || (h->close.covers(h, n_frames) && h->close.source == 1), SD_ERR_INVALID_ARG,
             "sd_track_close_points (source 1) has not run on these slots since the last extraction");
  SD_HIP_CHECK(hipSetDevice(h->device));
  return launch_need_keyframe(h->tb, h->d_close, n_frames, rgbd != 0, frame_id, min_frames, max_frames, h->pnp_stream);
}

static int new_points(sd_track* h, int n_frames, int mode, int source, float th_depth, int use_flags, int frame_id, int min_keypoints) {
  SD_TRY(wait_inputs(h, false));
  // Frame::invfx = 1.0f / fx (src/Frame.cc:90), rounded on the host
  SD_TRY(launch_new_points(h->cur, h->tb, h->cam, 1.0f / h->cam.ffx, 1.0f / h->cam.ffy, n_frames, mode, source, th_depth, use_flags, frame_id,
                           min_keypoints, h->pnp_stream));
  h->made.set(h, n_frames, mode, source);
  return mark_reads(h, false);
}

int sd_track_stereo_init(sd_track* h, int n_frames, int min_keypoints) {
  SD_TRY(check_batch(h, n_frames));
  SD_REQUIRE(h->have_cam, SD_ERR_INVALID_ARG, "sd_track_set_camera has not been called");
  SD_TRY(check_paired(h));
  SD_REQUIRE(h->cur->have_geom && h->cur->last_frames >= n_frames, SD_ERR_INVALID_ARG, "current frames have not been extracted");
  SD_HIP_CHECK(hipSetDevice(h->device));
  END_RESULTS(h, "sd_track_stereo_init");
  return new_points(h, n_frames, 2, 0, 0.f, 0, 0, min_keypoints);
}

int sd_track_create_keyframe_points(sd_track* h, int n_frames, int source, float th_depth, int use_flags, int frame_id) {
  SD_TRY(check_batch(h, n_frames));
  SD_REQUIRE(source == 0 || source == 1, SD_ERR_INVALID_ARG, "source must be 0 (sd_track_with_motion_model) or 1 (sd_track_local_map)");
  SD_TRY(check_paired(h));
  SD_REQUIRE(h->ran[source].covers(h, n_frames) && h->cur->last_frames >= n_frames, SD_ERR_INVALID_ARG, not_run_msg(source));
  SD_HIP_CHECK(hipSetDevice(h->device));
  return new_points(h, n_frames, 1, source, th_depth, use_flags != 0, frame_id, 0);
}

int sd_track_get_created(sd_track* h, int frame0, int n_frames, int32_t* info4, int32_t* kp_index, double* Xw, int32_t* ids, int cap) {
  TRACK_RANGE(h, frame0, n_frames);
  SD_REQUIRE(info4 && cap >= 0, SD_ERR_INVALID_ARG, "bad arguments");
  const size_t K = h->kp_cap, n = n_frames, o = frame0;
  const TrackBuffers& tb = h->tb;
  hipStream_t s = h->cur->stream;
  std::vector<int32_t> list(n * K), id(n * K);
  std::vector<double> X(n * K * 3);
  SD_TRY(download(info4, tb.np_info, o, n, 4, s));
  SD_TRY(download(list.data(), tb.np_list, o, n, K, s));
  SD_TRY(download(id.data(), tb.np_id, o, n, K, s));
  SD_TRY(download(X.data(), tb.np_Xw, o, n, K * 3, s));
  SD_HIP_CHECK(hipStreamSynchronize(s));
  for (size_t f = 0; f < n; f++) SD_REQUIRE(info4[f * 4 + 1] <= cap, SD_ERR_CAPACITY, "cap is smaller than a slot's number of created points");
  for (size_t f = 0; f < n; f++)
    for (int r = 0; r < info4[f * 4 + 1]; r++) {   // creation order
      const size_t i = (size_t)list[f * K + r], d = f * (size_t)cap + r;
      if (kp_index) kp_index[d] = (int32_t)i;
      if (ids) ids[d] = id[f * K + i];
      if (Xw) std::memcpy(Xw + d * 3, &X[(f * K + i) * 3], 3 * sizeof(double));
    }
  return SD_OK;
}

int sd_track_set_prior(sd_track* h, int frame0, int n_frames, const double* T_cm, int relative) {
  SD_REQUIRE(h && T_cm, SD_ERR_INVALID_ARG, "NULL argument");
  SD_TRY(check_range(h, frame0, n_frames, RANGE_CHECK));
  SD_REQUIRE(relative == 0 || relative == 1, SD_ERR_INVALID_ARG, "relative must be 0 or 1");
  SD_HIP_CHECK(hipSetDevice(h->device));
  SD_TRY(h->pose_ring.upload(h->d_prior, T_cm, (size_t)n_frames * 16, h->pnp_stream));
  hipLaunchKernelGGL(k_set_prior, dim3((n_frames * 16 + 255) / 256), dim3(256), 0, h->pnp_stream, h->d_prior, h->tb, frame0, n_frames, relative);
  SD_HIP_CHECK(hipGetLastError());
  return SD_OK;
}

// ---- motion model on the device (kernels: track_motion.hip)

int sd_track_motion_predict(sd_track* h, int n_frames, double dt) {
  SD_TRY(check_batch(h, n_frames));
  SD_REQUIRE(std::isfinite(dt) && dt >= 0.0, SD_ERR_INVALID_ARG, "dt must be finite and not negative");
  SD_TRY(check_paired(h));
  SD_HIP_CHECK(hipSetDevice(h->device));
  if (h->sensor_model == SD_SENSOR_IMU) return launch_imu_predict(h->tb, n_frames, dt, h->pnp_stream);
  return launch_motion_predict(h->tb, n_frames, dt, h->pnp_stream);
}

int sd_track_motion_update(sd_track* h, int n_frames, int source) {
  SD_TRY(check_batch(h, n_frames));
  SD_REQUIRE(source >= -1 && source <= 1, SD_ERR_INVALID_ARG,
             "source must be -1 (every slot tracked), 0 (sd_track_with_motion_model) or 1 (sd_track_local_map)");
  SD_TRY(check_paired(h));
  SD_REQUIRE(source < 0 || h->ran[source].covers(h, n_frames), SD_ERR_INVALID_ARG, not_run_msg(source));
  if (h->sensor_model == SD_SENSOR_IMU)   // the reference asserts on the size of measurements_ (IMU::Z)
    for (int f = 0; f < n_frames; f++)
      SD_REQUIRE(h->meas_set[f], SD_ERR_INVALID_ARG, "sd_track_set_measurements has not covered these slots since the IMU model was chosen");
  SD_HIP_CHECK(hipSetDevice(h->device));
  if (h->sensor_model == SD_SENSOR_IMU) return launch_imu_update(h->tb, n_frames, source, h->pnp_stream);
  return launch_motion_update(h->tb, n_frames, source, h->pnp_stream);
}

int sd_track_motion_restart(sd_track* h, int frame0, int n_frames) {
  QUEUE_RANGE(h, frame0, n_frames);
  if (h->sensor_model == SD_SENSOR_IMU) return launch_imu_init(h->tb, frame0, n_frames, 0, h->pnp_stream);
  return launch_motion_init(h->tb, frame0, n_frames, h->pnp_stream);
}

int sd_track_get_motion(sd_track* h, int frame0, int n_frames, double* X6, double* Pdiag6, int32_t* started, double* it_time,
                        double* E_cm, double* last_pose_cm) {
  SD_REQUIRE(!h || h->sensor_model == SD_SENSOR_CONSTANT_VELOCITY, SD_ERR_INVALID_ARG, "the IMU sensor model is selected: sd_track_get_imu");
  TRACK_RANGE(h, frame0, n_frames);
  hipStream_t s = h->cur->stream;
  const TrackBuffers& tb = h->tb;
  const size_t o = frame0, n = n_frames;
  SD_TRY(download(X6, tb.mo_X, o, n, 6, s));
  SD_TRY(download(Pdiag6, tb.mo_P, o, n, 6, s));
  SD_TRY(download(started, tb.mo_started, o, n, 1, s));
  SD_TRY(download(it_time, tb.mo_it, o, n, 1, s));
  SD_TRY(download(E_cm, tb.mo_E, o, n, 16, s));
  SD_TRY(download(last_pose_cm, tb.mo_last, o, n, 16, s));
  return wait_for(s);
}

int sd_track_set_motion(sd_track* h, int frame0, int n_frames, const double* X6, const double* Pdiag6, const int32_t* started,
                        const double* it_time) {
  SD_REQUIRE(!h || h->sensor_model == SD_SENSOR_CONSTANT_VELOCITY, SD_ERR_INVALID_ARG, "the IMU sensor model is selected: sd_track_set_imu");
  TRACK_RANGE(h, frame0, n_frames);
  hipStream_t s = h->cur->stream;
  const TrackBuffers& tb = h->tb;
  const size_t o = frame0, n = n_frames;
  SD_TRY(upload(tb.mo_X, X6, o, n, 6, s));
  SD_TRY(upload(tb.mo_P, Pdiag6, o, n, 6, s));
  SD_TRY(upload(tb.mo_started, started, o, n, 1, s));
  SD_TRY(upload(tb.mo_it, it_time, o, n, 1, s));
  return wait_for(s);
}

// ---- the IMU sensor model (kernels: track_imu.hip)

int sd_track_set_sensor_model(sd_track* h, int model) {
  SD_REQUIRE(h, SD_ERR_INVALID_ARG, "handle is NULL");
  SD_REQUIRE(model == SD_SENSOR_CONSTANT_VELOCITY || model == SD_SENSOR_IMU, SD_ERR_INVALID_ARG,
             "model must be SD_SENSOR_CONSTANT_VELOCITY or SD_SENSOR_IMU");
  SD_HIP_CHECK(hipSetDevice(h->device));
  // a new Tracking constructs its EKF: every slot's filter of the chosen model restarts
  SD_TRY(model == SD_SENSOR_IMU ? launch_imu_init(h->tb, 0, h->max_batch, 1, h->pnp_stream)
                                : launch_motion_init(h->tb, 0, h->max_batch, h->pnp_stream));
  h->sensor_model = model;
  h->meas_set.assign((size_t)h->max_batch, 0);
  return SD_OK;
}

int sd_track_get_sensor_model(sd_track* h, int* model) {
  SD_REQUIRE(h && model, SD_ERR_INVALID_ARG, "NULL argument");
  *model = h->sensor_model;
  return SD_OK;
}

// Tracking::SetMeasurements for slots frame0 .. frame0 + n_frames - 1
int sd_track_set_measurements(sd_track* h, int frame0, int n_frames, const double* wa6) {
  SD_REQUIRE(h && wa6, SD_ERR_INVALID_ARG, "NULL argument");
  SD_TRY(check_range(h, frame0, n_frames, RANGE_CHECK));
  SD_REQUIRE(h->sensor_model == SD_SENSOR_IMU, SD_ERR_INVALID_ARG, "the constant-velocity model takes no measurements (sd_track_set_sensor_model)");
  for (size_t i = 0; i < (size_t)n_frames * 6; i++) SD_REQUIRE(std::isfinite(wa6[i]), SD_ERR_INVALID_ARG, "measurements must be finite");
  SD_HIP_CHECK(hipSetDevice(h->device));
  SD_TRY(h->pose_ring.upload(h->tb.im_meas + (size_t)frame0 * 6, wa6, (size_t)n_frames * 6, h->pnp_stream));
  for (int f = frame0; f < frame0 + n_frames; f++) h->meas_set[f] = 1;
  return SD_OK;
}

int sd_track_get_imu(sd_track* h, int frame0, int n_frames, double* X16, double* P256, double* gravity3, int32_t* started, double* it_time,
                     double* last_pose_cm, double* measurements6) {
  TRACK_RANGE(h, frame0, n_frames);
  hipStream_t s = h->cur->stream;
  const TrackBuffers& tb = h->tb;
  const size_t o = frame0, n = n_frames;
  SD_TRY(download(X16, tb.im_X, o, n, 16, s));
  SD_TRY(download(P256, tb.im_P, o, n, 256, s));
  SD_TRY(download(gravity3, tb.im_g, o, n, 3, s));
  SD_TRY(download(started, tb.im_started, o, n, 1, s));
  SD_TRY(download(it_time, tb.im_it, o, n, 1, s));
  SD_TRY(download(last_pose_cm, tb.im_last, o, n, 16, s));
  SD_TRY(download(measurements6, tb.im_meas, o, n, 6, s));
  return wait_for(s);
}

int sd_track_set_imu(sd_track* h, int frame0, int n_frames, const double* X16, const double* P256, const double* gravity3,
                     const int32_t* started, const double* it_time) {
  SD_REQUIRE(!h || h->sensor_model == SD_SENSOR_IMU, SD_ERR_INVALID_ARG, "the constant-velocity model is selected: sd_track_set_motion");
  TRACK_RANGE(h, frame0, n_frames);
  hipStream_t s = h->cur->stream;
  const TrackBuffers& tb = h->tb;
  const size_t o = frame0, n = n_frames;
  SD_TRY(upload(tb.im_X, X16, o, n, 16, s));
  SD_TRY(upload(tb.im_P, P256, o, n, 256, s));
  SD_TRY(upload(tb.im_g, gravity3, o, n, 3, s));
  SD_TRY(upload(tb.im_started, started, o, n, 1, s));
  SD_TRY(upload(tb.im_it, it_time, o, n, 1, s));
  return wait_for(s);
}

int sd_track_get_last(sd_track* h, int frame0, int n_frames, int32_t* n_last, uint8_t* valid, double* Xw, uint8_t* desc, int32_t* octave,
                      float* angle, int32_t* obs, int32_t* ids) {
  TRACK_RANGE(h, frame0, n_frames);
  hipStream_t s = h->cur->stream;
  const TrackBuffers& tb = h->tb;
  const size_t M = h->max_points, o = frame0, n = n_frames;
  SD_TRY(download(n_last, tb.n_last, o, n, 1, s));
  SD_TRY(download(valid, tb.valid, o, n, M, s));
  SD_TRY(download(Xw, tb.Xw, o, n, M * 3, s));
  SD_TRY(download(desc, tb.mp_desc, o, n, M * 32, s));
  SD_TRY(download(octave, tb.octave, o, n, M, s));
  SD_TRY(download(angle, tb.angle, o, n, M, s));
  SD_TRY(download(obs, tb.obs, o, n, M, s));
  SD_TRY(download(ids, tb.last_id, o, n, M, s));
  return wait_for(s);
}

}  // extern "C"
