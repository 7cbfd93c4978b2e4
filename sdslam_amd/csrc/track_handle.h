// The sd_track handle and the host helpers its entry points share (track.hip: creation and the batched stages;
// track_seq.hip: sequential tracking).  Not part of the ABI.  In order: UploadRing and RunStamp (the sequential loop's two
// small types), the handle, what the cached results are stamped with and what ends them (inputs_now / END_RESULTS over track_results.h),
// wait_inputs / mark_reads (ordering against the extractors), the argument preambles (check_ready, check_batch / check_paired,
// check_range with TRACK_RANGE / QUEUE_RANGE, require_ref_frames), the stage timers and run_stage (the bracket every batched
// stage launches in), hip_error and Blob (the scaffold of the debug entries), and the typed copies between host arrays and the
// per-slot device buffers (download / upload, download_rows / upload_rows), whose byte counts come from the buffer's element type.
#pragma once
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>
#include <vector>

#include "orb_internal.h"
#include "track_internal.h"
#include "track_results.h"

// Small host arrays on their way into device memory without a host wait: the next of kSlots pinned buffers takes a copy, which
// goes to the device on the caller's stream, behind whatever that stream has queued.  A buffer is written again once the copy
// out of it has run (kSlots calls later: only then can the host wait).
struct UploadRing {
  static const int kSlots = 4;
  void* host[kSlots] = {};
  hipEvent_t ev[kSlots] = {};
  bool pending[kSlots] = {};
  int next = 0;
  size_t slot_bytes = 0;

  hipError_t create(size_t bytes) {
    slot_bytes = bytes;
    hipError_t e = hipSuccess;
    for (int r = 0; r < kSlots && e == hipSuccess; r++) {
      e = hipHostMalloc(&host[r], bytes, hipHostMallocDefault);
      if (e == hipSuccess) e = hipEventCreateWithFlags(&ev[r], hipEventDisableTiming);
    }
    return e;
  }
  void destroy() {
    for (int r = 0; r < kSlots; r++) {
      if (host[r]) (void)hipHostFree(host[r]);
      if (ev[r]) (void)hipEventDestroy(ev[r]);
    }
  }
  template <typename T>
  int upload(T* dst, const T* src, size_t count, hipStream_t s) {
    const size_t bytes = count * sizeof(T);
    SD_REQUIRE(bytes <= slot_bytes, SD_ERR_CAPACITY, "upload exceeds the pinned ring buffer");
    const int r = next;
    next = (r + 1) % kSlots;
    if (pending[r]) SD_HIP_CHECK(hipEventSynchronize(ev[r]));   // its copy of kSlots calls ago has run
    std::memcpy(host[r], src, bytes);
    SD_HIP_CHECK(hipMemcpyAsync(dst, host[r], bytes, hipMemcpyHostToDevice, s));
    SD_HIP_CHECK(hipEventRecord(ev[r], s));
    pending[r] = true;
    return SD_OK;
  }
};

// "This call ran on this extraction of `cur`, for slots < n" (mode / source: what the call was asked for, where a later call
// has to know).  An extraction of `cur` ends it, and sd_track_advance resets it.
struct RunStamp {
  const sd_orb* cur = nullptr;
  unsigned long long serial = 0;
  int n = 0, mode = 0, source = -1;
  inline void set(const sd_track* h, int n_frames, int mode_ = 0, int source_ = -1);
  inline bool covers(const sd_track* h, int n_frames) const;
};

struct sd_track {
  sd_orb* cur = nullptr;
  sd_orb* ref = nullptr;
  int max_points = 0, max_batch = 0, kp_cap = 0, device = 0;
  int rand_per_frame = 0;
  std::vector<int> rand_len;      // rand() values actually supplied per slot (sd_track_set_rand)
  // What the stages that cache a result between calls left, and on which inputs (track_results.h: stamps, and the table of
  // what ends them).  pnp: the solvers sd_track_pnp_iterate continues; sim3: those of sd_track_sim3_iterate; tri: the matches of
  // sd_track_get_triangulation_matches; triang: sd_track_get_triangulated / _get_new_points; fuse: sd_track_get_fuse;
  // refresh: sd_track_get_refreshed; append: sd_track_get_appended (and sd_track_get_new_points after an append).
  sd::Results res;
  sd::PnpParams pnp_params{};
  int pnp_iter_upper = 0;          // upper bound of mnIterations of the PnP solvers
  sd::Sim3Params sim3_params{};
  int sim3_max_its = 0, sim3_iter_upper = 0;   // maxIterations argument / upper bound of mnIterations of the Sim3 solvers
  UploadRing sim3_ring;            // [kp_cap + 1] int32: the mRansacMaxIts table of a sd_track_sim3 call
  int32_t* d_sim3_max_its = nullptr;
  std::vector<uint8_t> f12_set;    // [max_batch] sd_track_set_f12 has covered the slot
  sd::TriangBuffers nb{};
  std::vector<uint8_t> scw_set;    // [max_batch] sd_track_set_fuse_scw has covered the slot
  sd::FuseBuffers fu{};
  sd::RefreshBuffers rf{};         // sd_track_set_observations / _refresh_points (track_refresh.hip; refresh_create / refresh_destroy)
  sd::BaBuffers ba{};              // sd_track_local_ba's scratch (track_ba.hip; ba_create / ba_destroy / ba_grow)
  std::vector<uint8_t> ba_roles;   // [max_batch + 1] the roles of sd_track_set_ba_keyframes, the current keyframe's last
  int ba_n_ref = 0;                // its n_ref_frames
  bool ba_roles_set = false;
  unsigned long long ba_serial = 0;   // rf.serial of the lists the last bundle adjustment ran on
  sd::CullBuffers cu{};            // sd_track_cull_keyframes / _erase_observations (track_cull.hip; cull_create / cull_destroy / cull_grow)
  sd::TrackBuffers tb{};
  sd::TrackCam cam{};
  bool have_cam = false;
  float* d_sf = nullptr;
  float* d_inv_sf = nullptr;
  float* d_sigma2 = nullptr;
  float* d_inv_sigma2 = nullptr;
  float* d_scale_thr = nullptr;   // MapPoint::PredictScale breakpoints (see k_match_local)
  std::vector<void*> allocs;
  // The tracking kernels (align, match, PnP: latency-bound, few waves) run on their own stream, so
  // the extraction of the next batch on cur->stream overlaps them; `cur` is double-buffered
  // (orb_internal.h: output sets) and every tracking launch waits for the extraction it consumes
  // (ev_extract_done) and marks the sets it read (ev_set_free).
  hipStream_t pnp_stream = nullptr;
  bool profiling = false;
  hipEvent_t ev_fence = nullptr;   // sd_track_stream_fence
  // sequential tracking: what ran on the current extraction of `cur` --
  RunStamp ran[2];                 // [0] sd_track_with_motion_model, [1] sd_track_local_map (sd_track_advance's source)
  RunStamp close;                  // sd_track_close_points (sd_track_need_keyframe reads its counts)
  RunStamp made;                   // point creation (mode 2 sd_track_stereo_init, 1 sd_track_create_keyframe_points): advance hands its np_* on
  bool ids_on = false;             // sd_track_set_map_ids has been called: sd_track_local_map applies the seen-point exclusion
  // Both feed the tracking stream, so a setter queues behind the hand-off that wrote Tref without a host wait.  Two, because a
  // loop step issues several uploads behind the same tracking kernels: one shared ring would make the host wait within a step.
  UploadRing pose_ring;            // [max_batch][16] double: sd_track_set_prior, sd_track_set_measurements
  UploadRing small_ring;           // [max_batch][8] int32: sd_track_set_keyframe_state / _flags, sd_track_set_next_map_id
  double* d_prior = nullptr;       // [max_batch][16]
  int32_t* d_close = nullptr;      // [max_batch][2] sd_track_close_points: nTrackedClose, nNonTrackedClose
  int32_t* d_kf_stage = nullptr;   // [max_batch][8]
  // sd_track_set_sensor_model: which filter sd_track_motion_predict / _update / _restart run (per handle, as per Tracking)
  int sensor_model = SD_SENSOR_CONSTANT_VELOCITY;
  std::vector<uint8_t> meas_set;   // [max_batch] sd_track_set_measurements has covered the slot since the model was chosen
  static const int kRing = 128;
  hipEvent_t ev[kRing][6] = {};
  int ev_calls[3] = {0, 0, 0};
};

inline void RunStamp::set(const sd_track* h, int n_frames, int mode_, int source_) {
  *this = RunStamp{h->cur, h->cur->extract_serial, n_frames, mode_, source_};
}
inline bool RunStamp::covers(const sd_track* h, int n_frames) const {
  return cur == h->cur && serial == h->cur->extract_serial && n_frames <= n;
}

// track_refresh.hip: the observation block and its pinned mirror, which sd_track_set_observations may replace (not in `allocs`)
int refresh_create(sd_track* h);
void refresh_destroy(sd_track* h);
// track_ba.hip: the bundle adjustment's scratch (not in `allocs`: ba_grow replaces it when the observation block grows)
int ba_create(sd_track* h);
void ba_destroy(sd_track* h);
int ba_grow(sd_track* h, size_t n_obs);
// track_cull.hip: the culling's scratch (not in `allocs`: cull_grow replaces it when the observation block grows)
int cull_create(sd_track* h);
void cull_destroy(sd_track* h);
int cull_grow(sd_track* h, size_t n_obs);

// What a stage that runs now computes its result on: h->res.x.set(n, BIND_X, inputs_now(h)) after it, h->res.x.live(n, inputs_now(h)) later
static inline sd::ResultInputs inputs_now(const sd_track* h) { return {h->cur->extract_serial, h->ref->extract_serial, h->tb.cur_bcast}; }
// The entry point named ends the results of its row of kEnds
#define END_RESULTS(h, entry)                                                  \
  do {                                                                         \
    constexpr int ends_ = sd::ends_of(entry);                                  \
    static_assert(ends_ >= 0, "no row of kEnds (track_results.h) for " entry); \
    sd::end_results((h)->res, (unsigned)ends_);                                \
  } while (0)

// MapPoint::PredictScale (src/MapPoint.cc:355-385): nScale = ceil(log(ratio) / mfLogScaleFactor), float overloads,
// mfLogScaleFactor = log(mfScaleFactor) (src/Frame.cc:80).  thr[n] = smallest float ratio that reaches level n,
// by bisection over the float bit patterns with THIS host's libm (the function is monotone).
static inline void predict_scale_thresholds(float scale_factor, float (&thr)[SD_MAX_LEVELS]) {
  const float Lsf = logf(scale_factor);
  thr[0] = 0.f;
  for (int n = 1; n < SD_MAX_LEVELS; n++) {
    uint32_t lo = 1, hi = 0x7f800000u;   // hi = +inf: never reached
    while (lo < hi) {
      const uint32_t mid = lo + (hi - lo) / 2;
      float r;
      memcpy(&r, &mid, 4);
      const int ns = (int)ceilf(logf(r) / Lsf);
      if (ns >= n) hi = mid;
      else lo = mid + 1;
    }
    memcpy(&thr[n], &lo, 4);
  }
}

// "<the call `source` names> has not run on these slots since the last extraction"; 2: sd_track_stereo_init
static inline const char* not_run_msg(int source) {
  return source == 0   ? "sd_track_with_motion_model has not run on these slots since the last extraction"
         : source == 1 ? "sd_track_local_map has not run on these slots since the last extraction"
                       : "sd_track_stereo_init has not run on these slots since the last extraction";
}

// Order the tracking stream behind the extractions it consumes ...
static inline int wait_inputs(sd_track* h, bool need_ref, bool pyramid_only = false) {
  // ImageAlign reads pyramids only: it may start as soon as the current batch's pyramid exists, beside FAST / selection /
  // descriptors of the same batch (option "track.align_start" = 0 restores the wait for the whole extraction)
  const int align_start = sd::opt(sd::OPT_ALIGN_START);
  const bool early = align_start != 0;
  // ... but not beside FAST: k_align holds 30 KB of LDS per frame (4 frames per CU), FAST wants 24-39 KB per workgroup, while
  // selection + descriptors, which follow FAST, use next to none.  Waiting for the end of the batch's FAST launches instead of
  // its pyramid: full step 175.2 -> 178.8 k frames/s (three alternating runs; k_align 1.38 -> 0.84 ms in the pipeline).
  // "track.align_start" = 1: wait for the pyramid only; 2 (default): for the FAST launches.
  const bool after_fast = align_start == 2;
  if (h->cur->extract_recorded) {
    hipEvent_t ev = h->cur->ev_extract_done;
    if (pyramid_only && early && h->cur->pyr_event_live) ev = after_fast ? h->cur->ev_fast_done : h->cur->ev_pyr_done;
    SD_HIP_CHECK(hipStreamWaitEvent(h->pnp_stream, ev, 0));
  }
  if (need_ref && h->ref->extract_recorded) SD_HIP_CHECK(hipStreamWaitEvent(h->pnp_stream, h->ref->ev_extract_done, 0));
  return SD_OK;
}
// ... and tell the extractors which output sets the kernel just queued is reading.
static inline int mark_reads(sd_track* h, bool used_ref) {
  sd_orb* c = h->cur;
  SD_HIP_CHECK(hipEventRecord(c->ev_set_free[c->set], h->pnp_stream));
  c->set_busy[c->set] = true;
  if (used_ref && h->ref != h->cur) {
    sd_orb* r = h->ref;
    SD_HIP_CHECK(hipEventRecord(r->ev_set_free[r->set], h->pnp_stream));
    r->set_busy[r->set] = true;
  }
  return SD_OK;
}

// per_cur_frame: the call walks the frames of `cur` themselves (not tracker slots), so the broadcast does not apply
static inline int check_ready(sd_track* h, int n_frames, bool per_cur_frame = false) {
  SD_REQUIRE(h, SD_ERR_INVALID_ARG, "handle is NULL");
  SD_REQUIRE(h->have_cam, SD_ERR_INVALID_ARG, "sd_track_set_camera has not been called");
  SD_REQUIRE(n_frames >= 1 && n_frames <= h->max_batch, SD_ERR_CAPACITY, "n_frames exceeds max_batch");
  const int need = (h->tb.cur_bcast >= 0 && !per_cur_frame) ? h->tb.cur_bcast + 1 : n_frames;
  SD_REQUIRE(h->cur->have_geom && h->cur->last_frames >= need, SD_ERR_INVALID_ARG, "current frames have not been extracted");
  SD_HIP_CHECK(hipSetDevice(h->device));
  return SD_OK;
}

// The preamble of the sequential calls on slots < n_frames comes in pieces, because every entry point keeps the order of its
// checks and has argument and state checks of its own between them: the handle and the batch ...
static inline int check_batch(const sd_track* h, int n_frames) {
  SD_REQUIRE(h, SD_ERR_INVALID_ARG, "handle is NULL");
  SD_REQUIRE(n_frames >= 1 && n_frames <= h->max_batch, SD_ERR_CAPACITY, "n_frames exceeds max_batch");
  return SD_OK;
}
// ... "slot f pairs with current frame f" (the sequential loop never runs in broadcast mode) ... and hipSetDevice, last.
static inline int check_paired(const sd_track* h) {
  SD_REQUIRE(h->tb.cur_bcast < 0, SD_ERR_INVALID_ARG, "broadcast mode is on (sd_track_set_current_broadcast)");
  return SD_OK;
}

// The preamble of the calls on slots frame0 .. frame0 + n - 1: the range alone (the caller checks more before it sets the device),
// or the device too (the call queues on the tracking stream), or also a wait for that stream (the call touches what it uses).
enum RangeUse { RANGE_CHECK, RANGE_QUEUE, RANGE_SYNC };
static inline int check_range(const sd_track* h, int frame0, int n, RangeUse use) {
  SD_REQUIRE(h, SD_ERR_INVALID_ARG, "handle is NULL");
  SD_REQUIRE(frame0 >= 0 && n >= 1 && frame0 + n <= h->max_batch, SD_ERR_CAPACITY, "frame range exceeds max_batch");
  if (use != RANGE_CHECK) SD_HIP_CHECK(hipSetDevice(h->device));
  if (use == RANGE_SYNC) SD_HIP_CHECK(hipStreamSynchronize(h->pnp_stream));
  return SD_OK;
}
#define TRACK_RANGE(h, frame0, n) SD_TRY(check_range((h), (frame0), (n), RANGE_SYNC))
#define QUEUE_RANGE(h, frame0, n) SD_TRY(check_range((h), (frame0), (n), RANGE_QUEUE))

// Frames 0 .. n_frames - 1 of the `ref` extractor exist; same_size: and have the geometry of the current frames (ImageAlign);
// same_capacity: and a keypoint row of theirs is as long as one of `cur` (the two-extractor stages index both with kp_cap)
static inline int require_ref_frames(const sd_track* h, int n_frames, bool same_size, bool same_capacity = false) {
  const bool extracted = h->ref->have_geom && h->ref->last_frames >= n_frames;
  if (same_size)
    SD_REQUIRE(extracted && h->ref->cur_w == h->cur->cur_w && h->ref->cur_h == h->cur->cur_h, SD_ERR_INVALID_ARG,
               "reference frames not extracted or of different size");
  else
    SD_REQUIRE(extracted, SD_ERR_INVALID_ARG, "keyframes of the ref extractor have not been extracted");
  if (same_capacity)
    SD_REQUIRE(keypoint_capacity(h->ref) == h->kp_cap, SD_ERR_INVALID_ARG, "cur / ref extractors must share the keypoint capacity");
  return SD_OK;
}

// Stage timers (sd_track_set_profiling / sd_track_stage_ms): call number c of stage k records its start and stop on the tracking
// stream into events 2k and 2k + 1 of ring slot c % kRing.  stage_end counts the call whether or not its launch succeeded.
enum { STAGE_NONE = -1, STAGE_ALIGN = 0, STAGE_MATCH = 1, STAGE_SOLVE = 2 };
static inline hipEvent_t* stage_events(sd_track* h, int k, int call) { return &h->ev[call % sd_track::kRing][2 * k]; }
static inline int stage_begin(sd_track* h, int k) {
  if (h->profiling) SD_HIP_CHECK(hipEventRecord(stage_events(h, k, h->ev_calls[k])[0], h->pnp_stream));
  return SD_OK;
}
static inline int stage_end(sd_track* h, int k) {
  if (!h->profiling) return SD_OK;
  SD_HIP_CHECK(hipEventRecord(stage_events(h, k, h->ev_calls[k])[1], h->pnp_stream));
  h->ev_calls[k]++;
  return SD_OK;
}

// What every single-launch stage does once its entry point has checked its arguments (check_ready first, then its own checks:
// they stay in the entry point, in its order): wait for the extractions, launch(tracking stream) between the timer records of
// stage `timer` (STAGE_NONE: untimed), mark the output sets as read.  need_ref: the launch reads the ref extractor's frames too.
template <typename Launch>
static inline int run_stage(sd_track* h, bool need_ref, bool pyramid_only, int timer, Launch&& launch) {
  SD_TRY(wait_inputs(h, need_ref, pyramid_only));
  if (timer != STAGE_NONE) SD_TRY(stage_begin(h, timer));
  const int rc = launch(h->pnp_stream);
  if (timer != STAGE_NONE) SD_TRY(stage_end(h, timer));
  SD_TRY(rc);
  return mark_reads(h, need_ref);
}

// The host wait that ends a getter or setter: its copies have run
static inline int wait_for(hipStream_t s) {
  SD_HIP_CHECK(hipStreamSynchronize(s));
  return SD_OK;
}

// "<entry point>: <HIP's message>" where a call has to free what it allocated before it reports
static inline int hip_error(const char* name, hipError_t e) {
  sd::set_error(std::string(name) + ": " + hipGetErrorString(e));
  return SD_ERR_HIP;
}

// The device memory of a debug entry: one allocation carved in 16-byte steps, with a zeroed host mirror.  reserve every array
// (inputs with their source), run the launch on pointers from dev<T>(), take the outputs.
struct Blob {
  uint8_t* base = nullptr;
  std::vector<uint8_t> host;   // the mirror: its size is the allocation's
  // `count` elements of T, the first n of them copied from src; returns the array's offset
  template <typename T>
  size_t reserve(size_t count, const T* src = nullptr, size_t n = 0) {
    const size_t off = host.size();
    host.resize(off + ((count * sizeof(T) + 15) & ~(size_t)15), 0);
    put(off, src, n * sizeof(T));
    return off;
  }
  void put(size_t off, const void* src, size_t n) { if (n) std::memcpy(host.data() + off, src, n); }
  template <typename T>
  T* dev(size_t off) const { return (T*)(base + off); }
  // Allocate, copy the mirror in, launch() on the null stream, copy everything back, free -- whatever failed
  template <typename Launch>
  int run(const char* name, Launch&& launch) {
    SD_HIP_CHECK(hipMalloc(&base, host.size()));
    hipError_t e = hipMemcpy(base, host.data(), host.size(), hipMemcpyHostToDevice);
    int rc = SD_OK;
    if (e == hipSuccess) {
      rc = launch();
      if (rc == SD_OK) e = hipMemcpy(host.data(), base, host.size(), hipMemcpyDeviceToHost);
    }
    (void)hipFree(base);
    base = nullptr;
    return e != hipSuccess ? hip_error(name, e) : rc;
  }
  void take(void* dst, size_t off, size_t n) const { if (n) std::memcpy(dst, host.data() + off, n); }
};

// Slots frame0 .. frame0 + n - 1 of a device buffer with per_slot elements a slot, to / from a dense host array.  A NULL host
// pointer is an output the caller does not want / an input it leaves as it is: no copy.
template <typename T>
static inline int download(T* dst, const T* src, size_t frame0, size_t n, size_t per_slot, hipStream_t s) {
  if (dst) SD_HIP_CHECK(hipMemcpyAsync(dst, src + frame0 * per_slot, n * per_slot * sizeof(T), hipMemcpyDeviceToHost, s));
  return SD_OK;
}
template <typename T>
static inline int upload(T* dst, const T* src, size_t frame0, size_t n, size_t per_slot, hipStream_t s) {
  if (src) SD_HIP_CHECK(hipMemcpyAsync(dst + frame0 * per_slot, src, n * per_slot * sizeof(T), hipMemcpyHostToDevice, s));
  return SD_OK;
}
// The same where the host rows have a pitch of their own: n rows, the device's of K elements, the caller's of `cap` (>= K to
// read whole rows, <= K to write the first `cap` elements of each).  Pitches in elements, of any size.
template <typename T>
static inline int download_rows(T* dst, size_t cap, const T* src, size_t frame0, size_t n, size_t K, hipStream_t s) {
  if (dst)
    SD_HIP_CHECK(hipMemcpy2DAsync(dst, cap * sizeof(T), src + frame0 * K, K * sizeof(T), K * sizeof(T), n, hipMemcpyDeviceToHost, s));
  return SD_OK;
}
template <typename T>
static inline int upload_rows(T* dst, size_t K, const T* src, size_t cap, size_t frame0, size_t n, hipStream_t s) {
  SD_HIP_CHECK(hipMemcpy2DAsync(dst + frame0 * K, K * sizeof(T), src, cap * sizeof(T), cap * sizeof(T), n, hipMemcpyHostToDevice, s));
  return SD_OK;
}
