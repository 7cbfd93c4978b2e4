// Internal layout of the sd_orb handle and what orb.hip (kernels + launch pipeline) and orb_host.hip (handle + C ABI) share; the
// sd_track sources read the handle through track_handle.h.  Not part of the ABI.
#pragma once
#include <hip/hip_runtime.h>

#include <array>
#include <cstring>

#include "orb_plan.h"
#include "sd_common.h"

enum { ST_PYR = 0, ST_FAST, ST_SELECT, ST_BLUR, ST_DESC, ST_COUNT };
// Stage events of one profiled call (sd_orb::ev): pyramid on the stream the resize chain runs on, FAST on the fast stream,
// blur on the auxiliary stream, selection and descriptors on the main stream.
enum StageEvent {
  EV_PYR_BEGIN = 0, EV_PYR_END, EV_FAST_END, EV_BLUR_BEGIN, EV_DESC_BEGIN, EV_DESC_END, EV_BLUR_END, EV_SELECT_END, EV_FAST_BEGIN,
  EV_SELECT_BEGIN, EV_STAGE_COUNT
};

// Limits of the kernels that the host layer checks a planned geometry / addresses a buffer against
#define SEL_MAX_CELLS 512   // grid cells of one level (k_select_quota: one lane per level, four ints per cell in LDS)
#define SD_BLUR_SHIFT 1     // column offset of the blurred levels against the pyramid's layout (see k_blur)

struct sd_orb {
  int nfeatures, nlevels, thFAST;
  float scaleFactor;
  int max_w, max_h, max_batch, device;
  sd::HostPlan hp;
  bool have_geom = false;
  int cur_w = 0, cur_h = 0;
  int last_frames = 0;
  hipStream_t own_stream = nullptr, stream = nullptr;
  // blur depends only on the pyramid: it runs on aux_stream beside FAST + selection
  hipStream_t aux_stream = nullptr;
  hipEvent_t ev_pyr_done = nullptr, ev_blur_done = nullptr;
  // FAST of level l needs only level l of the pyramid: it runs on fast_stream as soon as that level is complete,
  // beside the (small, dependent) resize launches of the remaining levels
  hipStream_t fast_stream = nullptr;
  hipEvent_t ev_level[SD_MAX_LEVELS] = {};
  hipEvent_t ev_fast_done = nullptr;
  hipEvent_t ev_select_done = nullptr, ev_body_start = nullptr;   // end of a call's selection (d_cand free again) / start of a call on `stream`
  bool select_recorded = false;
  // Output sets.  What a tracker reads (padded pyramid, keypoints, descriptors, counts) exists once
  // or -- after sd::orb_enable_double_buffer, which sd_track_create calls on its `cur` handle -- twice:
  // extraction alternates between the sets, so batch n+1 is extracted on `stream` while the tracker
  // still works on batch n on its own stream.  d_pyr / d_kps / d_kps_un / d_desc / d_nout below always
  // alias the set of the most recent extraction.  A tracker records ev_set_free[set] after every
  // kernel that reads a set; the extraction that is about to overwrite that set waits for it.
  int nsets = 1, set = 0;
  uint8_t* pyr_set[2] = {nullptr, nullptr};
  sd_keypoint* kps_set[2] = {nullptr, nullptr};
  sd_keypoint* kps_un_set[2] = {nullptr, nullptr};
  uint8_t* desc_set[2] = {nullptr, nullptr};
  int32_t* nout_set[2] = {nullptr, nullptr};
  hipEvent_t ev_set_free[2] = {nullptr, nullptr};
  bool set_busy[2] = {false, false};
  hipEvent_t ev_user_fence[2] = {nullptr, nullptr};   // sd_orb_stream_fence
  hipEvent_t ev_extract_done = nullptr;   // end of the most recent extraction on `stream`
  bool extract_recorded = false;
  unsigned long long extract_serial = 0;  // extractions launched so far (a tracker checks that its inputs have not been replaced)
  bool pyr_event_live = false;            // ev_pyr_done of the most recent extraction is a real record (not a captured graph node)
  // device buffers
  sd::OrbPlan* d_plan = nullptr;
  sd::CellGeom* d_cells = nullptr;
  sd::BlurTile* d_tiles = nullptr;
  int32_t* d_coef = nullptr;
  uint8_t* d_img = nullptr;     // staging for host-input calls
  uint8_t* d_pyr = nullptr;
  uint8_t* d_blur = nullptr;
  uint32_t* d_cand = nullptr;
  uint32_t* d_scratch = nullptr;
  int32_t* d_cell_count = nullptr;
  uint32_t* d_sel = nullptr;
  int32_t* d_sel_count = nullptr;
  int32_t* d_cell_keep = nullptr;   // split selection: kept count / offset in the level list per (frame, cell), list length per (frame, level)
  int32_t* d_cell_off = nullptr;
  int32_t* d_lvl_m = nullptr;
  sd_keypoint* d_kps = nullptr;
  sd_keypoint* d_kps_un = nullptr;   // Frame::mvKeysUn (== d_kps when k1 == 0)
  bool have_dist = false;
  float dist_K[4] = {0, 0, 0, 0};    // fx, fy, cx, cy as CV_32F (Converter::toCvMat)
  float dist[5] = {0, 0, 0, 0, 0};   // k1, k2, p1, p2, k3
  uint8_t* d_desc = nullptr;
  int32_t* d_nout = nullptr;
  // hipGraph cache of the extraction pipeline (multi-stream fork/join captured once per argument set); opt-in with
  // option "extract.use_graph" -- see orb_launch_pipeline for the measurement that keeps direct launches the default
  struct GraphKey {   // everything a captured pipeline_body bakes in
    const void* imgs = nullptr;
    int n = 0, stride = 0, set = -1;
    size_t frame_stride = 0;
    bool dist = false;
    float distv[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};   // fx, fy, cx, cy, k1, k2, p1, p2, k3; zeros without distortion
    bool operator==(const GraphKey& o) const {
      return imgs == o.imgs && n == o.n && stride == o.stride && set == o.set && frame_stride == o.frame_stride && dist == o.dist &&
             memcmp(distv, o.distv, sizeof(distv)) == 0;
    }
  };
  struct GraphEntry {
    GraphKey key;
    hipGraphExec_t exec = nullptr;
  };
  GraphEntry graphs[4];
  int graph_next = 0;
  bool profiling = false;
  // ring of per-call stage events: the bench reads mean stage times over its whole timed region
  static const int kRing = 128;
  hipEvent_t ev[kRing][EV_STAGE_COUNT] = {};
  // one (start, stop) pair per k_fast_cells launch: the FAST stage is reported as the SUM of its launches' durations (the stream
  // waits for pyramid levels between them; EV_FAST_BEGIN .. EV_FAST_END would count those gaps).  Created when profiling is first switched on.
  static const int kFastPairs = SD_MAX_LEVELS + 1;
  hipEvent_t evf[kRing][2 * kFastPairs] = {};
  int evf_n[kRing] = {};
  bool evf_ready = false;
  int ev_calls = 0;   // calls recorded since profiling was (re-)enabled
};

// Keypoints a frame can hold: the sum of the per-level quotas (hp.plan.nsel is the same number, but only once a geometry is planned)
static inline int keypoint_capacity(const sd_orb* h) {
  int n = 0;
  for (int q : h->hp.quota) n += q;
  return n;
}

// Frame::mvKeysUn of the most recent extraction: the keypoints themselves where the camera has no distortion
static inline sd_keypoint* keys_un(const sd_orb* h) { return h->have_dist ? h->d_kps_un : h->d_kps; }

static inline void select_set(sd_orb* h, int sidx) {
  h->set = sidx;
  h->d_pyr = h->pyr_set[sidx];
  h->d_kps = h->kps_set[sidx];
  h->d_kps_un = h->kps_un_set[sidx];
  h->d_desc = h->desc_set[sidx];
  h->d_nout = h->nout_set[sidx];
}

// The cache key of an extraction of n frames at d_imgs into the handle's current output set
static inline sd_orb::GraphKey graph_key(const sd_orb* h, const void* d_imgs, int n, int stride, size_t frame_stride) {
  sd_orb::GraphKey k;
  k.imgs = d_imgs; k.n = n; k.stride = stride; k.set = h->set; k.frame_stride = frame_stride;
  k.dist = h->have_dist;
  if (k.dist) {
    memcpy(k.distv, h->dist_K, sizeof(h->dist_K));
    memcpy(k.distv + 4, h->dist, sizeof(h->dist));
  }
  return k;
}

// The untimed events that live as long as the handle, in creation order (ev_user_fence is created on first use)
template <class F>
static inline void for_each_event(sd_orb* h, F f) {
  for (hipEvent_t& e : h->ev_set_free) f(e);
  f(h->ev_extract_done);
  for (hipEvent_t& e : h->ev_level) f(e);
  f(h->ev_fast_done);
  f(h->ev_select_done);
  f(h->ev_body_start);
  f(h->ev_pyr_done);
  f(h->ev_blur_done);
}

// Device buffers sized by the planned geometry (freed and rebuilt when the frame size changes) / by the handle's capacity
static inline std::array<void**, 14> geom_buffers(sd_orb* h) {
  return {(void**)&h->d_cells, (void**)&h->d_tiles, (void**)&h->d_coef, (void**)&h->pyr_set[0], (void**)&h->pyr_set[1],
          (void**)&h->d_blur, (void**)&h->d_cand, (void**)&h->d_scratch, (void**)&h->d_cell_count, (void**)&h->d_sel,
          (void**)&h->d_sel_count, (void**)&h->d_cell_keep, (void**)&h->d_cell_off, (void**)&h->d_lvl_m};
}
static inline std::array<void**, 10> fixed_buffers(sd_orb* h) {
  return {(void**)&h->d_plan, (void**)&h->d_img, (void**)&h->kps_set[0], (void**)&h->kps_set[1], (void**)&h->kps_un_set[0],
          (void**)&h->kps_un_set[1], (void**)&h->desc_set[0], (void**)&h->desc_set[1], (void**)&h->nout_set[0], (void**)&h->nout_set[1]};
}

namespace sd {
// orb.hip: the kernels of one extraction of n frames at d_imgs into the next output set.  frames_ready: the frames are complete on
// the device (or ordered by sd_orb_stream_fence), not written by a copy queued on the extraction stream
int orb_launch_pipeline(sd_orb* h, const uint8_t* d_imgs, int n, int stride, size_t frame_stride, bool frames_ready);
void orb_drop_graphs(sd_orb* h);           // orb.hip
int orb_enable_double_buffer(sd_orb* h);   // orb_host.hip; idempotent
}
