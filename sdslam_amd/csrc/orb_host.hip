// Host layer of ORB extraction: the sd_orb handle (creation, geometry, output sets), the sd_orb_* C ABI around the launch pipeline
// of orb.hip (sd::orb_launch_pipeline), the downloads, debug read-outs and stage timers, and the library's small general entry
// points (sd_last_error, sd_version, sd_dev_* / sd_host_*, sd_hamming).  No kernel is defined or launched here.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "orb_internal.h"

using namespace sd;

static thread_local std::string g_err;
namespace sd {
void set_error(const std::string& msg) { g_err = msg; }
}

static const char* kStageNames[ST_COUNT] = {"pyramid", "fast_nms", "select", "blur", "orient_desc"};

// max(count, 1) * per elements of T
template <class T>
static int dev_alloc(T*& p, size_t count, size_t per = 1) {
  SD_HIP_CHECK(hipMalloc(&p, std::max<size_t>(count, 1) * per * sizeof(T)));
  return SD_OK;
}

template <class T>
static int upload_vec(T* dst, const std::vector<T>& v, hipStream_t stream) {
  if (!v.empty()) SD_HIP_CHECK(hipMemcpyAsync(dst, v.data(), v.size() * sizeof(T), hipMemcpyHostToDevice, stream));
  return SD_OK;
}

template <size_t N>
static void free_all(const std::array<void**, N>& ptrs) {
  for (void** p : ptrs) {
    if (*p) (void)hipFree(*p);
    *p = nullptr;
  }
}

static void free_geom(sd_orb* h) {
  free_all(geom_buffers(h));
  h->d_pyr = nullptr;
}

static int wait_trackers(sd_orb* h) {   // host-side: nothing may still read any output set
  for (int i = 0; i < 2; i++)
    if (h->set_busy[i]) {
      SD_HIP_CHECK(hipEventSynchronize(h->ev_set_free[i]));
      h->set_busy[i] = false;
    }
  return SD_OK;
}

// Padded pyramid of output set i, zeroed on the handle's stream
static int alloc_pyramid(sd_orb* h, int i, const OrbPlan& plan) {
  const size_t bytes = plan.pyr_frame_bytes * h->max_batch + 4096;
  SD_TRY(dev_alloc(h->pyr_set[i], bytes));
  SD_HIP_CHECK(hipMemsetAsync(h->pyr_set[i], 0, bytes, h->stream));
  return SD_OK;
}

// What a tracker reads of an extraction: keypoints, undistorted keypoints, descriptors, zeroed counts, and the pyramid if a
// geometry exists (build_geometry allocates it otherwise)
static int alloc_output_set(sd_orb* h, int i) {
  const size_t cap = std::max(keypoint_capacity(h), 1), B = h->max_batch;
  SD_TRY(dev_alloc(h->kps_set[i], cap * B));
  SD_TRY(dev_alloc(h->kps_un_set[i], cap * B));
  SD_TRY(dev_alloc(h->desc_set[i], cap * B * 32));
  SD_TRY(dev_alloc(h->nout_set[i], B));
  SD_HIP_CHECK(hipMemset(h->nout_set[i], 0, B * 4));
  if (h->have_geom) {
    SD_TRY(alloc_pyramid(h, i, h->hp.plan));
    SD_HIP_CHECK(hipStreamSynchronize(h->stream));
  }
  return SD_OK;
}

// Geometry (re)build.  Everything that can fail -- planning, allocation, upload -- works on a LOCAL plan and the handle is
// marked "no geometry" first, so a failure (a frame too small to plan, an allocation that does not fit) leaves a handle
// that rebuilds from scratch on its next call instead of one whose host plan no longer matches its device buffers.
static int build_geometry(sd_orb* h, const HostPlan& hp) {
  const size_t B = h->max_batch;
  const size_t pyr_bytes = hp.plan.pyr_frame_bytes * B + 4096;
  SD_TRY(dev_alloc(h->d_cells, hp.cells.size()));
  SD_TRY(dev_alloc(h->d_tiles, hp.blur_tiles.size()));
  SD_TRY(dev_alloc(h->d_coef, hp.coef.size()));
  for (int i = 0; i < h->nsets; i++) SD_TRY(alloc_pyramid(h, i, hp.plan));
  select_set(h, 0);
  SD_TRY(dev_alloc(h->d_blur, pyr_bytes));
  SD_TRY(dev_alloc(h->d_cand, hp.plan.cand_per_frame, B));
  SD_TRY(dev_alloc(h->d_scratch, hp.plan.cand_per_frame, B));
  SD_TRY(dev_alloc(h->d_cell_count, hp.plan.ncells, B));
  SD_TRY(dev_alloc(h->d_sel, hp.plan.nsel, B));
  SD_TRY(dev_alloc(h->d_sel_count, h->nlevels, B));
  SD_TRY(dev_alloc(h->d_cell_keep, hp.plan.ncells, B));
  SD_TRY(dev_alloc(h->d_cell_off, hp.plan.ncells, B));
  SD_TRY(dev_alloc(h->d_lvl_m, h->nlevels, B));
  SD_HIP_CHECK(hipMemsetAsync(h->d_blur, 0, pyr_bytes, h->stream));
  SD_TRY(upload_vec(h->d_cells, hp.cells, h->stream));
  SD_TRY(upload_vec(h->d_tiles, hp.blur_tiles, h->stream));
  SD_TRY(upload_vec(h->d_coef, hp.coef, h->stream));
  SD_HIP_CHECK(hipMemcpyAsync(h->d_plan, &hp.plan, sizeof(OrbPlan), hipMemcpyHostToDevice, h->stream));
  SD_HIP_CHECK(hipStreamSynchronize(h->stream));
  return SD_OK;
}

static int ensure_geometry(sd_orb* h, int w, int hgt) {
  if (h->have_geom && h->cur_w == w && h->cur_h == hgt) return SD_OK;
  SD_REQUIRE(w <= h->max_w && hgt <= h->max_h, SD_ERR_CAPACITY, "frame larger than the handle's max_w x max_h");
  const char* why = "";
  HostPlan np = h->hp;   // carries the size-independent tables (scale factors, quotas, umax, pattern)
  if (!plan_geometry(h->nfeatures, h->nlevels, h->thFAST, w, hgt, np, &why)) {
    set_error(std::string("unsupported geometry: ") + why);
    return SD_ERR_INVALID_ARG;   // the handle keeps its previous, still consistent geometry
  }
  SD_REQUIRE(np.max_cells_per_level <= SEL_MAX_CELLS && (size_t)np.plan.ncells * 16 <= 60 * 1024, SD_ERR_INVALID_ARG,
             "too many grid cells (k_select_quota keeps four ints per cell in LDS)");
  SD_HIP_CHECK(hipSetDevice(h->device));
  SD_HIP_CHECK(hipStreamSynchronize(h->stream));
  SD_TRY(wait_trackers(h));
  orb_drop_graphs(h);
  h->select_recorded = false;
  h->have_geom = false;
  h->cur_w = h->cur_h = 0;
  h->last_frames = 0;
  free_geom(h);
  const int rc = build_geometry(h, np);
  if (rc != SD_OK) {
    free_geom(h);   // partial allocations; have_geom stays false: the next call rebuilds everything
    return rc;
  }
  h->hp = std::move(np);
  h->have_geom = true;
  h->cur_w = w;
  h->cur_h = hgt;
  return SD_OK;
}

// Behind the checks of the two entry points.  frames_ready: the caller's frames are complete on the device (or ordered by
// sd_orb_stream_fence); the host-input entry point copies them on the extraction stream just before
static int extract_device(sd_orb* h, const uint8_t* d_imgs, int n_frames, int w, int hgt, int stride, size_t frame_stride, bool frames_ready) {
  SD_TRY(ensure_geometry(h, w, hgt));
  return orb_launch_pipeline(h, d_imgs, n_frames, stride, frame_stride, frames_ready);
}

static int check_frame_range(const sd_orb* h, int frame0, int n_frames) {
  SD_REQUIRE(frame0 >= 0 && n_frames >= 1 && frame0 + n_frames <= h->last_frames, SD_ERR_INVALID_ARG,
             "frame range outside the last batch");
  return SD_OK;
}

// First half of a download, behind check_frame_range: the keypoint counts of the frames (a host wait for the extraction), then
// -- unless nothing but the counts is wanted -- the caller's row capacity
static int download_counts(sd_orb* h, int frame0, int n_frames, int cap_per_frame, bool counts_only, int32_t* n_out) {
  SD_HIP_CHECK(hipSetDevice(h->device));
  SD_HIP_CHECK(hipMemcpyAsync(n_out, h->d_nout + frame0, (size_t)n_frames * 4, hipMemcpyDeviceToHost, h->stream));
  SD_HIP_CHECK(hipStreamSynchronize(h->stream));
  for (int f = 0; f < n_frames; f++)
    SD_REQUIRE(n_out[f] <= cap_per_frame || counts_only, SD_ERR_CAPACITY, "cap_per_frame smaller than keypoint count");
  return SD_OK;
}

// Second half: the first n[f] entries (elem bytes each) of every frame's device row into rows of cap_per_frame entries; queued only
static int download_rows(sd_orb* h, const void* d_src, size_t elem, void* out, int frame0, int n_frames, int cap_per_frame, const int32_t* n) {
  const size_t cap = std::max(h->hp.plan.nsel, 1);
  for (int f = 0; f < n_frames; f++)
    if (n[f] > 0)
      SD_HIP_CHECK(hipMemcpyAsync((uint8_t*)out + (size_t)f * cap_per_frame * elem, (const uint8_t*)d_src + (size_t)(frame0 + f) * cap * elem,
                                  (size_t)n[f] * elem, hipMemcpyDeviceToHost, h->stream));
  return SD_OK;
}

static int check_frame_level(const sd_orb* h, int frame, int level) {
  SD_REQUIRE(h && h->have_geom && level >= 0 && level < h->nlevels && frame >= 0 && frame < h->last_frames,
             SD_ERR_INVALID_ARG, "bad frame/level");
  return SD_OK;
}

static int copy_level(sd_orb* h, const uint8_t* base, int frame, int level, int padded, uint8_t* out, int out_stride) {
  SD_REQUIRE(out, SD_ERR_INVALID_ARG, "bad frame/level");
  SD_TRY(check_frame_level(h, frame, level));
  const LevelGeom& L = h->hp.plan.lv[level];
  SD_HIP_CHECK(hipSetDevice(h->device));
  const uint8_t* src = base + (size_t)frame * h->hp.plan.pyr_frame_bytes + L.off;
  int wc = L.w, hc = L.h;
  if (padded) {
    wc += 2 * SD_EDGE;
    hc += 2 * SD_EDGE;
  } else {
    src += (size_t)SD_EDGE * L.pstride + SD_EDGE;
  }
  SD_REQUIRE(out_stride >= wc, SD_ERR_INVALID_ARG, "out_stride too small");
  SD_HIP_CHECK(hipMemcpy2DAsync(out, out_stride, src, L.pstride, wc, hc, hipMemcpyDeviceToHost, h->stream));
  SD_HIP_CHECK(hipStreamSynchronize(h->stream));
  return SD_OK;
}

// Streams, fixed-size buffers, output set 0 and events of a new handle; the caller destroys the handle when a step fails
static int init_handle(sd_orb* h) {
  SD_HIP_CHECK(hipStreamCreateWithFlags(&h->own_stream, hipStreamNonBlocking));
  SD_TRY(dev_alloc(h->d_plan, 1));
  SD_TRY(dev_alloc(h->d_img, (size_t)h->max_w * h->max_h * h->max_batch));
  SD_TRY(alloc_output_set(h, 0));
  hipError_t e = hipSuccess;
  for_each_event(h, [&e](hipEvent_t& ev) {
    if (e == hipSuccess) e = hipEventCreateWithFlags(&ev, hipEventDisableTiming);
  });
  SD_HIP_CHECK(e);
  select_set(h, 0);
  for (auto& ring : h->ev)
    for (hipEvent_t& ev : ring) SD_HIP_CHECK(hipEventCreate(&ev));
  SD_HIP_CHECK(hipStreamCreateWithFlags(&h->aux_stream, hipStreamNonBlocking));
  SD_HIP_CHECK(hipStreamCreateWithFlags(&h->fast_stream, hipStreamNonBlocking));
  h->stream = h->own_stream;
  return SD_OK;
}

namespace sd {
// Second output set for a handle whose frames a tracker consumes on its own stream.
int orb_enable_double_buffer(sd_orb* h) {
  if (h->nsets == 2) return SD_OK;
  SD_HIP_CHECK(hipSetDevice(h->device));
  SD_HIP_CHECK(hipStreamSynchronize(h->stream));
  SD_TRY(alloc_output_set(h, 1));
  h->nsets = 2;
  return SD_OK;
}
}  // namespace sd

extern "C" {

const char* sd_last_error(void) { return g_err.c_str(); }
const char* sd_version(void) { return "sdslam_hip 0.1 (gfx950)"; }

int sd_device_count(void) {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

int sd_orb_create(int nfeatures, float scale_factor, int nlevels, int th_fast, int max_w, int max_h, int max_batch,
                  int device, sd_orb** out) {
  SD_REQUIRE(out != nullptr, SD_ERR_INVALID_ARG, "out is NULL");
  *out = nullptr;
  SD_REQUIRE(nfeatures > 0 && nlevels >= 1 && nlevels <= SD_MAX_LEVELS && scale_factor > 1.0f, SD_ERR_INVALID_ARG,
             "bad extractor parameters");
  SD_REQUIRE(max_w >= 1 && max_h >= 1 && max_w <= SD_MAX_DIM && max_h <= SD_MAX_DIM && max_batch >= 1, SD_ERR_INVALID_ARG,
             "bad capacity parameters");
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0) {
    set_error("no HIP device visible: the HIP path is the only implementation (no CPU fallback)");
    return SD_ERR_NO_DEVICE;
  }
  SD_REQUIRE(device >= 0 && device < ndev, SD_ERR_INVALID_ARG, "device index out of range");
  SD_HIP_CHECK(hipSetDevice(device));
  sd_orb* h = new sd_orb();
  h->nfeatures = nfeatures;
  h->scaleFactor = scale_factor;
  h->nlevels = nlevels;
  h->thFAST = th_fast;
  h->max_w = max_w;
  h->max_h = max_h;
  h->max_batch = max_batch;
  h->device = device;
  plan_tables(nfeatures, scale_factor, nlevels, h->hp);
  const int rc = init_handle(h);
  if (rc != SD_OK) {
    sd_orb_destroy(h);
    return rc;
  }
  *out = h;
  return SD_OK;
}

void sd_orb_destroy(sd_orb* h) {
  if (!h) return;
  (void)hipSetDevice(h->device);
  if (h->stream) (void)hipStreamSynchronize(h->stream);
  (void)wait_trackers(h);
  orb_drop_graphs(h);
  free_geom(h);
  free_all(fixed_buffers(h));
  for (hipStream_t st : {h->aux_stream, h->fast_stream})
    if (st) { (void)hipStreamSynchronize(st); (void)hipStreamDestroy(st); }
  auto destroy = [](hipEvent_t& e) {
    if (e) (void)hipEventDestroy(e);
  };
  for_each_event(h, destroy);
  for (hipEvent_t& e : h->ev_user_fence) destroy(e);
  for (int r = 0; r < sd_orb::kRing; r++) {
    for (hipEvent_t& e : h->ev[r]) destroy(e);
    for (hipEvent_t& e : h->evf[r]) destroy(e);
  }
  if (h->own_stream) (void)hipStreamDestroy(h->own_stream);
  delete h;
}

int sd_orb_levels(const sd_orb* h) { return h ? h->nlevels : 0; }

// Host-only (no GPU needed): geometry the extractor would use for a w x h frame.
int sd_orb_plan_info(int nfeatures, float scale_factor, int nlevels, int th_fast, int w, int hgt, int32_t* level_info,
                     int32_t* cell_zones, int cell_cap, int32_t* n_cells, uint64_t* bytes_per_frame) {
  SD_REQUIRE(level_info && n_cells, SD_ERR_INVALID_ARG, "NULL argument");
  SD_REQUIRE(nfeatures > 0 && nlevels >= 1 && nlevels <= SD_MAX_LEVELS && scale_factor > 1.0f, SD_ERR_INVALID_ARG,
             "bad extractor parameters");
  HostPlan hp;
  plan_tables(nfeatures, scale_factor, nlevels, hp);
  const char* why = "";
  if (!plan_geometry(nfeatures, nlevels, th_fast, w, hgt, hp, &why)) {
    set_error(std::string("unsupported geometry: ") + why);
    return SD_ERR_INVALID_ARG;
  }
  for (int l = 0; l < nlevels; l++) {
    const LevelGeom& L = hp.plan.lv[l];
    int32_t* o = level_info + 8 * l;
    o[0] = L.w; o[1] = L.h; o[2] = L.quota; o[3] = L.cols; o[4] = L.rows; o[5] = L.cellW; o[6] = L.cellH; o[7] = L.nfeaturesCell;
  }
  *n_cells = hp.plan.ncells;
  if (cell_zones) {
    SD_REQUIRE(cell_cap >= hp.plan.ncells, SD_ERR_CAPACITY, "cell_cap too small");
    for (int c = 0; c < hp.plan.ncells; c++) {
      const CellGeom& C = hp.cells[c];
      int32_t* o = cell_zones + 6 * c;
      o[0] = C.level; o[1] = C.zx0; o[2] = C.zy0; o[3] = C.zw; o[4] = C.zh; o[5] = C.evaluated;
    }
  }
  if (bytes_per_frame) *bytes_per_frame = hp.plan.pyr_frame_bytes * 2 + (uint64_t)hp.plan.cand_per_frame * 8;
  return SD_OK;
}

// Host-only: the row-block table k_pyr_rows would walk on `level` of that geometry (under the current "extract.pyr_rows")
int sd_orb_plan_row_blocks(int nfeatures, float scale_factor, int nlevels, int th_fast, int w, int hgt, int level, int32_t* blocks,
                           int block_cap, int32_t* n_blocks) {
  SD_REQUIRE(n_blocks, SD_ERR_INVALID_ARG, "NULL argument");
  SD_REQUIRE(nfeatures > 0 && nlevels >= 1 && nlevels <= SD_MAX_LEVELS && scale_factor > 1.0f && level >= 0 && level < nlevels,
             SD_ERR_INVALID_ARG, "bad extractor parameters");
  HostPlan hp;
  plan_tables(nfeatures, scale_factor, nlevels, hp);
  const char* why = "";
  if (!plan_geometry(nfeatures, nlevels, th_fast, w, hgt, hp, &why)) {
    set_error(std::string("unsupported geometry: ") + why);
    return SD_ERR_INVALID_ARG;
  }
  const LevelGeom& L = hp.plan.lv[level];
  *n_blocks = L.nblk;
  if (blocks) {
    SD_REQUIRE(block_cap >= L.nblk, SD_ERR_CAPACITY, "block_cap too small");
    for (int b = 0; b < L.nblk; b++) {
      PyrRowBlock k;
      memcpy(&k, hp.coef.data() + L.cb + (size_t)b * (sizeof(PyrRowBlock) / 4), sizeof(k));
      int32_t* o = blocks + 4 * b;
      o[0] = k.y0; o[1] = k.n_border & 0xff; o[2] = k.sy0; o[3] = k.n_border >> 8;
    }
  }
  return SD_OK;
}

int sd_orb_scale_tables(const sd_orb* h, float* sf, float* inv_sf, float* sigma2, float* inv_sigma2) {
  SD_REQUIRE(h, SD_ERR_INVALID_ARG, "handle is NULL");
  for (int i = 0; i < h->nlevels; i++) {
    if (sf) sf[i] = h->hp.sf[i];
    if (inv_sf) inv_sf[i] = h->hp.inv_sf[i];
    if (sigma2) sigma2[i] = h->hp.sigma2[i];
    if (inv_sigma2) inv_sigma2[i] = h->hp.inv_sigma2[i];
  }
  return SD_OK;
}

int sd_orb_features_per_level(const sd_orb* h, int32_t* quota) {
  SD_REQUIRE(h && quota, SD_ERR_INVALID_ARG, "NULL argument");
  for (int i = 0; i < h->nlevels; i++) quota[i] = h->hp.quota[i];
  return SD_OK;
}

int sd_orb_extract_batch_device(sd_orb* h, const void* d_imgs, int n_frames, int w, int hgt, int stride,
                                size_t frame_stride) {
  SD_REQUIRE(h && d_imgs, SD_ERR_INVALID_ARG, "NULL argument");
  SD_REQUIRE(n_frames >= 1 && n_frames <= h->max_batch, SD_ERR_CAPACITY, "n_frames exceeds max_batch");
  SD_REQUIRE(w >= 1 && hgt >= 1 && stride >= w && frame_stride >= (size_t)stride * (hgt - 1) + w, SD_ERR_INVALID_ARG,
             "bad image shape/stride");
  SD_HIP_CHECK(hipSetDevice(h->device));
  return extract_device(h, (const uint8_t*)d_imgs, n_frames, w, hgt, stride, frame_stride, true);
}

int sd_orb_download(sd_orb* h, int frame0, int n_frames, sd_keypoint* kps_out, uint8_t* desc_out, int cap_per_frame,
                    int32_t* n_out) {
  SD_REQUIRE(h && n_out, SD_ERR_INVALID_ARG, "NULL argument");
  SD_TRY(check_frame_range(h, frame0, n_frames));
  SD_TRY(download_counts(h, frame0, n_frames, cap_per_frame, !kps_out && !desc_out, n_out));
  const int cap = std::max(h->hp.plan.nsel, 1);
  if (cap_per_frame == cap && n_frames > 8) {
    // same row pitch on both sides: two bulk copies instead of 2 x n_frames small ones (entries beyond n_out[f] are
    // whatever the device rows hold; callers must not read them)
    if (kps_out)
      SD_HIP_CHECK(hipMemcpyAsync(kps_out, h->d_kps + (size_t)frame0 * cap, (size_t)n_frames * cap * sizeof(sd_keypoint),
                                  hipMemcpyDeviceToHost, h->stream));
    if (desc_out)
      SD_HIP_CHECK(hipMemcpyAsync(desc_out, h->d_desc + (size_t)frame0 * cap * 32, (size_t)n_frames * cap * 32, hipMemcpyDeviceToHost,
                                  h->stream));
  } else {
    if (kps_out) SD_TRY(download_rows(h, h->d_kps, sizeof(sd_keypoint), kps_out, frame0, n_frames, cap_per_frame, n_out));
    if (desc_out) SD_TRY(download_rows(h, h->d_desc, 32, desc_out, frame0, n_frames, cap_per_frame, n_out));
  }
  SD_HIP_CHECK(hipStreamSynchronize(h->stream));
  return SD_OK;
}

int sd_orb_extract_batch(sd_orb* h, const uint8_t* imgs, int n_frames, int w, int hgt, int stride, size_t frame_stride,
                         sd_keypoint* kps_out, uint8_t* desc_out, int cap_per_frame, int32_t* n_out) {
  SD_REQUIRE(h && n_out, SD_ERR_INVALID_ARG, "NULL argument");
  if (w <= 0 || hgt <= 0 || !imgs) {   // _image.empty(): return silently (src/ORBextractor.cc:622-623)
    for (int f = 0; f < n_frames; f++) n_out[f] = 0;
    return SD_OK;
  }
  SD_REQUIRE(n_frames >= 1 && n_frames <= h->max_batch, SD_ERR_CAPACITY, "n_frames exceeds max_batch");
  SD_REQUIRE(w <= h->max_w && hgt <= h->max_h, SD_ERR_CAPACITY, "frame larger than the handle's max_w x max_h");
  SD_REQUIRE(stride >= w, SD_ERR_INVALID_ARG, "stride < width");
  SD_HIP_CHECK(hipSetDevice(h->device));
  // pack rows tightly into the staging buffer (one copy when the frames already are tightly packed)
  if (stride == w && (n_frames == 1 || frame_stride == (size_t)w * hgt)) {
    SD_HIP_CHECK(hipMemcpyAsync(h->d_img, imgs, (size_t)n_frames * w * hgt, hipMemcpyHostToDevice, h->stream));
  } else {
    for (int f = 0; f < n_frames; f++)
      SD_HIP_CHECK(hipMemcpy2DAsync(h->d_img + (size_t)f * w * hgt, w, imgs + (size_t)f * frame_stride, stride, w,
                                    (size_t)hgt, hipMemcpyHostToDevice, h->stream));
  }
  // (not frames_ready: the frames reach d_img by the copy queued on the extraction stream just above)
  SD_TRY(extract_device(h, h->d_img, n_frames, w, hgt, w, (size_t)w * hgt, false));
  return sd_orb_download(h, 0, n_frames, kps_out, desc_out, cap_per_frame, n_out);
}

int sd_orb_extract(sd_orb* h, const uint8_t* img, int w, int hgt, int stride, sd_keypoint* kps_out, uint8_t* desc_out,
                   int cap, int* n_out) {
  SD_REQUIRE(n_out, SD_ERR_INVALID_ARG, "n_out is NULL");
  int32_t n = 0;
  int rc = sd_orb_extract_batch(h, img, 1, w, hgt, stride, (size_t)stride * (hgt > 0 ? hgt : 0), kps_out, desc_out, cap, &n);
  *n_out = n;
  return rc;
}

int sd_orb_set_distortion(sd_orb* h, float fx, float fy, float cx, float cy, float k1, float k2, float p1, float p2, float k3) {
  SD_REQUIRE(h, SD_ERR_INVALID_ARG, "handle is NULL");
  SD_REQUIRE(fx > 0 && fy > 0, SD_ERR_INVALID_ARG, "bad camera matrix");
  h->dist_K[0] = fx; h->dist_K[1] = fy; h->dist_K[2] = cx; h->dist_K[3] = cy;
  h->dist[0] = k1; h->dist[1] = k2; h->dist[2] = p1; h->dist[3] = p2; h->dist[4] = k3;
  h->have_dist = (k1 != 0.0f);   // mDistCoef.at<float>(0) == 0.0 -> mvKeysUn = mvKeys
  return SD_OK;
}

int sd_orb_download_undistorted(sd_orb* h, int frame0, int n_frames, sd_keypoint* kps_un_out, int cap_per_frame) {
  SD_REQUIRE(h && kps_un_out, SD_ERR_INVALID_ARG, "NULL argument");
  SD_TRY(check_frame_range(h, frame0, n_frames));
  std::vector<int32_t> n(n_frames);
  SD_TRY(download_counts(h, frame0, n_frames, cap_per_frame, false, n.data()));
  SD_TRY(download_rows(h, keys_un(h), sizeof(sd_keypoint), kps_un_out, frame0, n_frames, cap_per_frame, n.data()));
  SD_HIP_CHECK(hipStreamSynchronize(h->stream));
  return SD_OK;
}

int sd_orb_level_info(const sd_orb* h, int level, int* w, int* hgt) {
  SD_REQUIRE(h && h->have_geom && level >= 0 && level < h->nlevels, SD_ERR_INVALID_ARG, "no geometry / bad level");
  if (w) *w = h->hp.plan.lv[level].w;
  if (hgt) *hgt = h->hp.plan.lv[level].h;
  return SD_OK;
}

int sd_orb_level_copy(sd_orb* h, int frame, int level, int padded, uint8_t* out, int out_stride) {
  SD_REQUIRE(h, SD_ERR_INVALID_ARG, "handle is NULL");
  return copy_level(h, h->d_pyr, frame, level, padded, out, out_stride);
}

int sd_orb_debug_blurred(sd_orb* h, int frame, int level, uint8_t* out, int out_stride) {
  SD_REQUIRE(h, SD_ERR_INVALID_ARG, "handle is NULL");
  return copy_level(h, h->d_blur + SD_BLUR_SHIFT, frame, level, 0, out, out_stride);
}

int sd_orb_debug_cell_counts(sd_orb* h, int frame, int level, int32_t* out, int cap, int* n_cells) {
  SD_REQUIRE(out && n_cells, SD_ERR_INVALID_ARG, "bad frame/level");
  SD_TRY(check_frame_level(h, frame, level));
  const LevelGeom& L = h->hp.plan.lv[level];
  *n_cells = L.ncells;
  SD_REQUIRE(cap >= L.ncells, SD_ERR_CAPACITY, "cap too small");
  if (L.ncells == 0) return SD_OK;
  SD_HIP_CHECK(hipSetDevice(h->device));
  SD_HIP_CHECK(hipMemcpyAsync(out, h->d_cell_count + (size_t)frame * h->hp.plan.ncells + L.cell0, (size_t)L.ncells * 4,
                              hipMemcpyDeviceToHost, h->stream));
  SD_HIP_CHECK(hipStreamSynchronize(h->stream));
  return SD_OK;
}

int sd_orb_debug_level_keys(sd_orb* h, int frame, int level, uint32_t* keys_out, int cap, int* n) {
  SD_REQUIRE(keys_out && n, SD_ERR_INVALID_ARG, "bad frame/level");
  SD_TRY(check_frame_level(h, frame, level));
  const LevelGeom& L = h->hp.plan.lv[level];
  SD_HIP_CHECK(hipSetDevice(h->device));
  int32_t cnt = 0;
  SD_HIP_CHECK(hipMemcpyAsync(&cnt, h->d_sel_count + (size_t)frame * h->nlevels + level, 4, hipMemcpyDeviceToHost, h->stream));
  SD_HIP_CHECK(hipStreamSynchronize(h->stream));
  *n = cnt;
  SD_REQUIRE(cap >= cnt, SD_ERR_CAPACITY, "cap too small");
  if (cnt > 0) {
    SD_HIP_CHECK(hipMemcpyAsync(keys_out, h->d_sel + (size_t)frame * h->hp.plan.nsel + L.sel_off, (size_t)cnt * 4,
                                hipMemcpyDeviceToHost, h->stream));
    SD_HIP_CHECK(hipStreamSynchronize(h->stream));
  }
  return SD_OK;
}

// Caller-made keypoints and descriptors in place of an extraction's (the hand-worked matcher cases of tests/match_cases.py).  What
// orb_launch_pipeline does around its kernels happens around the copies, except that the output set stays the current one: wait
// for a tracker that still reads it, record the end, count an extraction.
int sd_debug_orb_set_keypoints(sd_orb* h, int frame0, int n_frames, const int32_t* n, const sd_keypoint* kps, const uint8_t* desc,
                               int cap) {
  SD_REQUIRE(h && n && kps && desc, SD_ERR_INVALID_ARG, "NULL argument");
  SD_REQUIRE(frame0 >= 0 && n_frames >= 1 && frame0 + n_frames <= h->max_batch, SD_ERR_CAPACITY, "frame range exceeds max_batch");
  SD_REQUIRE(h->have_geom, SD_ERR_INVALID_ARG, "no extraction has run on this handle (the output set has no geometry yet)");
  SD_REQUIRE(!h->have_dist, SD_ERR_INVALID_ARG, "a distortion is set: the undistorted keypoints would be a second array");
  const int kcap = h->hp.plan.nsel;
  for (int f = 0; f < n_frames; f++)
    SD_REQUIRE(n[f] >= 0 && n[f] <= kcap && n[f] <= cap, SD_ERR_CAPACITY, "keypoint count exceeds the keypoint capacity");
  SD_HIP_CHECK(hipSetDevice(h->device));
  hipStream_t s = h->stream;
  if (h->set_busy[h->set]) {
    SD_HIP_CHECK(hipStreamWaitEvent(s, h->ev_set_free[h->set], 0));
    h->set_busy[h->set] = false;
  }
  for (int f = 0; f < n_frames; f++) {
    if (n[f] == 0) continue;
    const size_t row = (size_t)(frame0 + f) * kcap;
    SD_HIP_CHECK(hipMemcpyAsync(h->d_kps + row, kps + (size_t)f * cap, (size_t)n[f] * sizeof(sd_keypoint), hipMemcpyHostToDevice, s));
    SD_HIP_CHECK(hipMemcpyAsync(h->d_desc + row * 32, desc + (size_t)f * cap * 32, (size_t)n[f] * 32, hipMemcpyHostToDevice, s));
  }
  SD_HIP_CHECK(hipMemcpyAsync(h->d_nout + frame0, n, (size_t)n_frames * 4, hipMemcpyHostToDevice, s));
  SD_HIP_CHECK(hipEventRecord(h->ev_extract_done, s));
  h->extract_recorded = true;
  h->extract_serial++;
  h->last_frames = std::max(h->last_frames, frame0 + n_frames);
  SD_HIP_CHECK(hipStreamSynchronize(s));   // the caller's arrays are its own again
  return SD_OK;
}

int sd_orb_set_stream(sd_orb* h, void* hip_stream) {
  SD_REQUIRE(h, SD_ERR_INVALID_ARG, "handle is NULL");
  SD_HIP_CHECK(hipSetDevice(h->device));
  SD_HIP_CHECK(hipStreamSynchronize(h->stream));
  h->stream = hip_stream ? (hipStream_t)hip_stream : h->own_stream;
  return SD_OK;
}

// Ordering against a caller's HIP stream (an upload stream that fills the frames of the next batch while this one is being
// processed).  direction 0: `hip_stream` waits for everything queued on the extraction stream so far (the frames of the
// extractions queued so far have been consumed when it proceeds); 1: the extraction stream and the FAST and auxiliary
// streams, on which an early level-0 FAST / resize chain of a later extraction reads the frames (pipeline_body), wait for
// everything queued on `hip_stream` so far.  A wait takes the event's state at the time it is queued, so every fence
// holds, not only the last one.
int sd_orb_stream_fence(sd_orb* h, void* hip_stream, int direction) {
  SD_REQUIRE(h && (direction == 0 || direction == 1), SD_ERR_INVALID_ARG, "bad arguments");
  SD_HIP_CHECK(hipSetDevice(h->device));
  hipStream_t ext = (hipStream_t)hip_stream;
  for (int i = 0; i < 2; i++)
    if (!h->ev_user_fence[i]) SD_HIP_CHECK(hipEventCreateWithFlags(&h->ev_user_fence[i], hipEventDisableTiming));
  if (direction == 0) {
    SD_HIP_CHECK(hipEventRecord(h->ev_user_fence[0], h->stream));
    SD_HIP_CHECK(hipStreamWaitEvent(ext, h->ev_user_fence[0], 0));
  } else {
    SD_HIP_CHECK(hipEventRecord(h->ev_user_fence[1], ext));
    SD_HIP_CHECK(hipStreamWaitEvent(h->stream, h->ev_user_fence[1], 0));
    SD_HIP_CHECK(hipStreamWaitEvent(h->fast_stream, h->ev_user_fence[1], 0));
    SD_HIP_CHECK(hipStreamWaitEvent(h->aux_stream, h->ev_user_fence[1], 0));
  }
  return SD_OK;
}

int sd_orb_sync(sd_orb* h) {
  SD_REQUIRE(h, SD_ERR_INVALID_ARG, "handle is NULL");
  SD_HIP_CHECK(hipSetDevice(h->device));
  SD_HIP_CHECK(hipStreamSynchronize(h->aux_stream));
  SD_HIP_CHECK(hipStreamSynchronize(h->stream));
  return SD_OK;
}

int sd_orb_set_profiling(sd_orb* h, int on) {
  SD_REQUIRE(h, SD_ERR_INVALID_ARG, "handle is NULL");
  if (on && !h->evf_ready) {
    SD_HIP_CHECK(hipSetDevice(h->device));
    for (int r = 0; r < sd_orb::kRing; r++)
      for (int i = 0; i < 2 * sd_orb::kFastPairs; i++) SD_HIP_CHECK(hipEventCreate(&h->evf[r][i]));
    h->evf_ready = true;
  }
  h->profiling = on != 0;
  h->ev_calls = 0;
  return SD_OK;
}

int sd_orb_num_stages(void) { return ST_COUNT; }
const char* sd_orb_stage_name(int stage) { return (stage >= 0 && stage < ST_COUNT) ? kStageNames[stage] : ""; }

int sd_orb_stage_ms(sd_orb* h, float* ms_out, int cap) {
  SD_REQUIRE(h && ms_out && cap >= ST_COUNT, SD_ERR_INVALID_ARG, "bad arguments");
  SD_REQUIRE(h->profiling && h->ev_calls > 0, SD_ERR_INVALID_ARG, "profiling is off or no call recorded");
  SD_HIP_CHECK(hipSetDevice(h->device));
  SD_HIP_CHECK(hipStreamSynchronize(h->stream));
  const int n = std::min(h->ev_calls, (int)sd_orb::kRing);
  for (int i = 0; i < ST_COUNT; i++) ms_out[i] = 0.f;
  static const StageEvent kBegin[ST_COUNT] = {EV_PYR_BEGIN, EV_FAST_BEGIN, EV_SELECT_BEGIN, EV_BLUR_BEGIN, EV_DESC_BEGIN};
  static const StageEvent kEnd[ST_COUNT] = {EV_PYR_END, EV_FAST_END, EV_SELECT_END, EV_BLUR_END, EV_DESC_END};
  SD_HIP_CHECK(hipStreamSynchronize(h->aux_stream));
  SD_HIP_CHECK(hipStreamSynchronize(h->fast_stream));
  for (int r = 0; r < n; r++) {
    const int slot = (h->ev_calls - 1 - r) % sd_orb::kRing;
    for (int i = 0; i < ST_COUNT; i++) {
      float ms = 0;
      if (i == ST_FAST && h->evf_n[slot] > 0) {   // sum of the k_fast_cells launches (what a kernel trace of the same run adds up to)
        for (int k = 0; k < h->evf_n[slot]; k++) {
          float one = 0;
          SD_HIP_CHECK(hipEventElapsedTime(&one, h->evf[slot][2 * k], h->evf[slot][2 * k + 1]));
          ms += one;
        }
      } else {
        SD_HIP_CHECK(hipEventElapsedTime(&ms, h->ev[slot][kBegin[i]], h->ev[slot][kEnd[i]]));
      }
      ms_out[i] += ms / n;
    }
  }
  return SD_OK;
}

int sd_orb_stage_bytes(const sd_orb* h, double* bytes_out, int cap) {
  SD_REQUIRE(h && bytes_out && cap >= ST_COUNT && h->have_geom, SD_ERR_INVALID_ARG, "bad arguments / no geometry yet");
  for (int i = 0; i < ST_COUNT; i++) bytes_out[i] = h->hp.stage_bytes[i];
  return SD_OK;
}

int sd_dev_alloc(size_t bytes, void** out) {
  SD_REQUIRE(out, SD_ERR_INVALID_ARG, "out is NULL");
  SD_HIP_CHECK(hipMalloc(out, bytes));
  return SD_OK;
}
int sd_dev_free(void* p) {
  SD_HIP_CHECK(hipFree(p));
  return SD_OK;
}
// Page-locked host memory for frames / results: with it the host-buffer entry points copy at the PCIe rate
// (pageable buffers go through the driver's staging copies, measured 6 GB/s on the test box).
int sd_host_alloc(size_t bytes, void** out) {
  SD_REQUIRE(out, SD_ERR_INVALID_ARG, "out is NULL");
  SD_HIP_CHECK(hipHostMalloc(out, bytes, hipHostMallocDefault));
  return SD_OK;
}
int sd_host_free(void* p) {
  SD_HIP_CHECK(hipHostFree(p));
  return SD_OK;
}
int sd_dev_upload(void* dst, const void* src, size_t bytes) {
  SD_HIP_CHECK(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
  return SD_OK;
}
int sd_dev_download(void* dst, const void* src, size_t bytes) {
  SD_HIP_CHECK(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
  return SD_OK;
}

// ORBmatcher::DescriptorDistance (src/ORBmatcher.cc:1459-1473): 256-bit Hamming distance
int sd_hamming(const uint8_t* a32, const uint8_t* b32) {
  int dist = 0;
  for (int i = 0; i < 4; i++) {
    uint64_t x, y;
    memcpy(&x, a32 + 8 * i, 8);
    memcpy(&y, b32 + 8 * i, 8);
    dist += __builtin_popcountll(x ^ y);
  }
  return dist;
}

}  // extern "C"
