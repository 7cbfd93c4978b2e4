// MapPoint::ComputeDistinctiveDescriptors and MapPoint::UpdateNormalAndDepth on MI355X, for a list of map points at once
//   ComputeDistinctiveDescriptors()     reference src/MapPoint.cc:225-284
//   UpdateNormalAndDepth()              src/MapPoint.cc:304-343
// callers LocalMapping::SearchInNeighbors (src/LocalMapping.cc:478-488), ::CreateNewMapPoints' recent points (:140-147),
// LoopClosing::SearchAndFuse (src/LoopClosing.cc:457-484) and Tracking::CreateNewKeyFrame (src/Tracking.cc:874-875).
//
// Keyframes are frames of the extractors: obs_frame >= 0 is a frame of `ref` (pose Tref), -1 the current keyframe (the broadcast
// frame of `cur`, or frame 0 without a broadcast; pose Tcur of slot 0), -2 a keyframe that is not resident.  The observations of
// point p are the entries obs_off[p] .. obs_off[p + 1] - 1, IN THE CALLER'S ORDER: the reference iterates a std::map keyed by
// pointer, whose order is nobody's to reproduce, and the order decides two things -- the least median is taken with a strict `<`
// (the first row wins a tie) and the normal is summed one term after the other.  The result is the reference's loops run over
// the list as given.
//
// k_refresh_points: one wave per point, REFRESH_WAVES points per workgroup (LDS layout: track_refresh_lds.h).
//   1. status.  point bad or no observations -> SKIPPED (both functions return early); more than SD_REFRESH_MAX_OBS -> TOO_MANY;
//      an observation with frame -2 -> NOT_RESIDENT; a frame or keypoint index that names nothing, or a ref_obs outside the list
//      -> BAD_INDEX, and nothing is read through it.  None of these writes anything but the status.
//   2. normal and depth (every observation, bad keyframes included, as :323-329): lane l takes observations l, l + 64, ...:
//      d = Xw - Ow, len = sqrt((d.x^2 + d.y^2) + d.z^2), t = d / len per component, all double, every operation rounded on its
//      own (no contraction).  The terms go to LDS; lanes 0..2 sum one component each IN LIST ORDER from 0.0 and divide by (double)n.
//      Lane 3: dist = (float)|Xw - Ow(ref_obs)|, mfMaxDistance = dist * sf[octave of the ref observation's undistorted keypoint],
//      mfMinDistance = mfMaxDistance / sf[nlevels - 1], float.  Ow comes from k_refresh_centres (camera_centre of track_internal.h).
//   3. descriptor (observations of keyframes that are not bad, :246): their descriptors are compacted in order into LDS, with the
//      position each came from.  N = their number; none -> no descriptor (:250).  Lane i owns row i (then i + 64, ...): its own
//      descriptor in 8 VGPRs, the distance to descriptor j = sum of __popc over the 8 xor-ed dwords (sd_hamming), j a broadcast
//      read.  The row's median is the element of rank (N - 1) / 2, diagonal 0 included: the least v with #{d <= v} >= rank + 1.
//      A row is NOT kept (at the cap a wave's rows are 256 x 256 nine-bit values, 128 KB as uint16_t; a byte cannot hold the 256
//      of complementary descriptors): it is walked twice, with 16 and 15 counters in registers (constant indexing, unrolled) --
//      #{d <= 16 k + 15} picks the bucket of 16 values, #{d <= 16 b + m} the value in it; bucket 16 is the value 256.
//      Winner: wave minimum of median << 9 | row, i.e. least median, first row on ties.
// Stores are plain vector stores.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <string>
#include <vector>

#include "track_handle.h"
#include "track_match_dev.h"
#include "track_refresh_lds.h"

static_assert(REFRESH_CAP == SD_REFRESH_MAX_OBS, "the LDS layout is sized for the ABI's capacity");

namespace sd {

struct RefreshArgs {
  // the observation lists (CSR)
  const int32_t* off;        // [n_points + 1]
  const int32_t* ref_obs;    // [n_points]
  const uint8_t* point_bad;  // [n_points] or NULL
  const int32_t* frame;      // [n_obs]
  const int32_t* kp;         // [n_obs]
  const uint8_t* kf_bad;     // [n_obs] or NULL
  int n_points, n_obs;
  // the keyframes: rows of `cap` entries per frame
  const sd_keypoint* ref_kps;   // mvKeysUn
  const uint8_t* ref_desc;
  const int32_t* ref_nkp;
  int ref_cap, n_ref;        // frames 0 .. n_ref - 1 exist
  const sd_keypoint* cur_kps;
  const uint8_t* cur_desc;
  const int32_t* cur_nkp;
  int cur_cap, cur_frame;    // the frame observations with -1 name; -1: none
  const double* centre;      // [n_ref + 1][3]: Ow of the ref frames, then of the current keyframe
  const double* Xw;          // [n_points][3]
  const float* sf;           // [nlevels] mvScaleFactors
  int nlevels;
  // results
  uint8_t* status;
  int32_t* best_obs;
  int32_t* best_median;
  uint8_t* desc;
  double* normal;
  float* max_dist;
  float* min_dist;
  // write-through into a local-map row (NULL: none)
  uint8_t* lm_desc;
  double* lm_normal;
  float* lm_min;
  float* lm_max;
  float* lm_mfmax;
};

// Ow of every keyframe an observation can name: thread f < n_ref from Tref[f], thread n_ref from Tcur[0]
__global__ void k_refresh_centres(const double* __restrict__ Tref, const double* __restrict__ Tcur, int n_ref, double* __restrict__ centre) {
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f > n_ref) return;
  const double* T = f < n_ref ? Tref + (size_t)f * 16 : Tcur;
  for (int r = 0; r < 3; r++) centre[(size_t)f * 3 + r] = camera_centre(T, r);
}

// Where observation (fr, k) lives: 0 and the keypoint's row `e` in its extractor / its centre, or the status bit that says why not
struct ObsAt {
  const sd_keypoint* kp;
  const uint8_t* desc;
  const double* centre;
};
__device__ __forceinline__ int locate_obs(const RefreshArgs& a, int fr, int k, ObsAt* at) {
  if (fr == -2) return SD_REFRESH_NOT_RESIDENT;
  const bool cur = fr == -1;
  if (fr < -2 || fr >= a.n_ref || (cur && a.cur_frame < 0)) return SD_REFRESH_BAD_INDEX;
  const int f = cur ? a.cur_frame : fr, cap = cur ? a.cur_cap : a.ref_cap;
  const int nk = min((cur ? a.cur_nkp : a.ref_nkp)[f], cap);
  if (k < 0 || k >= nk) return SD_REFRESH_BAD_INDEX;
  const size_t e = (size_t)f * cap + k;
  at->kp = (cur ? a.cur_kps : a.ref_kps) + e;
  at->desc = (cur ? a.cur_desc : a.ref_desc) + e * 32;
  at->centre = a.centre + (size_t)(cur ? a.n_ref : fr) * 3;
  return 0;
}

// Xw - Ow and its length
__device__ __forceinline__ double view_vector(const double* __restrict__ X, const double* __restrict__ Ow, double (&d)[3]) {
  for (int k = 0; k < 3; k++) d[k] = __dsub_rn(X[k], Ow[k]);
  return __dsqrt_rn(dot3(d[0], d[1], d[2], d[0], d[1], d[2]));
}

// Hamming distance of this lane's descriptor to compacted descriptor j (a broadcast read of its 8 words)
__device__ __forceinline__ int row_distance(const uint32_t (&own)[8], const uint32_t* s_desc, int j) {
  int d = 0;
#pragma unroll
  for (int w = 0; w < 8; w++) d += __popc(own[w] ^ s_desc[LdsRefreshWave::desc_word(w, j)]);
  return d;
}

// The element of rank `rank` of row `own` against the N compacted descriptors (header, step 3)
__device__ __forceinline__ int row_median(const uint32_t (&own)[8], const uint32_t* s_desc, int N, int rank) {
  const int need = rank + 1;
  int c[16];
#pragma unroll
  for (int k = 0; k < 16; k++) c[k] = 0;
  for (int j = 0; j < N; j++) {
    const int d = row_distance(own, s_desc, j);
#pragma unroll
    for (int k = 0; k < 16; k++) c[k] += d <= 16 * k + 15 ? 1 : 0;
  }
  int b = 0;   // buckets that end below the rank: 16 = every value up to 255 does, the element is 256
#pragma unroll
  for (int k = 0; k < 16; k++) b += c[k] < need ? 1 : 0;
  const int base = 16 * b;
#pragma unroll
  for (int m = 0; m < 15; m++) c[m] = 0;
  for (int j = 0; j < N; j++) {
    const int e = row_distance(own, s_desc, j) - base;
#pragma unroll
    for (int m = 0; m < 15; m++) c[m] += e <= m ? 1 : 0;
  }
  int v = base;   // #{d <= base + 15} >= need by the choice of b (b = 16: #{d <= 256} = N)
#pragma unroll
  for (int m = 0; m < 15; m++) v += c[m] < need ? 1 : 0;
  return v;
}

__global__ __launch_bounds__(64 * REFRESH_WAVES) void k_refresh_points(RefreshArgs a) {
  __shared__ __attribute__((aligned(16))) uint8_t smem[kLdsRefreshBytes];
  constexpr LdsRefreshWave L;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  uint8_t* mine = smem + (size_t)wave * L.bytes;
  uint32_t* s_desc = lds_at<uint32_t>(mine, L.desc);
  double* s_term = lds_at<double>(mine, L.term);
  uint16_t* s_pos = lds_at<uint16_t>(mine, L.pos);
  const int p = blockIdx.x * REFRESH_WAVES + wave;
  const bool have_point = p < a.n_points;   // (a wave without a point still takes part in the barriers)

  // 1. status
  int o0 = 0, n = 0, status = 0;
  if (have_point) {
    o0 = a.off[p];
    n = a.off[p + 1] - o0;
    if ((a.point_bad && a.point_bad[p]) || n <= 0) status = SD_REFRESH_SKIPPED;
    else if (n > REFRESH_CAP) status = SD_REFRESH_TOO_MANY;
    else if (o0 < 0 || o0 + n > min(a.n_obs, a.off[a.n_points]) || a.ref_obs[p] < 0 || a.ref_obs[p] >= n) status = SD_REFRESH_BAD_INDEX;
  }
  if (have_point && status == 0) {
    int why = 0;
    for (int o = lane; o < n; o += 64) {
      ObsAt at;
      why |= locate_obs(a, a.frame[o0 + o], a.kp[o0 + o], &at);
    }
    const bool not_resident = __ballot(why & SD_REFRESH_NOT_RESIDENT) != 0, bad_index = __ballot(why & SD_REFRESH_BAD_INDEX) != 0;
    status = not_resident ? SD_REFRESH_NOT_RESIDENT : (bad_index ? SD_REFRESH_BAD_INDEX : 0);
  }
  const bool run = have_point && status == 0;   // wave-uniform
  double X[3] = {0.0, 0.0, 0.0};
  if (run)
    for (int k = 0; k < 3; k++) X[k] = a.Xw[(size_t)p * 3 + k];

  // 2. the terms of the normal, one observation per lane
  if (run)
    for (int o = lane; o < n; o += 64) {
      ObsAt at;
      (void)locate_obs(a, a.frame[o0 + o], a.kp[o0 + o], &at);
      double d[3];
      const double len = view_vector(X, at.centre, d);
      for (int k = 0; k < 3; k++) s_term[LdsRefreshWave::term_at(k, o)] = __ddiv_rn(d[k], len);
    }
  __syncthreads();
  float mf_max = 0.f, mf_min = 0.f;
  if (run && lane < 3) {   // normal = normal + normali / normali.norm(), in list order; then normal / n
    double sum = 0.0;
    for (int o = 0; o < n; o++) sum = __dadd_rn(sum, s_term[LdsRefreshWave::term_at(lane, o)]);
    const double nk = __ddiv_rn(sum, (double)n);
    a.normal[(size_t)p * 3 + lane] = nk;
    if (a.lm_normal) a.lm_normal[(size_t)p * 3 + lane] = nk;
  }
  if (run && lane == 3) {
    const int o = a.ref_obs[p];
    ObsAt at;
    (void)locate_obs(a, a.frame[o0 + o], a.kp[o0 + o], &at);
    double d[3];
    const float dist = (float)view_vector(X, at.centre, d);
    mf_max = __fmul_rn(dist, a.sf[min(max(at.kp->octave, 0), a.nlevels - 1)]);
    mf_min = __fdiv_rn(mf_max, a.sf[a.nlevels - 1]);
    a.max_dist[p] = mf_max;
    a.min_dist[p] = mf_min;
    if (a.lm_mfmax) {   // GetMaxDistanceInvariance / GetMinDistanceInvariance: 1.2f * mfMaxDistance, 0.8f * mfMinDistance
      a.lm_mfmax[p] = mf_max;
      a.lm_max[p] = __fmul_rn(1.2f, mf_max);
      a.lm_min[p] = __fmul_rn(0.8f, mf_min);
    }
  }
  __syncthreads();   // the terms are read: the descriptors may take their place

  // 3. the descriptors of the keyframes that are not bad, compacted in order
  int N = 0;
  if (run)
    for (int o_base = 0; o_base < n; o_base += 64) {
      const int o = o_base + lane;
      const bool take = o < n && !(a.kf_bad && a.kf_bad[o0 + o]);
      const int j = wave_append(take, lanemask_lt(lane), N);
      if (take) {
        ObsAt at;
        (void)locate_obs(a, a.frame[o0 + o], a.kp[o0 + o], &at);
        uint32_t w[8];
        load_desc8((const uint32_t*)at.desc, 0, w);
#pragma unroll
        for (int k = 0; k < 8; k++) s_desc[LdsRefreshWave::desc_word(k, j)] = w[k];
        s_pos[j] = (uint16_t)o;
      }
    }
  __syncthreads();
  uint32_t best = 0xFFFFFFFFu;
  if (run && N > 0) {
    const int rank = (N - 1) / 2;   // vDists[0.5 * (N - 1)]
    for (int i0 = 0; i0 < N; i0 += 64) {
      const int i = i0 + lane;
      if (i < N) {
        uint32_t own[8];
#pragma unroll
        for (int w = 0; w < 8; w++) own[w] = s_desc[LdsRefreshWave::desc_word(w, i)];
        best = min(best, ((uint32_t)row_median(own, s_desc, N, rank) << 9) | (uint32_t)i);
      }
    }
  }
  best = wave_min_u32(best);
  if (run && N > 0) {
    const int row = (int)(best & 511u);
    if (lane < 8) {
      const uint32_t w = s_desc[LdsRefreshWave::desc_word(lane, row)];
      ((uint32_t*)(a.desc + (size_t)p * 32))[lane] = w;
      if (a.lm_desc) ((uint32_t*)(a.lm_desc + (size_t)p * 32))[lane] = w;
    }
    if (lane == 8) {
      a.best_obs[p] = (int32_t)s_pos[row];
      a.best_median[p] = (int32_t)(best >> 9);
    }
    status |= SD_REFRESH_DESC;
  }
  if (run) status |= SD_REFRESH_NORMAL;
  if (have_point && lane == 0) a.status[p] = (uint8_t)status;
}

static int launch_refresh_args(const RefreshArgs& a, hipStream_t s) {
  if (a.n_points == 0) return SD_OK;
  hipLaunchKernelGGL(k_refresh_points, dim3((a.n_points + REFRESH_WAVES - 1) / REFRESH_WAVES), dim3(64 * REFRESH_WAVES), 0, s, a);
  SD_HIP_CHECK(hipGetLastError());
  return SD_OK;
}

int launch_refresh(const sd_orb* cur, const sd_orb* ref, const TrackBuffers& tb, const RefreshBuffers& rf, const float* d_sf, int n_batch,
                   int point_row, int write_local, hipStream_t s) {
  RefreshArgs a{};
  a.off = (const int32_t*)(rf.obs + rf.o_off);
  a.ref_obs = (const int32_t*)(rf.obs + rf.o_ref);
  a.frame = (const int32_t*)(rf.obs + rf.o_frame);
  a.kp = (const int32_t*)(rf.obs + rf.o_kp);
  a.point_bad = rf.o_pbad ? rf.obs + rf.o_pbad : nullptr;
  a.kf_bad = rf.o_kbad ? rf.obs + rf.o_kbad : nullptr;
  a.n_points = rf.n_points;
  a.n_obs = rf.n_obs;
  a.ref_kps = keys_un(ref);
  a.ref_desc = ref->d_desc;
  a.ref_nkp = ref->d_nout;
  a.ref_cap = keypoint_capacity(ref);
  a.n_ref = ref->have_geom ? std::min(n_batch, ref->last_frames) : 0;
  a.cur_kps = keys_un(cur);
  a.cur_desc = cur->d_desc;
  a.cur_nkp = cur->d_nout;
  a.cur_cap = tb.kp_cap;
  const int cf = tb.cur_bcast >= 0 ? tb.cur_bcast : 0;
  a.cur_frame = cur->have_geom && cur->last_frames > cf ? cf : -1;
  a.centre = rf.centre;
  const size_t row = (size_t)point_row * tb.max_points;
  a.Xw = tb.lm_Xw + row * 3;
  a.sf = d_sf;
  a.nlevels = cur->nlevels;
  a.status = rf.status;
  a.best_obs = rf.best_obs;
  a.best_median = rf.best_median;
  a.desc = rf.desc;
  a.normal = rf.normal;
  a.max_dist = rf.max_dist;
  a.min_dist = rf.min_dist;
  if (write_local) {
    a.lm_desc = tb.lm_desc + row * 32;
    a.lm_normal = tb.lm_normal + row * 3;
    a.lm_min = tb.lm_min + row;
    a.lm_max = tb.lm_max + row;
    a.lm_mfmax = tb.lm_mfmax + row;
  }
  // the centres of all n_batch slots: a pose that was never set is zeros, and no observation that passes locate_obs reads it
  hipLaunchKernelGGL(k_refresh_centres, dim3((a.n_ref + 1 + 63) / 64), dim3(64), 0, s, tb.Tref, tb.Tcur, a.n_ref, rf.centre);
  SD_HIP_CHECK(hipGetLastError());
  return launch_refresh_args(a, s);
}

// The packed observation block of n_points points and n_obs observations: offsets of its arrays and its size
struct ObsPack {
  size_t off, ref, frame, kp, pbad, kbad, bytes;
  ObsPack(size_t n_points, size_t n_obs) {
    size_t b = 16;   // (offset 0 is "absent")
    auto take = [&](size_t n) { const size_t o = b; b = align_up(b + n, 16); return o; };
    off = take((n_points + 1) * 4);
    ref = take(n_points * 4);
    frame = take(n_obs * 4);
    kp = take(n_obs * 4);
    pbad = take(n_points);
    kbad = take(n_obs);
    bytes = b;
  }
};

}  // namespace sd

using namespace sd;

// sd_track_create / sd_track_destroy (track.hip)
int refresh_create(sd_track* h) {
  RefreshBuffers& rf = h->rf;
  rf.n_points = -1;
  rf.obs_bytes = ObsPack((size_t)h->max_points, (size_t)h->max_points * 16).bytes;
  SD_HIP_CHECK(hipMalloc((void**)&rf.obs, rf.obs_bytes));
  SD_HIP_CHECK(hipMalloc((void**)&rf.twin, rf.obs_bytes));
  SD_HIP_CHECK(hipHostMalloc((void**)&rf.stage, rf.obs_bytes, hipHostMallocDefault));
  SD_HIP_CHECK(hipEventCreateWithFlags(&rf.ev_staged, hipEventDisableTiming));
  return SD_OK;
}
void refresh_destroy(sd_track* h) {
  RefreshBuffers& rf = h->rf;
  if (rf.obs) (void)hipFree(rf.obs);
  if (rf.twin) (void)hipFree(rf.twin);
  if (rf.stage) (void)hipHostFree(rf.stage);
  if (rf.ev_staged) (void)hipEventDestroy(rf.ev_staged);
  rf.obs = rf.twin = rf.stage = nullptr;
  rf.ev_staged = nullptr;
}

namespace {

// What both entries check of the lists themselves; *total = obs_off[n_points]
int check_lists(int n_points, const int32_t* obs_off, const int32_t* ref_obs, int* total) {
  SD_REQUIRE(n_points >= 0 && obs_off && (n_points == 0 || ref_obs), SD_ERR_INVALID_ARG, "NULL list or negative n_points");
  SD_REQUIRE(obs_off[0] == 0, SD_ERR_INVALID_ARG, "obs_off[0] must be 0");
  for (int i = 0; i < n_points; i++) {
    SD_REQUIRE(obs_off[i + 1] >= obs_off[i], SD_ERR_INVALID_ARG, "obs_off is not monotone");
    const int len = obs_off[i + 1] - obs_off[i];
    SD_REQUIRE(len == 0 || (ref_obs[i] >= 0 && ref_obs[i] < len), SD_ERR_INVALID_ARG, "ref_obs outside the point's list");
  }
  *total = obs_off[n_points];
  return SD_OK;
}

const char* const kNoRefresh =
    "sd_track_refresh_points has not run (or the extractions, poses, local points, observations or the broadcast setting were "
    "replaced since)";

}  // namespace

extern "C" {

int sd_track_set_observations(sd_track* h, int n_points, const int32_t* obs_off, const int32_t* obs_frame, const int32_t* obs_kp,
                              const uint8_t* obs_kf_bad, const int32_t* ref_obs, const uint8_t* point_bad) {
  SD_REQUIRE(h, SD_ERR_INVALID_ARG, "handle is NULL");
  SD_REQUIRE(n_points <= h->max_points, SD_ERR_CAPACITY, "n_points exceeds max_points");
  int total = 0;
  SD_TRY(check_lists(n_points, obs_off, ref_obs, &total));
  SD_REQUIRE(total == 0 || (obs_frame && obs_kp), SD_ERR_INVALID_ARG, "NULL observation array");
  int max_ref = -1;
  bool has_cur = false;
  for (int o = 0; o < total; o++) {
    SD_REQUIRE(obs_frame[o] >= -2 && obs_frame[o] < h->max_batch, SD_ERR_INVALID_ARG, "obs_frame outside [-2, max_batch)");
    max_ref = std::max(max_ref, obs_frame[o]);
    has_cur = has_cur || obs_frame[o] == -1;
  }
  SD_HIP_CHECK(hipSetDevice(h->device));
  END_RESULTS(h, "sd_track_set_observations");
  RefreshBuffers& rf = h->rf;
  rf.n_points = -1;
  const ObsPack pk((size_t)n_points, (size_t)total);
  if (pk.bytes > rf.obs_bytes) {   // the one grow-only allocation (track_internal.h): queued kernels may still read the old block
    SD_HIP_CHECK(hipStreamSynchronize(h->pnp_stream));
    uint8_t *d = nullptr, *tw = nullptr, *st = nullptr;
    const size_t want = std::max(pk.bytes, rf.obs_bytes * 2);
    SD_HIP_CHECK(hipMalloc((void**)&d, want));
    hipError_t e = hipMalloc((void**)&tw, want);
    if (e == hipSuccess) e = hipHostMalloc((void**)&st, want, hipHostMallocDefault);
    if (e != hipSuccess) {
      (void)hipFree(d);
      if (tw) (void)hipFree(tw);
      return hip_error("sd_track_set_observations", e);
    }
    (void)hipFree(rf.obs);
    (void)hipFree(rf.twin);
    (void)hipHostFree(rf.stage);
    rf.obs = d;
    rf.twin = tw;
    rf.stage = st;
    rf.obs_bytes = want;
    rf.staged = false;
  }
  SD_TRY(ba_grow(h, (size_t)total));   // the bundle adjustment's scratch holds as many observations as this block
  SD_TRY(cull_grow(h, (size_t)total));   // ... and so does the culling's
  if (rf.staged) SD_HIP_CHECK(hipEventSynchronize(rf.ev_staged));   // the last upload has left the pinned block
  uint8_t* st = rf.stage;
  std::memcpy(st + pk.off, obs_off, ((size_t)n_points + 1) * 4);
  if (n_points) std::memcpy(st + pk.ref, ref_obs, (size_t)n_points * 4);
  if (total) {
    std::memcpy(st + pk.frame, obs_frame, (size_t)total * 4);
    std::memcpy(st + pk.kp, obs_kp, (size_t)total * 4);
    if (obs_kf_bad) std::memcpy(st + pk.kbad, obs_kf_bad, (size_t)total);
  }
  if (point_bad && n_points) std::memcpy(st + pk.pbad, point_bad, (size_t)n_points);
  SD_HIP_CHECK(hipMemcpyAsync(rf.obs, st, pk.bytes, hipMemcpyHostToDevice, h->pnp_stream));
  SD_HIP_CHECK(hipEventRecord(rf.ev_staged, h->pnp_stream));
  rf.staged = true;
  rf.o_off = pk.off; rf.o_ref = pk.ref; rf.o_frame = pk.frame; rf.o_kp = pk.kp;
  rf.o_pbad = point_bad ? pk.pbad : 0;
  rf.o_kbad = obs_kf_bad ? pk.kbad : 0;
  rf.at_pbad = pk.pbad; rf.at_kbad = pk.kbad;
  rf.serial++;
  rf.n_points = n_points;
  rf.n_obs = total;
  rf.max_ref_frame = max_ref;
  rf.has_cur = has_cur;
  return SD_OK;
}

int sd_track_refresh_points(sd_track* h, int point_row, int write_local) {
  SD_REQUIRE(h, SD_ERR_INVALID_ARG, "handle is NULL");
  SD_REQUIRE(h->rf.n_points >= 0, SD_ERR_INVALID_ARG, "sd_track_set_observations has not been called");
  SD_REQUIRE(point_row >= 0 && point_row < h->max_batch, SD_ERR_INVALID_ARG, "point_row outside [0, max_batch)");
  SD_REQUIRE(write_local == 0 || write_local == 1, SD_ERR_INVALID_ARG, "write_local must be 0 or 1");
  SD_REQUIRE(h->rf.max_ref_frame < 0 || (h->ref->have_geom && h->ref->last_frames > h->rf.max_ref_frame), SD_ERR_INVALID_ARG,
             "an observation names a frame of the ref extractor that has not been extracted");
  const int cf = h->tb.cur_bcast >= 0 ? h->tb.cur_bcast : 0;
  SD_REQUIRE(!h->rf.has_cur || (h->cur->have_geom && h->cur->last_frames > cf), SD_ERR_INVALID_ARG,
             "an observation names the current keyframe, which has not been extracted");
  SD_HIP_CHECK(hipSetDevice(h->device));
  if (write_local) END_RESULTS(h, "sd_track_refresh_points(write_local)");
  else END_RESULTS(h, "sd_track_refresh_points");
  SD_TRY(run_stage(h, true, false, STAGE_NONE, [&](hipStream_t s) {
    return launch_refresh(h->cur, h->ref, h->tb, h->rf, h->d_sf, h->max_batch, point_row, write_local, s);
  }));
  h->res.refresh.set(1, BIND_REFRESH, inputs_now(h), h->rf.n_points);
  return SD_OK;
}

int sd_track_get_refreshed(sd_track* h, uint8_t* status, int32_t* best_obs, int32_t* best_median, uint8_t* desc, double* normal,
                           float* max_dist, float* min_dist, int cap) {
  TRACK_RANGE(h, 0, 1);
  SD_REQUIRE(h->res.refresh.live(1, inputs_now(h)), SD_ERR_INVALID_ARG, kNoRefresh);
  const size_t n = (size_t)h->res.refresh.payload;
  SD_REQUIRE(!(status || best_obs || best_median || desc || normal || max_dist || min_dist) || (cap >= 0 && (size_t)cap >= n),
             SD_ERR_CAPACITY, "cap smaller than the number of points");
  if (n == 0) return SD_OK;
  hipStream_t s = h->cur->stream;
  const RefreshBuffers& rf = h->rf;
  SD_TRY(download(status, rf.status, 0, n, 1, s));
  SD_TRY(download(best_obs, rf.best_obs, 0, n, 1, s));
  SD_TRY(download(best_median, rf.best_median, 0, n, 1, s));
  SD_TRY(download(desc, rf.desc, 0, n, 32, s));
  SD_TRY(download(normal, rf.normal, 0, n, 3, s));
  SD_TRY(download(max_dist, rf.max_dist, 0, n, 1, s));
  SD_TRY(download(min_dist, rf.min_dist, 0, n, 1, s));
  return wait_for(s);
}

int sd_debug_refresh_points(int n_points, const int32_t* obs_off, const uint8_t* obs_desc, const double* obs_centre,
                            const int32_t* obs_octave, const uint8_t* obs_kf_bad, const int32_t* ref_obs, const uint8_t* point_bad,
                            const double* Xw, const float* scale_factors, int nlevels, uint8_t* status, int32_t* best_obs,
                            int32_t* best_median, uint8_t* desc, double* normal, float* max_dist, float* min_dist) {
  int total = 0;
  SD_TRY(check_lists(n_points, obs_off, ref_obs, &total));
  SD_REQUIRE(n_points <= (1 << 20) && total <= (1 << 24), SD_ERR_CAPACITY, "at most 2^20 points and 2^24 observations");
  SD_REQUIRE((total == 0 || (obs_desc && obs_centre && obs_octave)) &&
                 (n_points == 0 || (Xw && status && best_obs && best_median && desc && normal && max_dist && min_dist)),
             SD_ERR_INVALID_ARG, "NULL array");
  SD_REQUIRE(scale_factors && nlevels >= 1 && nlevels <= SD_MAX_LEVELS, SD_ERR_INVALID_ARG, "bad scale table");
  if (n_points == 0) return SD_OK;
  // every observation is a keyframe of its own with one keypoint: frame o, keypoint 0
  const size_t P = (size_t)n_points, O = (size_t)std::max(total, 1);
  std::vector<sd_keypoint> kps(O);
  std::vector<int32_t> frame(O), kp(O, 0), nkp(O, 1);
  for (int o = 0; o < total; o++) {
    kps[o] = sd_keypoint{0, 0, 0, 0, 0, obs_octave[o], -1};
    frame[o] = o;
  }
  Blob b;
  const size_t o_off = b.reserve(P + 1, obs_off, P + 1), o_ref = b.reserve(P, ref_obs, P);
  const size_t o_pb = b.reserve(P, point_bad, point_bad ? P : 0), o_fr = b.reserve(O, frame.data(), O), o_kp = b.reserve(O, kp.data(), O);
  const size_t o_kb = b.reserve(O, obs_kf_bad, obs_kf_bad ? (size_t)total : 0), o_k = b.reserve(O, kps.data(), O);
  const size_t o_d = b.reserve(O * 32, obs_desc, (size_t)total * 32), o_nk = b.reserve(O, nkp.data(), O);
  const size_t o_c = b.reserve(O * 3 + 3, obs_centre, (size_t)total * 3), o_X = b.reserve(P * 3, Xw, P * 3);
  const size_t o_sf = b.reserve(nlevels, scale_factors, nlevels);
  // the outputs start as the caller's arrays: what the kernel does not write comes back unchanged
  const size_t r_st = b.reserve(P, status, P), r_bo = b.reserve(P, best_obs, P), r_bm = b.reserve(P, best_median, P);
  const size_t r_d = b.reserve(P * 32, desc, P * 32), r_n = b.reserve(P * 3, normal, P * 3);
  const size_t r_mx = b.reserve(P, max_dist, P), r_mn = b.reserve(P, min_dist, P);
  SD_TRY(b.run("sd_debug_refresh_points", [&] {
    RefreshArgs a{};
    a.off = b.dev<int32_t>(o_off); a.ref_obs = b.dev<int32_t>(o_ref); a.point_bad = point_bad ? b.dev<uint8_t>(o_pb) : nullptr;
    a.frame = b.dev<int32_t>(o_fr); a.kp = b.dev<int32_t>(o_kp); a.kf_bad = obs_kf_bad ? b.dev<uint8_t>(o_kb) : nullptr;
    a.n_points = n_points; a.n_obs = total;
    a.ref_kps = b.dev<sd_keypoint>(o_k); a.ref_desc = b.dev<uint8_t>(o_d); a.ref_nkp = b.dev<int32_t>(o_nk);
    a.ref_cap = 1; a.n_ref = total; a.cur_frame = -1;
    a.centre = b.dev<double>(o_c); a.Xw = b.dev<double>(o_X); a.sf = b.dev<float>(o_sf); a.nlevels = nlevels;
    a.status = b.dev<uint8_t>(r_st); a.best_obs = b.dev<int32_t>(r_bo); a.best_median = b.dev<int32_t>(r_bm);
    a.desc = b.dev<uint8_t>(r_d); a.normal = b.dev<double>(r_n); a.max_dist = b.dev<float>(r_mx); a.min_dist = b.dev<float>(r_mn);
    return launch_refresh_args(a, 0);
  }));
  b.take(status, r_st, P);
  b.take(best_obs, r_bo, P * 4);
  b.take(best_median, r_bm, P * 4);
  b.take(desc, r_d, P * 32);
  b.take(normal, r_n, P * 24);
  b.take(max_dist, r_mx, P * 4);
  b.take(min_dist, r_mn, P * 4);
  return SD_OK;
}

}  // extern "C"
