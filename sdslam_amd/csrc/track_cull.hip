// LocalMapping::KeyFrameCulling and the erasure of observations on MI355X, on the resident lists of sd_track_set_observations
//   KeyFrameCulling()                   reference src/LocalMapping.cc:580-634
//   KeyFrame::SetBadFlag()              src/KeyFrame.cc:430-446 (the map-point part)
//   MapPoint::EraseObservation()        src/MapPoint.cc:110-134
//   MapPoint::SetBadFlag()              src/MapPoint.cc:146-161
//
// The lists are those of track_refresh.hip: point p owns the entries obs_off[p] .. obs_off[p + 1] - 1 in the caller's order, a
// keyframe is a frame of `ref` (>= 0), the current keyframe (-1) or not resident (-2).  A keyframe appears at most once in a list
// (mObservations is a map).  A point whose point_bad is set has, in the reference, neither observations nor matches (SetBadFlag
// cleared both): its entries are nobody's, no call here reads, counts or kills them.
//
// k_cull_gather   lane per point: per entry its camera, octave, mvDepth and weight in nObs (2 where mvuRight >= 0), per point the
//                 refusal bits.  The debug entry supplies these arrays itself.
// k_cull          ONE workgroup of 1024 lanes walks the candidates in order over state kept in global memory (dead, nObs, ref_obs,
//                 bad).  Point p belongs to lane p % 1024 in every step of every candidate, so a point's state has one reader and
//                 one writer for the whole run and needs no fence; the only values that cross lanes are nRedundant and nMPs, which
//                 go through the wave reduction of sd_wave.h and a 16-entry LDS table summed in wave order.  A camera -> entries
//                 transpose would save the scan of each point's list for the candidate's entry, a handful of entries a point, and
//                 costs a counting pass and a second index: not built (DESIGN.md section 4 has the measured time).
// k_erase         ONE workgroup: mark (lane per point: nObs falls by the weights of the killed entries, a point with a killed
//                 entry and nObs <= 2 loses every entry), an exclusive prefix sum over the survivor counts, a stable move of the
//                 survivors into the twin block.  The order in which a point's entries are erased cannot matter: nObs only falls,
//                 so "nObs <= 2 at some erasure" is "nObs <= 2 after all of them", and a bad point loses every entry either way.
// No atomics of any kind; stores are plain vector stores.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <type_traits>
#include <vector>

#include "sd_wave.h"
#include "track_handle.h"

namespace sd {

constexpr int CULL_LANES = 1024, CULL_WAVES = CULL_LANES / 64;

struct CullLists {
  const int32_t* off;        // [n_points + 1]
  const int32_t* ref_obs;    // [n_points]
  const uint8_t* point_bad;  // [n_points] or NULL
  int n_points;
  // per entry (k_cull_gather, or the debug entry's arrays)
  const int32_t* e_kf;
  const int32_t* e_oct;
  const float* e_depth;
  const uint8_t* e_w;
  const uint8_t* p_flag;     // [n_points] SD_CULL_NOT_RESIDENT / SD_CULL_BAD_INDEX of the point's entries
};

struct CullArgs {
  CullLists l;
  const int32_t* cand;       // [n_cand] frames, then [n_cand] flags
  int n_cand, monocular;
  float th_depth;
  uint8_t* verdict;
  int32_t* counts2;
  uint8_t* dead;
  uint8_t* pbad;
  int32_t* ref_new;
  int32_t* nobs;
  int32_t* info;
};

// What the gather reads of the handle
struct CullGather {
  const int32_t* off;
  const uint8_t* point_bad;
  const int32_t* frame;
  const int32_t* kp;
  int n_points;
  const sd_keypoint* ref_kps;
  const int32_t* ref_nkp;
  const float* ref_ur;
  const float* ref_depth;
  int ref_cap, n_ref;
  const sd_keypoint* cur_kps;
  const int32_t* cur_nkp;
  const float* cur_ur;
  int cur_cap, cur_frame, cur_cam;
  int32_t* e_kf;
  int32_t* e_oct;
  float* e_depth;
  uint8_t* e_w;
  uint8_t* p_flag;
};

__global__ __launch_bounds__(256) void k_cull_gather(CullGather g) {
  const int p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= g.n_points) return;
  const bool pbad = g.point_bad && g.point_bad[p];
  int why = 0;
  for (int e = g.off[p]; e < g.off[p + 1]; e++) {
    const int fr = g.frame[e], k = g.kp[e];
    const bool cur = fr == -1;
    int kf = -2, oct = 0, w = 1;
    float depth = -1.f;
    if (fr == -2) why |= SD_CULL_NOT_RESIDENT;
    else if (fr < -2 || fr >= g.n_ref || (cur && g.cur_frame < 0)) why |= SD_CULL_BAD_INDEX;
    else {
      const int f = cur ? g.cur_frame : fr, cap = cur ? g.cur_cap : g.ref_cap;
      const int nk = min((cur ? g.cur_nkp : g.ref_nkp)[f], cap);
      if (k < 0 || k >= nk) why |= SD_CULL_BAD_INDEX;
      else {
        const size_t at = (size_t)f * cap + k;
        kf = cur ? g.cur_cam : fr;
        oct = (cur ? g.cur_kps : g.ref_kps)[at].octave;
        w = (cur ? g.cur_ur : g.ref_ur)[at] >= 0.f ? 2 : 1;
        if (!cur) depth = g.ref_depth[at];   // only a ref frame can be a candidate
      }
    }
    g.e_kf[e] = kf; g.e_oct[e] = oct; g.e_depth[e] = depth; g.e_w[e] = (uint8_t)w;
  }
  g.p_flag[p] = pbad ? 0 : (uint8_t)why;   // a bad point's entries are nobody's
}

// Sum of v over the workgroup, every lane gets it: wave reduction, then the waves' sums in wave order
__device__ __forceinline__ int cull_block_sum(int v, int* s_red) {
  const int s = wave_sum_i32(v);
  __syncthreads();   // the table's last readers are done
  if ((threadIdx.x & 63) == 0) s_red[threadIdx.x >> 6] = s;
  __syncthreads();
  int t = 0;
  for (int w = 0; w < CULL_WAVES; w++) t += s_red[w];
  return t;
}

// The live entry of [o0, o1) in camera f, -1: none
__device__ __forceinline__ int cull_find(const CullArgs& a, int o0, int o1, int f) {
  for (int e = o0; e < o1; e++)
    if (a.l.e_kf[e] == f && !a.dead[e]) return e;
  return -1;
}

__global__ __launch_bounds__(CULL_LANES) void k_cull(CullArgs a) {
  __shared__ int s_red[CULL_WAVES];
  const int t = threadIdx.x, P = a.l.n_points;
  // the refusals, before anything is written
  int why = 0;
  for (int p = t; p < P; p += CULL_LANES) why |= a.l.p_flag[p];
  const int nr = cull_block_sum((why & SD_CULL_NOT_RESIDENT) ? 1 : 0, s_red), bi = cull_block_sum((why & SD_CULL_BAD_INDEX) ? 1 : 0, s_red);
  if (nr || bi) {
    if (t < 8) a.info[t] = t == 0 ? (nr ? SD_CULL_NOT_RESIDENT : SD_CULL_BAD_INDEX) : 0;
    return;
  }
  for (int p = t; p < P; p += CULL_LANES) {
    const int o0 = a.l.off[p], o1 = a.l.off[p + 1];
    int n = 0;
    for (int e = o0; e < o1; e++) { n += a.l.e_w[e]; a.dead[e] = 0; }
    a.nobs[p] = n;
    a.pbad[p] = 0;
    a.ref_new[p] = a.l.ref_obs[p];
  }
  int n_culled = 0, n_tbe = 0, n_dead = 0, n_bad = 0;   // n_dead, n_bad: this lane's share
  for (int c = 0; c < a.n_cand; c++) {
    const int f = a.cand[c], fl = a.cand[a.n_cand + c];
    if (fl & 1) {   // mnId == 0 (:589)
      if (t == 0) { a.verdict[c] = SD_CULL_SKIPPED_ID0; a.counts2[2 * c] = 0; a.counts2[2 * c + 1] = 0; }
      continue;
    }
    int nMPs = 0, nRed = 0;
    for (int p = t; p < P; p += CULL_LANES) {
      if ((a.l.point_bad && a.l.point_bad[p]) || a.pbad[p]) continue;
      const int o0 = a.l.off[p], o1 = a.l.off[p + 1];
      const int i = cull_find(a, o0, o1, f);
      if (i < 0) continue;
      if (!a.monocular) {
        const float d = a.l.e_depth[i];
        if (d > a.th_depth || d < 0.f) continue;
      }
      nMPs++;
      if (a.nobs[p] > 3) {
        const int lim = a.l.e_oct[i] + 1;
        int n = 0;
        for (int e = o0; e < o1; e++) n += (e != i && !a.dead[e] && a.l.e_oct[e] <= lim) ? 1 : 0;
        nRed += n >= 3 ? 1 : 0;
      }
    }
    nMPs = cull_block_sum(nMPs, s_red);
    nRed = cull_block_sum(nRed, s_red);
    const bool cull = (double)nRed > 0.9 * (double)nMPs;
    const int verdict = !cull ? SD_CULL_KEPT : ((fl & 2) ? SD_CULL_TO_BE_ERASED : SD_CULL_CULLED);
    if (t == 0) { a.verdict[c] = (uint8_t)verdict; a.counts2[2 * c] = nRed; a.counts2[2 * c + 1] = nMPs; }
    n_culled += verdict == SD_CULL_CULLED;
    n_tbe += verdict == SD_CULL_TO_BE_ERASED;
    if (verdict != SD_CULL_CULLED) continue;
    // KeyFrame::SetBadFlag: EraseObservation(pKF) on every point it holds
    for (int p = t; p < P; p += CULL_LANES) {
      if ((a.l.point_bad && a.l.point_bad[p]) || a.pbad[p]) continue;
      const int o0 = a.l.off[p], o1 = a.l.off[p + 1];
      const int i = cull_find(a, o0, o1, f);
      if (i < 0) continue;
      a.dead[i] = 1;
      n_dead++;
      const int n = a.nobs[p] - a.l.e_w[i];
      a.nobs[p] = n;
      if (a.ref_new[p] == i - o0) {   // mpRefKF = mObservations.begin()->first
        int first = -1;
        for (int e = o1 - 1; e >= o0; e--) first = a.dead[e] ? first : e - o0;
        a.ref_new[p] = first;
      }
      if (n <= 2) {   // MapPoint::SetBadFlag
        a.pbad[p] = 1;
        n_bad++;
        for (int e = o0; e < o1; e++)
          if (!a.dead[e]) { a.dead[e] = 2; n_dead++; }
      }
    }
  }
  n_dead = cull_block_sum(n_dead, s_red);
  n_bad = cull_block_sum(n_bad, s_red);
  if (t < 8) a.info[t] = t == 1 ? n_culled : (t == 2 ? n_tbe : (t == 3 ? n_dead : (t == 4 ? n_bad : 0)));
}

struct EraseArgs {
  // the lists as they stand
  const int32_t* off;
  const int32_t* ref_obs;
  const uint8_t* point_bad;  // or NULL
  const int32_t* frame;      // or NULL (the debug entry moves no payload)
  const int32_t* kp;
  const uint8_t* kf_bad;     // or NULL
  const uint8_t* e_w;
  const uint8_t* kill;       // [E] non-zero: the entry is erased
  const int32_t* gate;       // or NULL; gate[0] != 0: the run that left `kill` refused, nothing is erased
  int n_points, n_obs;       // n_obs: what the block was packed for (>= off[n_points])
  // the twin
  int32_t* off_new;
  int32_t* ref_new;
  uint8_t* pbad_new;
  int32_t* frame_new;
  int32_t* kp_new;
  uint8_t* kbad_new;
  // the record
  int32_t* map;
  int32_t* nobs;
  int32_t* cnt;
  int32_t* info;
};

__global__ __launch_bounds__(CULL_LANES) void k_erase(EraseArgs a) {
  __shared__ int s_scan[CULL_LANES];
  __shared__ int s_red[CULL_WAVES];
  const int t = threadIdx.x, P = a.n_points;
  const bool open = !a.gate || a.gate[0] == 0;
  // 1. mark: map[e] = 0 for a survivor, -1 otherwise
  int n_erased = 0, n_bad = 0;
  for (int p = t; p < P; p += CULL_LANES) {
    const int o0 = a.off[p], o1 = a.off[p + 1];
    const bool was_bad = a.point_bad && a.point_bad[p];
    const bool mine = open && !was_bad;   // a bad point's entries are nobody's: they stay as uploaded
    int n = 0, killed = 0;
    for (int e = o0; e < o1; e++) {
      const bool k = mine && a.kill[e] != 0;
      n += k ? 0 : a.e_w[e];
      killed += k;
    }
    const bool bad = killed > 0 && n <= 2;
    int keep = 0;
    for (int e = o0; e < o1; e++) {
      const bool k = bad || (mine && a.kill[e] != 0);
      a.map[e] = k ? -1 : 0;
      keep += !k;
    }
    n_erased += (o1 - o0) - keep;
    n_bad += bad && !was_bad;
    a.cnt[p] = keep;
    a.nobs[p] = bad ? 0 : n;
    a.pbad_new[p] = (was_bad || bad) ? 1 : 0;
  }
  __syncthreads();
  // 2. exclusive prefix sum over cnt: lane t owns points [t chunk, (t + 1) chunk)
  const int chunk = (P + CULL_LANES - 1) / CULL_LANES, p0 = min(t * chunk, P), p1 = min(p0 + chunk, P);
  int mine = 0;
  for (int p = p0; p < p1; p++) mine += a.cnt[p];
  s_scan[t] = mine;
  __syncthreads();
  for (int d = 1; d < CULL_LANES; d <<= 1) {
    const int v = t >= d ? s_scan[t - d] : 0;
    __syncthreads();
    s_scan[t] += v;
    __syncthreads();
  }
  int base = s_scan[t] - mine;
  const int total = s_scan[CULL_LANES - 1];
  for (int p = p0; p < p1; p++) { a.off_new[p] = base; base += a.cnt[p]; }
  if (t == 0) a.off_new[P] = total;
  __syncthreads();
  // 3. the stable move
  for (int p = t; p < P; p += CULL_LANES) {
    const int o0 = a.off[p], o1 = a.off[p + 1];
    const int old_ref = a.ref_obs[p];
    int at = a.off_new[p], ref = 0;
    const int first = at;
    for (int e = o0; e < o1; e++) {
      if (a.map[e] < 0) continue;
      if (e - o0 == old_ref) ref = at - first;   // mpRefKF survives; otherwise the first survivor, position 0
      a.map[e] = at;
      if (a.frame) {
        a.frame_new[at] = a.frame[e];
        a.kp_new[at] = a.kp[e];
        a.kbad_new[at] = a.kf_bad ? a.kf_bad[e] : 0;
      }
      at++;
    }
    a.ref_new[p] = ref;
  }
  n_erased = cull_block_sum(n_erased, s_red);
  n_bad = cull_block_sum(n_bad, s_red);
  if (t < 8) a.info[t] = t == 1 ? n_erased : (t == 2 ? n_bad : (t == 3 ? total : 0));
}

static int launch_cull(const CullArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_cull, dim3(1), dim3(CULL_LANES), 0, s, a);
  SD_HIP_CHECK(hipGetLastError());
  return SD_OK;
}
static int launch_erase(const EraseArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_erase, dim3(1), dim3(CULL_LANES), 0, s, a);
  SD_HIP_CHECK(hipGetLastError());
  return SD_OK;
}

static void cull_carve(CullBuffers& b, uint8_t* base, size_t P, size_t E, size_t C) {
  size_t o = 0;
  auto take = [&](auto** p, size_t count) {
    using T = std::remove_pointer_t<std::remove_pointer_t<decltype(p)>>;
    *p = (T*)(base + o);
    o = align_up(o + std::max<size_t>(count, 1) * sizeof(T), 16);
  };
  take(&b.e_kf, E); take(&b.e_oct, E); take(&b.e_depth, E); take(&b.e_w, E); take(&b.p_flag, P); take(&b.cand, 2 * C);
  take(&b.verdict, C); take(&b.counts2, 2 * C); take(&b.dead, E); take(&b.pbad, P); take(&b.ref_new, P); take(&b.nobs, P);
  take(&b.info, 8);
  take(&b.er_map, E); take(&b.er_nobs, P); take(&b.er_cnt, P); take(&b.er_info, 8);
  b.bytes = o;
  b.cap_points = P; b.cap_obs = E;
}

}  // namespace sd

using namespace sd;

static int cull_alloc(CullBuffers& b, size_t P, size_t E, size_t C) {
  CullBuffers probe{};
  cull_carve(probe, nullptr, P, E, C);
  uint8_t* base = nullptr;
  SD_HIP_CHECK(hipMalloc((void**)&base, probe.bytes));
  cull_carve(b, base, P, E, C);
  b.base = base;
  b.ran_cand = b.er_points = -1;
  return SD_OK;
}

// sd_track_create / sd_track_destroy (track.hip); sd_track_set_observations grows the scratch with its own block (track_refresh.hip)
int cull_create(sd_track* h) { return cull_alloc(h->cu, (size_t)h->max_points, (size_t)h->max_points * 16, (size_t)h->max_batch); }
void cull_destroy(sd_track* h) {
  if (h->cu.base) (void)hipFree(h->cu.base);
  h->cu.base = nullptr;
}
int cull_grow(sd_track* h, size_t n_obs) {
  if (n_obs <= h->cu.cap_obs) return SD_OK;
  SD_HIP_CHECK(hipStreamSynchronize(h->pnp_stream));   // queued kernels may still use the old scratch
  CullBuffers nb{};
  SD_TRY(cull_alloc(nb, h->cu.cap_points, std::max(n_obs, h->cu.cap_obs * 2), (size_t)h->max_batch));
  (void)hipFree(h->cu.base);
  h->cu = nb;   // the results of the last runs went with the old scratch
  return SD_OK;
}

namespace {

// k_cull_gather on the resident lists: what both calls begin with
int queue_gather(sd_track* h, hipStream_t s) {
  const RefreshBuffers& rf = h->rf;
  const TrackBuffers& tb = h->tb;
  CullGather g{};
  g.off = (const int32_t*)(rf.obs + rf.o_off);
  g.point_bad = rf.o_pbad ? rf.obs + rf.o_pbad : nullptr;
  g.frame = (const int32_t*)(rf.obs + rf.o_frame);
  g.kp = (const int32_t*)(rf.obs + rf.o_kp);
  g.n_points = rf.n_points;
  g.ref_kps = keys_un(h->ref);
  g.ref_nkp = h->ref->d_nout;
  g.ref_ur = tb.uright_ref;
  g.ref_depth = h->nb.depth_ref;
  g.ref_cap = keypoint_capacity(h->ref);
  g.n_ref = h->ref->have_geom ? std::min(h->max_batch, h->ref->last_frames) : 0;
  g.cur_kps = keys_un(h->cur);
  g.cur_nkp = h->cur->d_nout;
  g.cur_ur = tb.uright;
  g.cur_cap = tb.kp_cap;
  const int cf = tb.cur_bcast >= 0 ? tb.cur_bcast : 0;
  g.cur_frame = h->cur->have_geom && h->cur->last_frames > cf ? cf : -1;
  g.cur_cam = h->max_batch;
  g.e_kf = h->cu.e_kf; g.e_oct = h->cu.e_oct; g.e_depth = h->cu.e_depth; g.e_w = h->cu.e_w; g.p_flag = h->cu.p_flag;
  if (g.n_points == 0) return SD_OK;
  hipLaunchKernelGGL(k_cull_gather, dim3((g.n_points + 255) / 256), dim3(256), 0, s, g);
  SD_HIP_CHECK(hipGetLastError());
  return SD_OK;
}

// What both calls require of the handle before they read the extractors through the lists
int check_resident(const sd_track* h) {
  SD_REQUIRE(h->rf.n_points >= 0, SD_ERR_INVALID_ARG, "sd_track_set_observations has not been called");
  SD_REQUIRE(h->rf.max_ref_frame < 0 || (h->ref->have_geom && h->ref->last_frames > h->rf.max_ref_frame), SD_ERR_INVALID_ARG,
             "an observation names a frame of the ref extractor that has not been extracted");
  SD_REQUIRE(h->rf.max_ref_frame < 0 || keypoint_capacity(h->ref) == h->kp_cap, SD_ERR_INVALID_ARG,
             "cur / ref extractors must share the keypoint capacity");   // the mvuRight / mvDepth rows of both sides are kp_cap long
  const int cf = h->tb.cur_bcast >= 0 ? h->tb.cur_bcast : 0;
  SD_REQUIRE(!h->rf.has_cur || (h->cur->have_geom && h->cur->last_frames > cf), SD_ERR_INVALID_ARG,
             "an observation names the current keyframe, which has not been extracted");
  SD_REQUIRE((size_t)h->rf.n_obs <= h->cu.cap_obs && (size_t)h->rf.n_points <= h->cu.cap_points, SD_ERR_CAPACITY,
             "the observation lists exceed the culling's scratch");
  return SD_OK;
}

int check_csr(int n_points, const int32_t* obs_off, int* total) {
  SD_REQUIRE(n_points >= 0 && obs_off && obs_off[0] == 0, SD_ERR_INVALID_ARG, "NULL list, negative n_points or obs_off[0] != 0");
  for (int i = 0; i < n_points; i++) SD_REQUIRE(obs_off[i + 1] >= obs_off[i], SD_ERR_INVALID_ARG, "obs_off is not monotone");
  *total = obs_off[n_points];
  SD_REQUIRE(n_points <= (1 << 20) && *total <= (1 << 24), SD_ERR_CAPACITY, "at most 2^20 points and 2^24 observations");
  return SD_OK;
}

const char* const kNoCull = "sd_track_cull_keyframes has not run on the observation lists as they stand";
const char* const kNoErase = "sd_track_erase_observations has not run (or the observation lists were replaced since)";

}  // namespace

extern "C" {

int sd_track_cull_keyframes(sd_track* h, int n_cand, const int32_t* cand_frame, const uint8_t* cand_flags, int monocular, float th_depth) {
  SD_REQUIRE(h, SD_ERR_INVALID_ARG, "handle is NULL");
  SD_REQUIRE(n_cand >= 0 && (n_cand == 0 || (cand_frame && cand_flags)), SD_ERR_INVALID_ARG, "negative n_cand or NULL candidate array");
  SD_REQUIRE(monocular == 0 || monocular == 1, SD_ERR_INVALID_ARG, "monocular must be 0 or 1");
  std::vector<uint8_t> named((size_t)h->max_batch, 0);
  for (int c = 0; c < n_cand; c++) {
    SD_REQUIRE(cand_frame[c] >= 0 && cand_frame[c] < h->max_batch, SD_ERR_INVALID_ARG, "candidate outside [0, max_batch)");
    SD_REQUIRE(!named[cand_frame[c]], SD_ERR_INVALID_ARG, "a candidate is named twice");
    named[cand_frame[c]] = 1;
  }
  SD_TRY(check_resident(h));
  SD_HIP_CHECK(hipSetDevice(h->device));
  CullBuffers& cu = h->cu;
  cu.ran_cand = -1;
  if (n_cand) {
    std::vector<int32_t> packed(2 * (size_t)n_cand);
    for (int c = 0; c < n_cand; c++) { packed[c] = cand_frame[c]; packed[(size_t)n_cand + c] = cand_flags[c]; }
    SD_TRY(h->small_ring.upload(cu.cand, packed.data(), packed.size(), h->pnp_stream));
  }
  const RefreshBuffers& rf = h->rf;
  CullArgs a{};
  a.l.off = (const int32_t*)(rf.obs + rf.o_off);
  a.l.ref_obs = (const int32_t*)(rf.obs + rf.o_ref);
  a.l.point_bad = rf.o_pbad ? rf.obs + rf.o_pbad : nullptr;
  a.l.n_points = rf.n_points;
  a.l.e_kf = cu.e_kf; a.l.e_oct = cu.e_oct; a.l.e_depth = cu.e_depth; a.l.e_w = cu.e_w; a.l.p_flag = cu.p_flag;
  a.cand = cu.cand; a.n_cand = n_cand; a.monocular = monocular; a.th_depth = th_depth;
  a.verdict = cu.verdict; a.counts2 = cu.counts2; a.dead = cu.dead; a.pbad = cu.pbad; a.ref_new = cu.ref_new; a.nobs = cu.nobs;
  a.info = cu.info;
  SD_TRY(run_stage(h, true, false, STAGE_NONE, [&](hipStream_t s) {
    SD_TRY(queue_gather(h, s));
    return launch_cull(a, s);
  }));
  cu.ran_cand = n_cand;
  cu.ran_points = rf.n_points;
  cu.ran_obs = rf.n_obs;
  cu.ran_serial = rf.serial;
  return SD_OK;
}

int sd_track_get_culled(sd_track* h, uint8_t* verdict, int32_t* counts2, uint8_t* obs_dead, uint8_t* point_bad, int32_t* ref_obs,
                        int32_t* n_obs, int32_t* info8, int cap_cand, int cap_points, int cap_obs) {
  TRACK_RANGE(h, 0, 1);
  const CullBuffers& cu = h->cu;
  SD_REQUIRE(cu.ran_cand >= 0 && cu.ran_serial == h->rf.serial, SD_ERR_INVALID_ARG, kNoCull);
  const size_t C = (size_t)cu.ran_cand, P = (size_t)cu.ran_points, E = (size_t)cu.ran_obs;
  SD_REQUIRE(!(verdict || counts2) || (cap_cand >= 0 && (size_t)cap_cand >= C), SD_ERR_CAPACITY, "cap_cand smaller than the number of candidates");
  SD_REQUIRE(!(point_bad || ref_obs || n_obs) || (cap_points >= 0 && (size_t)cap_points >= P), SD_ERR_CAPACITY,
             "cap_points smaller than the number of points");
  SD_REQUIRE(!obs_dead || (cap_obs >= 0 && (size_t)cap_obs >= E), SD_ERR_CAPACITY, "cap_obs smaller than the number of observations");
  hipStream_t s = h->cur->stream;
  if (C) SD_TRY(download(verdict, cu.verdict, 0, C, 1, s));
  if (C) SD_TRY(download(counts2, cu.counts2, 0, C, 2, s));
  if (E) SD_TRY(download(obs_dead, cu.dead, 0, E, 1, s));
  if (P) SD_TRY(download(point_bad, cu.pbad, 0, P, 1, s));
  if (P) SD_TRY(download(ref_obs, cu.ref_new, 0, P, 1, s));
  if (P) SD_TRY(download(n_obs, cu.nobs, 0, P, 1, s));
  SD_TRY(download(info8, cu.info, 0, 8, 1, s));
  return wait_for(s);
}

int sd_track_erase_observations(sd_track* h, int source) {
  SD_REQUIRE(h, SD_ERR_INVALID_ARG, "handle is NULL");
  SD_REQUIRE(source == SD_ERASE_LOCAL_BA || source == SD_ERASE_CULL, SD_ERR_INVALID_ARG, "source must be SD_ERASE_LOCAL_BA or SD_ERASE_CULL");
  SD_TRY(check_resident(h));
  RefreshBuffers& rf = h->rf;
  CullBuffers& cu = h->cu;
  if (source == SD_ERASE_LOCAL_BA)
    SD_REQUIRE(h->ba.ran_points >= 0 && !h->ba.ran_global && h->ba_serial == rf.serial && h->ba.ran_obs == rf.n_obs, SD_ERR_INVALID_ARG,
               "sd_track_local_ba has not run on the observation lists as they stand");
  else
    SD_REQUIRE(cu.ran_cand >= 0 && cu.ran_serial == rf.serial, SD_ERR_INVALID_ARG, kNoCull);
  SD_HIP_CHECK(hipSetDevice(h->device));
  END_RESULTS(h, "sd_track_erase_observations");
  cu.er_points = -1;
  EraseArgs a{};
  a.off = (const int32_t*)(rf.obs + rf.o_off);
  a.ref_obs = (const int32_t*)(rf.obs + rf.o_ref);
  a.point_bad = rf.o_pbad ? rf.obs + rf.o_pbad : nullptr;
  a.frame = (const int32_t*)(rf.obs + rf.o_frame);
  a.kp = (const int32_t*)(rf.obs + rf.o_kp);
  a.kf_bad = rf.o_kbad ? rf.obs + rf.o_kbad : nullptr;
  // The weights are k_cull_gather's, which gives an entry it cannot locate (frame -2, a bad index) weight 1 whatever its mvuRight
  // is.  That cannot reach a result: local BA and the cull both refuse lists in which a point that is not bad has such an entry, a
  // refused bundle adjustment leaves obs_erase clear and a refused cull is gated below, so no point with such an entry has a
  // killed entry, and only points with a killed entry have their nObs looked at.
  a.e_w = cu.e_w;
  a.kill = source == SD_ERASE_LOCAL_BA ? h->ba.erase : cu.dead;
  a.gate = source == SD_ERASE_LOCAL_BA ? nullptr : cu.info;   // a refused bundle adjustment leaves obs_erase clear, a refused cull writes nothing
  a.n_points = rf.n_points;
  a.n_obs = rf.n_obs;
  a.off_new = (int32_t*)(rf.twin + rf.o_off);
  a.ref_new = (int32_t*)(rf.twin + rf.o_ref);
  a.pbad_new = rf.twin + rf.at_pbad;
  a.frame_new = (int32_t*)(rf.twin + rf.o_frame);
  a.kp_new = (int32_t*)(rf.twin + rf.o_kp);
  a.kbad_new = rf.twin + rf.at_kbad;
  a.map = cu.er_map; a.nobs = cu.er_nobs; a.cnt = cu.er_cnt; a.info = cu.er_info;
  SD_TRY(run_stage(h, true, false, STAGE_NONE, [&](hipStream_t s) {
    SD_TRY(queue_gather(h, s));
    return launch_erase(a, s);
  }));
  // The twin is the block now.  n_obs stays what the block was packed for: the lists end at obs_off[n_points], which only the
  // device knows; the kernels that walk entries by number read the end there (k_ba_gather clears its per-edge flags behind it,
  // k_refresh_points bounds a list by it), and the record of the bundle adjustment that asked for the erasure stays whole.
  std::swap(rf.obs, rf.twin);
  rf.o_pbad = rf.at_pbad;
  rf.serial++;
  cu.er_points = rf.n_points;
  cu.er_obs = rf.n_obs;
  cu.er_serial = rf.serial;
  return SD_OK;
}

int sd_track_get_erased(sd_track* h, int32_t* obs_off_new, int32_t* obs_map, uint8_t* point_bad, int32_t* ref_obs, int32_t* n_obs,
                        int32_t* info8, int cap_points, int cap_obs) {
  TRACK_RANGE(h, 0, 1);
  const CullBuffers& cu = h->cu;
  const RefreshBuffers& rf = h->rf;
  SD_REQUIRE(cu.er_points >= 0 && cu.er_serial == rf.serial, SD_ERR_INVALID_ARG, kNoErase);
  const size_t P = (size_t)cu.er_points, E = (size_t)cu.er_obs;
  SD_REQUIRE(!(obs_off_new || point_bad || ref_obs || n_obs) || (cap_points >= 0 && (size_t)cap_points >= P), SD_ERR_CAPACITY,
             "cap_points smaller than the number of points");
  SD_REQUIRE(!obs_map || (cap_obs >= 0 && (size_t)cap_obs >= E), SD_ERR_CAPACITY, "cap_obs smaller than the number of observations");
  hipStream_t s = h->cur->stream;
  SD_TRY(download(obs_off_new, (const int32_t*)(rf.obs + rf.o_off), 0, P + 1, 1, s));
  if (E) SD_TRY(download(obs_map, cu.er_map, 0, E, 1, s));
  if (P) SD_TRY(download(point_bad, (const uint8_t*)(rf.obs + rf.o_pbad), 0, P, 1, s));
  if (P) SD_TRY(download(ref_obs, (const int32_t*)(rf.obs + rf.o_ref), 0, P, 1, s));
  if (P) SD_TRY(download(n_obs, cu.er_nobs, 0, P, 1, s));
  SD_TRY(download(info8, cu.er_info, 0, 8, 1, s));
  return wait_for(s);
}

int sd_debug_cull_keyframes(int n_points, const int32_t* obs_off, const int32_t* obs_kf, const int32_t* obs_octave,
                            const uint8_t* obs_stereo, const float* obs_depth, const int32_t* ref_obs, const uint8_t* point_bad,
                            int n_kf, int n_cand, const int32_t* cand_kf, const uint8_t* cand_flags, int monocular, float th_depth,
                            uint8_t* verdict, int32_t* counts2, uint8_t* obs_dead, uint8_t* point_bad_out, int32_t* ref_obs_out,
                            int32_t* n_obs, int32_t* info8) {
  int total = 0;
  SD_TRY(check_csr(n_points, obs_off, &total));
  SD_REQUIRE((total == 0 || (obs_kf && obs_octave && obs_stereo && obs_depth && obs_dead)) &&
                 (n_points == 0 || (ref_obs && point_bad_out && ref_obs_out && n_obs)) && info8,
             SD_ERR_INVALID_ARG, "NULL array");
  SD_REQUIRE(n_kf >= 1 && n_cand >= 0 && n_cand <= n_kf && (n_cand == 0 || (cand_kf && cand_flags && verdict && counts2)), SD_ERR_INVALID_ARG,
             "bad keyframe or candidate count, or NULL candidate array");
  SD_REQUIRE(monocular == 0 || monocular == 1, SD_ERR_INVALID_ARG, "monocular must be 0 or 1");
  std::vector<uint8_t> named((size_t)n_kf, 0);
  for (int c = 0; c < n_cand; c++) {
    SD_REQUIRE(cand_kf[c] >= 0 && cand_kf[c] < n_kf, SD_ERR_INVALID_ARG, "candidate outside [0, n_kf)");
    SD_REQUIRE(!named[cand_kf[c]], SD_ERR_INVALID_ARG, "a candidate is named twice");
    named[cand_kf[c]] = 1;
  }
  // per point the refusal bits: obs_kf -2 is not resident, -1 the current keyframe, anything else outside [0, n_kf) a bad index
  const size_t P = (size_t)std::max(n_points, 1), E = (size_t)std::max(total, 1), C = (size_t)std::max(n_cand, 1);
  std::vector<uint8_t> p_flag(P, 0), w(E, 1);
  std::vector<int32_t> kf(E, 0), cand(2 * C, 0);
  for (int p = 0; p < n_points; p++)
    for (int e = obs_off[p]; e < obs_off[p + 1]; e++) {
      const int k = obs_kf[e];
      kf[e] = k == -1 ? n_kf : k;
      w[e] = obs_stereo[e] ? 2 : 1;
      if (point_bad && point_bad[p]) continue;
      if (k == -2) p_flag[p] |= SD_CULL_NOT_RESIDENT;
      else if (k < -2 || k >= n_kf) p_flag[p] |= SD_CULL_BAD_INDEX;
    }
  for (int c = 0; c < n_cand; c++) { cand[c] = cand_kf[c]; cand[(size_t)n_cand + c] = cand_flags[c]; }
  Blob b;
  const size_t o_off = b.reserve(P + 1, obs_off, (size_t)n_points + 1), o_ref = b.reserve(P, ref_obs, (size_t)n_points);
  const size_t o_pb = b.reserve(P, point_bad, point_bad ? (size_t)n_points : 0), o_kf = b.reserve(E, kf.data(), E);
  const size_t o_oc = b.reserve(E, obs_octave, (size_t)total), o_d = b.reserve(E, obs_depth, (size_t)total), o_w = b.reserve(E, w.data(), E);
  const size_t o_pf = b.reserve(P, p_flag.data(), P), o_c = b.reserve(2 * C, cand.data(), 2 * C);
  // the outputs start as the caller's arrays: a refusal writes info8 alone
  const size_t r_v = b.reserve(C, verdict, (size_t)n_cand), r_c2 = b.reserve(2 * C, counts2, 2 * (size_t)n_cand);
  const size_t r_dead = b.reserve(E, obs_dead, (size_t)total), r_pb = b.reserve(P, point_bad_out, (size_t)n_points);
  const size_t r_ref = b.reserve(P, ref_obs_out, (size_t)n_points), r_n = b.reserve(P, n_obs, (size_t)n_points);
  const size_t r_info = b.reserve(8, info8, 8);
  SD_TRY(b.run("sd_debug_cull_keyframes", [&] {
    CullArgs a{};
    a.l.off = b.dev<int32_t>(o_off); a.l.ref_obs = b.dev<int32_t>(o_ref); a.l.point_bad = point_bad ? b.dev<uint8_t>(o_pb) : nullptr;
    a.l.n_points = n_points;
    a.l.e_kf = b.dev<int32_t>(o_kf); a.l.e_oct = b.dev<int32_t>(o_oc); a.l.e_depth = b.dev<float>(o_d); a.l.e_w = b.dev<uint8_t>(o_w);
    a.l.p_flag = b.dev<uint8_t>(o_pf);
    a.cand = b.dev<int32_t>(o_c); a.n_cand = n_cand; a.monocular = monocular; a.th_depth = th_depth;
    a.verdict = b.dev<uint8_t>(r_v); a.counts2 = b.dev<int32_t>(r_c2); a.dead = b.dev<uint8_t>(r_dead); a.pbad = b.dev<uint8_t>(r_pb);
    a.ref_new = b.dev<int32_t>(r_ref); a.nobs = b.dev<int32_t>(r_n); a.info = b.dev<int32_t>(r_info);
    SD_TRY(launch_cull(a, 0));
    SD_HIP_CHECK(hipDeviceSynchronize());
    return SD_OK;
  }));
  b.take(verdict, r_v, (size_t)n_cand);
  b.take(counts2, r_c2, 8 * (size_t)n_cand);
  b.take(obs_dead, r_dead, (size_t)total);
  b.take(point_bad_out, r_pb, (size_t)n_points);
  b.take(ref_obs_out, r_ref, 4 * (size_t)n_points);
  b.take(n_obs, r_n, 4 * (size_t)n_points);
  b.take(info8, r_info, 32);
  return SD_OK;
}

int sd_debug_erase_observations(int n_points, const int32_t* obs_off, const uint8_t* obs_stereo, const uint8_t* obs_erase,
                                const int32_t* ref_obs, const uint8_t* point_bad, int32_t* obs_off_new, int32_t* obs_map,
                                uint8_t* point_bad_out, int32_t* ref_obs_out, int32_t* n_obs, int32_t* info8) {
  int total = 0;
  SD_TRY(check_csr(n_points, obs_off, &total));
  SD_REQUIRE((total == 0 || (obs_stereo && obs_erase && obs_map)) && (n_points == 0 || (ref_obs && point_bad_out && ref_obs_out && n_obs)) &&
                 obs_off_new && info8,
             SD_ERR_INVALID_ARG, "NULL array");
  const size_t P = (size_t)std::max(n_points, 1), E = (size_t)std::max(total, 1);
  std::vector<uint8_t> w(E, 1);
  for (int e = 0; e < total; e++) w[e] = obs_stereo[e] ? 2 : 1;
  Blob b;
  const size_t o_off = b.reserve(P + 1, obs_off, (size_t)n_points + 1), o_ref = b.reserve(P, ref_obs, (size_t)n_points);
  const size_t o_pb = b.reserve(P, point_bad, point_bad ? (size_t)n_points : 0), o_w = b.reserve(E, w.data(), E);
  const size_t o_k = b.reserve(E, obs_erase, (size_t)total), o_cnt = b.reserve<int32_t>(P);
  const size_t r_off = b.reserve<int32_t>(P + 1), r_map = b.reserve<int32_t>(E), r_pb = b.reserve<uint8_t>(P), r_ref = b.reserve<int32_t>(P);
  const size_t r_n = b.reserve<int32_t>(P), r_info = b.reserve<int32_t>(8);
  SD_TRY(b.run("sd_debug_erase_observations", [&] {
    EraseArgs a{};
    a.off = b.dev<int32_t>(o_off); a.ref_obs = b.dev<int32_t>(o_ref); a.point_bad = point_bad ? b.dev<uint8_t>(o_pb) : nullptr;
    a.e_w = b.dev<uint8_t>(o_w); a.kill = b.dev<uint8_t>(o_k);
    a.n_points = n_points; a.n_obs = total;
    a.off_new = b.dev<int32_t>(r_off); a.ref_new = b.dev<int32_t>(r_ref); a.pbad_new = b.dev<uint8_t>(r_pb);
    a.map = b.dev<int32_t>(r_map); a.nobs = b.dev<int32_t>(r_n); a.cnt = b.dev<int32_t>(o_cnt); a.info = b.dev<int32_t>(r_info);
    SD_TRY(launch_erase(a, 0));
    SD_HIP_CHECK(hipDeviceSynchronize());
    return SD_OK;
  }));
  b.take(obs_off_new, r_off, 4 * ((size_t)n_points + 1));
  b.take(obs_map, r_map, 4 * (size_t)total);
  b.take(point_bad_out, r_pb, (size_t)n_points);
  b.take(ref_obs_out, r_ref, 4 * (size_t)n_points);
  b.take(n_obs, r_n, 4 * (size_t)n_points);
  b.take(info8, r_info, 32);
  return SD_OK;
}

}  // extern "C"
