// The new map points of LocalMapping::CreateNewMapPoints become local-map rows on the device: what stands between
// sd_track_triangulate (track_newpoints_tri.hip), whose points live in TriangBuffers, and sd_track_fuse / sd_track_match_local /
// sd_track_refresh_points, which read the lm_* rows of sd_track_set_local (reference src/LocalMapping.cc:401-417 makes the point,
// :440-461 SearchInNeighbors hands mpCurrentKeyFrame's points to Fuse; MapPoint::AddObservation src/MapPoint.cc:98-108).
//
// k_append_points, one lane per point g = 0 .. info[0] - 1 of the live k_new_points_resolve result, in creation order.  The point
// goes to position p = base + j of row r:
//   row mode (point_row = r >= 0): j = g, base = lm_n[r]; cand[f][p] = f != slot_g for every f < n_cand_rows -- the point is in
//     its own neighbour's keyframe (IsInKeyFrame), in no other Fuse target; targets beyond the triangulation's slots get 1.
//   paired mode (point_row = -1): r = slot_g, j = g - (points of the slots before it: the prefix sum of count[b][1]),
//     base = lm_n[r]; cand[r][p] = 1.
//   Xw, normal from geo; mf_max_dist = dist.x; max_dist = 1.2f * dist.x, min_dist = 0.8f * dist.y (one float product each: what
//     callers of sd_track_set_local compute and k_refresh_points writes); desc as two 16-byte stores;
//   obs = nObs after the two AddObservation calls: (mvuRight1[kp1] >= 0 ? 2 : 1) + (mvuRight2[slot][idx2] >= 0 ? 2 : 1), from
//     the rows the triangulation read (KF1's is the row of the cur FRAME: the broadcast frame, or frame slot_g).
//   j >= max_points - base: the point is dropped -- nothing at or beyond max_points is addressed.  kp_claimed is not touched.
//   mark_flags: AddMapPoint on both keyframes, as the "holds a map point" flags of sd_track_set_point_flags -- sp_valid2[slot][idx2],
//     and sp_valid1 at kp1 in the row of every slot that stands for KF1: row slot_g when paired, rows 0 .. info[2] - 1 under the
//     broadcast (each slot's search read its own row of the one keyframe).  Appended points only.
// Every lane reads lm_n[r] and none writes it.  k_append_commit, one workgroup queued behind it, one lane per row: lm_n[r] += appended
// and result[r] = base | appended | dropped (rows that received nothing: their lm_n | 0 | 0).  No atomics.
#include <hip/hip_runtime.h>

#include <string>

#include "track_handle.h"

namespace sd {

#define APPEND_THREADS 256

struct AppendArgs {
  // the new points (TriangBuffers)
  const int32_t *info, *count, *pt;
  const double* geo;
  const float* dist;
  const uint8_t* desc;
  const float *ur1, *ur2;   // [.][cap] mvuRight of the cur frames / of the ref frames
  // the local-map rows, max_points entries each
  int32_t* lm_n;
  uint8_t* cand;
  double *Xw, *normal;
  float *dmin, *dmax, *mfmax;
  uint8_t* pdesc;
  int32_t* obs;
  uint8_t *has1, *has2;     // [B][cap] sd_track_set_point_flags
  int32_t* result;          // [B][3]
  int cap, max_points, max_batch, point_row, n_cand_rows, mark_flags;
};

// Points the resolve result holds, and those of slot b (paired)
__device__ __forceinline__ int append_total(const AppendArgs& a) { return min(max(a.info[0], 0), a.max_batch * a.cap); }
__device__ __forceinline__ int append_slots(const AppendArgs& a) { return min(max(a.info[2], 0), a.max_batch); }
__device__ __forceinline__ int append_base(const AppendArgs& a, int row) { return min(max(a.lm_n[row], 0), a.max_points); }

__global__ __launch_bounds__(APPEND_THREADS) void k_append_points(AppendArgs a) {
  const int g = blockIdx.x * APPEND_THREADS + threadIdx.x;
  if (g >= append_total(a)) return;
  const int B = a.max_batch, cap = a.cap, M = a.max_points;
  const int4 q = ((const int4*)a.pt)[g];   // KF1 keypoint | slot | KF2 keypoint | id
  const int kp1 = q.x, slot = q.y, idx2 = q.z;
  if (slot < 0 || slot >= B || kp1 < 0 || kp1 >= cap || idx2 < 0 || idx2 >= cap) return;   // (the resolve writes none such)
  int row = a.point_row, j = g;
  if (row < 0) {
    row = slot;
    for (int b = 0; b < slot; b++) j -= a.count[(size_t)b * 2 + 1];
  }
  const int base = append_base(a, row);
  if (j < 0 || j >= M - base) return;   // dropped: the row is full
  const int i = base + j;               // < M
  const size_t p = (size_t)row * M + i;
  for (int k = 0; k < 3; k++) {
    a.Xw[p * 3 + k] = a.geo[(size_t)g * 6 + k];
    a.normal[p * 3 + k] = a.geo[(size_t)g * 6 + 3 + k];
  }
  const float2 d = ((const float2*)a.dist)[g];
  a.mfmax[p] = d.x;
  a.dmax[p] = __fmul_rn(1.2f, d.x);
  a.dmin[p] = __fmul_rn(0.8f, d.y);
  const uint4* ds = (const uint4*)(a.desc + (size_t)g * 32);
  ((uint4*)(a.pdesc + p * 32))[0] = ds[0];
  ((uint4*)(a.pdesc + p * 32))[1] = ds[1];
  const int bc = a.info[1];
  const int fc = bc >= 0 ? min(bc, B - 1) : slot;
  a.obs[p] = (a.ur1[(size_t)fc * cap + kp1] >= 0 ? 2 : 1) + (a.ur2[(size_t)slot * cap + idx2] >= 0 ? 2 : 1);
  if (a.point_row >= 0) {
    for (int f = 0; f < a.n_cand_rows; f++) a.cand[(size_t)f * M + i] = f != slot;
  } else {
    a.cand[p] = 1;
  }
  if (a.mark_flags) {
    a.has2[(size_t)slot * cap + idx2] = 1;
    if (bc >= 0) {
      const int n = append_slots(a);
      for (int f = 0; f < n; f++) a.has1[(size_t)f * cap + kp1] = 1;
    } else {
      a.has1[(size_t)slot * cap + kp1] = 1;
    }
  }
}

__global__ __launch_bounds__(64) void k_append_commit(AppendArgs a) {
  const int n = append_slots(a);
  for (int row = threadIdx.x; row < a.max_batch; row += 64) {
    int arriving = 0;
    if (a.point_row >= 0) arriving = row == a.point_row ? append_total(a) : 0;
    else if (row < n) arriving = max(a.count[(size_t)row * 2 + 1], 0);
    const int base = append_base(a, row);
    const int appended = min(arriving, a.max_points - base);
    a.result[(size_t)row * 3] = base;
    a.result[(size_t)row * 3 + 1] = appended;
    a.result[(size_t)row * 3 + 2] = arriving - appended;
    if (appended > 0) a.lm_n[row] = base + appended;
  }
}

int launch_append_points(const TrackBuffers& tb, const TriangBuffers& nb, int max_batch, int point_row, int n_cand_rows, int mark_flags,
                         hipStream_t s) {
  AppendArgs a = {nb.info, nb.count, nb.pt, nb.geo, nb.dist, nb.desc, tb.uright, tb.uright_ref, tb.lm_n, tb.lm_cand, tb.lm_Xw,
                  tb.lm_normal, tb.lm_min, tb.lm_max, tb.lm_mfmax, tb.lm_desc, tb.lm_obs, tb.sp_valid1, tb.sp_valid2, nb.appended,
                  tb.kp_cap, tb.max_points, max_batch, point_row, n_cand_rows, mark_flags};
  // the number of points is on the device: one lane per row of the point list, the lanes beyond info[0] leave at once
  const int lanes = max_batch * tb.kp_cap;
  hipLaunchKernelGGL(k_append_points, dim3((lanes + APPEND_THREADS - 1) / APPEND_THREADS), dim3(APPEND_THREADS), 0, s, a);
  SD_HIP_CHECK(hipGetLastError());
  hipLaunchKernelGGL(k_append_commit, dim3(1), dim3(64), 0, s, a);
  SD_HIP_CHECK(hipGetLastError());
  return SD_OK;
}

}  // namespace sd

using namespace sd;

extern "C" {

int sd_track_append_new_points(sd_track* h, int point_row, int n_cand_rows, int mark_flags) {
  SD_REQUIRE(h, SD_ERR_INVALID_ARG, "handle is NULL");
  SD_REQUIRE(point_row >= -1 && point_row < h->max_batch, SD_ERR_INVALID_ARG, "point_row outside [-1, max_batch)");
  SD_REQUIRE(n_cand_rows >= 0 && n_cand_rows <= h->max_batch, SD_ERR_INVALID_ARG, "n_cand_rows outside [0, max_batch]");
  SD_REQUIRE(mark_flags == 0 || mark_flags == 1, SD_ERR_INVALID_ARG, "mark_flags must be 0 or 1");
  SD_REQUIRE(h->res.triang_live(h->res.triang.n, inputs_now(h)), SD_ERR_INVALID_ARG,
             "no live result of sd_track_triangulate (it has not run, or the search's result, mvDepth, the median depths or the camera "
             "were replaced since)");
  SD_REQUIRE(h->res.triang.payload == 0, SD_ERR_INVALID_ARG,
             "the points of this sd_track_triangulate result have been appended already (a second append would duplicate them)");
  SD_REQUIRE(point_row >= 0 || h->tb.cur_bcast < 0, SD_ERR_INVALID_ARG,
             "point_row = -1 needs a paired result: under the broadcast every point belongs to the one current keyframe's row");
  SD_HIP_CHECK(hipSetDevice(h->device));
  const int n_slots = h->res.triang.n;
  if (mark_flags) END_RESULTS(h, "sd_track_append_new_points(mark_flags)");   // (the search's result and its triangulation among them)
  else END_RESULTS(h, "sd_track_append_new_points");
  h->res.triang.payload = 1;
  // the kernels read the extractors' frames not at all, only buffers of this handle: queued behind the triangulation, no marks
  SD_TRY(launch_append_points(h->tb, h->nb, h->max_batch, point_row, n_cand_rows, mark_flags, h->pnp_stream));
  h->res.append.set(h->max_batch, BIND_APPEND, inputs_now(h), n_slots);
  return SD_OK;
}

int sd_track_get_appended(sd_track* h, int frame0, int n_rows, int32_t* base, int32_t* appended, int32_t* dropped) {
  TRACK_RANGE(h, frame0, n_rows);
  SD_REQUIRE(h->res.append.live(frame0 + n_rows, inputs_now(h)), SD_ERR_INVALID_ARG,
             "sd_track_append_new_points has not run (or sd_track_set_local / _set_local_view, a write-through refresh or a new "
             "triangulation came since)");
  hipStream_t s = h->cur->stream;
  const int32_t* src = h->nb.appended + (size_t)frame0 * 3;
  if (base) SD_HIP_CHECK(hipMemcpy2DAsync(base, 4, src, 12, 4, n_rows, hipMemcpyDeviceToHost, s));
  if (appended) SD_HIP_CHECK(hipMemcpy2DAsync(appended, 4, src + 1, 12, 4, n_rows, hipMemcpyDeviceToHost, s));
  if (dropped) SD_HIP_CHECK(hipMemcpy2DAsync(dropped, 4, src + 2, 12, 4, n_rows, hipMemcpyDeviceToHost, s));
  return wait_for(s);
}

int sd_track_get_local_points(sd_track* h, int row, int32_t* n_local, uint8_t* cand, double* Xw, double* normal, float* min_dist,
                              float* max_dist, float* mf_max_dist, uint8_t* desc, int32_t* obs, int cap) {
  TRACK_RANGE(h, row, 1);
  SD_REQUIRE(!(cand || Xw || normal || min_dist || max_dist || mf_max_dist || desc || obs) || cap >= h->max_points, SD_ERR_CAPACITY,
             "cap smaller than max_points");
  hipStream_t s = h->cur->stream;
  const size_t M = h->max_points, o = (size_t)row;
  const TrackBuffers& tb = h->tb;
  SD_TRY(download(n_local, tb.lm_n, o, 1, 1, s));
  SD_TRY(download(cand, tb.lm_cand, o, 1, M, s));
  SD_TRY(download(Xw, tb.lm_Xw, o, 1, M * 3, s));
  SD_TRY(download(normal, tb.lm_normal, o, 1, M * 3, s));
  SD_TRY(download(min_dist, tb.lm_min, o, 1, M, s));
  SD_TRY(download(max_dist, tb.lm_max, o, 1, M, s));
  SD_TRY(download(mf_max_dist, tb.lm_mfmax, o, 1, M, s));
  SD_TRY(download(desc, tb.lm_desc, o, 1, M * 32, s));
  SD_TRY(download(obs, tb.lm_obs, o, 1, M, s));
  return wait_for(s);
}

}  // extern "C"
