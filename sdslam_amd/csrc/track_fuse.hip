// ORBmatcher::Fuse, both overloads, on MI355X: the search for the keypoint a map point duplicates in a keyframe
//   Fuse(KeyFrame* pKF, const vector<MapPoint*>& vpMapPoints, th)                       reference src/ORBmatcher.cc:477-615
//   Fuse(KeyFrame* pKF, const Eigen::Matrix4d& Scw, vpPoints, th, vpReplacePoint)       src/ORBmatcher.cc:617-732
//   KeyFrame::GetFeaturesInArea / IsInImage                                             src/KeyFrame.cc:529-570
//   MapPoint::PredictScale(dist, KeyFrame*)                                             src/MapPoint.cc:355-369
// callers LocalMapping::SearchInNeighbors (src/LocalMapping.cc:422-492) and LoopClosing::SearchAndFuse (src/LoopClosing.cc:535-560).
//
// The device does the search (:493-594, :639-715): for keyframe KF and map point i, best_idx[i] = the keypoint the reference reaches
// :597 / :718 with when bestDist <= TH_LOW (50), else -1, and best_dist[i] = bestDist as the candidate loop leaves it (256: no
// candidate passed the gates; both overloads, although the Sim3 one starts from INT_MAX).  The search reads the point's position,
// normal, mfMaxDistance, min / max distance invariance and descriptor, and the keyframe's keypoints, descriptors, mvuRight, pose and
// K.  NOTHING in it reads mutable map state -- no observations, no mvpMapPoints, no result of another point or keyframe -- so any
// number of (keyframe, point list) pairs may be searched in one launch.  What the reference does with the result (Replace,
// AddObservation, AddMapPoint: :597-611, :718-728) stays with the caller, who walks the results in order (include/sdslam/sdslam.hpp).
//
// One workgroup per slot = one keyframe.  The keyframe's 64 x 48 bucket grid is built as in k_match_local (grid_key,
// grid_sort_and_starts); KeyFrame::GetFeaturesInArea is Frame's without the level arguments.  A group of FUSE_GL lanes takes one
// point: every lane evaluates the gates (uniform over the group), the group walks the window ONCE, a lane per grid entry, and takes
// min(dist << 22 | order-in-vIndices << 11 | idx) -- "smallest distance, first in vIndices order", which is what the strict `<` of
// :590 / :711 keeps.  No candidate list, no second best, no claims, no serial phase.
//
// Gates, in the reference's order and widths (the library is built with -ffp-contract=off; the float steps are spelled out):
//   p3Dc = (R[r][0] * X + R[r][1] * Y + R[r][2] * Z) + t[r] in double, left to right; reject p3Dc.z < 0
//   invz = (float)(1.0 / p3Dc.z); x = (float)(p3Dc.x * (double)invz), y likewise; u = fx * x + cx, v = fy * y + cy in float
//   KeyFrame::IsInImage: u >= mnMinX && u < mnMaxX && v >= mnMinY && v < mnMaxY   (NOT isInFrustum's u < min || u > max)
//   PO = p3Dw - Ow; dist3D = (float)sqrt((PO.x^2 + PO.y^2) + PO.z^2); reject dist3D < minDistance || dist3D > maxDistance
//   reject (PO.x * n.x + PO.y * n.y) + PO.z * n.z < 0.5 * (double)dist3D, in double
//   nPredictedLevel through the PredictScale breakpoints scale_thr (see k_match_local); radius = th * mvScaleFactors[level]
//   per keypoint of the window (|kp.x - u| < radius && |kp.y - v| < radius): octave in [level - 1, level]; SE3 overload only:
//     ex = u - kp.x, ey = v - kp.y; mvuRight[idx] >= 0 (0 counts as stereo): er = (u - bf * invz) - mvuRight[idx],
//     e2 = (ex * ex + ey * ey) + er * er, reject (double)(e2 * mvInvLevelSigma2[octave]) > 7.8; else e2 = ex * ex + ey * ey, > 5.99
// Pose, one thread per slot, every product and sum rounded on its own (T column-major, M[r][c] = T[c * 4 + r]):
//   SE3:  Rcw = M[0..2][0..2], tcw = M[0..2][3]
//   Sim3 (:625-629): scw = (float)sqrt((M[0][0] * M[0][0] + M[0][1] * M[0][1]) + M[0][2] * M[0][2]);
//         Rcw[r][c] = M[r][c] / (double)scw; tcw[r] = M[r][3] / (double)scw
//   both: Ow[c] = ((-Rcw[0][c]) * tcw[0] + (-Rcw[1][c]) * tcw[1]) + (-Rcw[2][c]) * tcw[2]     (-Rcw^T * tcw)
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "track_handle.h"
#include "track_match_dev.h"

namespace sd {

#define FUSE_WAVES 8
#ifndef FUSE_GL
#define FUSE_GL 8          // lanes per point: a window column's run of the sorted grid holds 3.4 keypoints on average, 9 at the
                           // 90th percentile; 4 and 16 lanes measured beside it
#endif
#define FUSE_TH_LOW 50
#define FUSE_NONE 0x7FFFFFFFu

struct FuseArgs {
  // the keyframes: rows of `cap` entries per frame of the extractor on the side in use
  const sd_keypoint* kps;
  const uint8_t* desc;
  const int32_t* nkp;
  const float* uright;
  const double* T;          // [B][16] column-major: Tcw (SE3) or Scw (Sim3)
  // the points: rows of max_points entries (the local-map buffers of sd_track_set_local)
  const int32_t* n_pts;
  const uint8_t* cand;
  const double* Xw;
  const double* normal;
  const float* dmin;
  const float* dmax;
  const float* mfmax;
  const uint8_t* pdesc;
  const float* sf;          // [nlevels] mvScaleFactors
  const float* inv_sigma2;  // [nlevels] mvInvLevelSigma2
  const float* scale_thr;   // [nlevels] PredictScale breakpoints
  int32_t* best_idx;        // [B][max_points]
  int32_t* best_dist;       // [B][max_points]
  int32_t* n_found;         // [B]
  double* pose;             // [B][15]
  int kf_bcast;             // >= 0: every slot's keyframe is THIS frame of the extractor; -1: frame f
  int point_row;            // >= 0: every slot reads the points of THIS row (cand stays per slot); -1: row f
  int cap, max_points, nlevels, KP2, sim3;
  float th;
};

// One point against the keyframe's grid: this lane's minimum key over the entries it visits (FUSE_NONE: none).  All lanes of the
// group call with the same point.
template <int GL>
__device__ __forceinline__ uint32_t fuse_point(const FuseArgs& a, const TrackCam& cam, const double* __restrict__ P /* Rcw | tcw | Ow */,
                                               int row, int i, const sd_keypoint* __restrict__ kps, const uint8_t* __restrict__ desc,
                                               const float* __restrict__ uright, const uint32_t* s_key, const uint16_t* s_cstart,
                                               float invW, float invH, int glane) {
  const size_t pi = (size_t)row * a.max_points + i;
  const double X0 = a.Xw[pi * 3], X1 = a.Xw[pi * 3 + 1], X2 = a.Xw[pi * 3 + 2];
  const double pz = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(P[6], X0), __dmul_rn(P[7], X1)), __dmul_rn(P[8], X2)), P[11]);
  if (pz < 0.0) return FUSE_NONE;
  const double px = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(P[0], X0), __dmul_rn(P[1], X1)), __dmul_rn(P[2], X2)), P[9]);
  const double py = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(P[3], X0), __dmul_rn(P[4], X1)), __dmul_rn(P[5], X2)), P[10]);
  const float invz = (float)__ddiv_rn(1.0, pz);
  const float x = (float)__dmul_rn(px, (double)invz), y = (float)__dmul_rn(py, (double)invz);
  const float u = __fadd_rn(__fmul_rn(cam.ffx, x), cam.fcx), v = __fadd_rn(__fmul_rn(cam.ffy, y), cam.fcy);
  if (!(u >= cam.min_x && u < cam.max_x && v >= cam.min_y && v < cam.max_y)) return FUSE_NONE;
  const float ur = __fsub_rn(u, __fmul_rn(cam.bf, invz));
  const double PO0 = __dsub_rn(X0, P[12]), PO1 = __dsub_rn(X1, P[13]), PO2 = __dsub_rn(X2, P[14]);
  const float dist3D = (float)sqrt(__dadd_rn(__dadd_rn(__dmul_rn(PO0, PO0), __dmul_rn(PO1, PO1)), __dmul_rn(PO2, PO2)));
  if (dist3D < a.dmin[pi] || dist3D > a.dmax[pi]) return FUSE_NONE;
  const double pn = __dadd_rn(__dadd_rn(__dmul_rn(PO0, a.normal[pi * 3]), __dmul_rn(PO1, a.normal[pi * 3 + 1])), __dmul_rn(PO2, a.normal[pi * 3 + 2]));
  if (pn < __dmul_rn(0.5, (double)dist3D)) return FUSE_NONE;
  const float ratio = __fdiv_rn(a.mfmax[pi], dist3D);
  int lvl = 0;
  for (int n = 1; n < a.nlevels; n++) lvl += (ratio >= a.scale_thr[n]) ? 1 : 0;   // PredictScale
  const float radius = __fmul_rn(a.th, a.sf[lvl]);

  // KeyFrame::GetFeaturesInArea(u, v, radius)
  const int nMinCellX = max(0, (int)floorf((u - cam.min_x - radius) * invW));
  if (nMinCellX >= GRID_COLS) return FUSE_NONE;
  const int nMaxCellX = min(GRID_COLS - 1, (int)ceilf((u - cam.min_x + radius) * invW));
  if (nMaxCellX < 0) return FUSE_NONE;
  const int nMinCellY = max(0, (int)floorf((v - cam.min_y - radius) * invH));
  if (nMinCellY >= GRID_ROWS) return FUSE_NONE;
  const int nMaxCellY = min(GRID_ROWS - 1, (int)ceilf((v - cam.min_y + radius) * invH));
  if (nMaxCellY < 0) return FUSE_NONE;
  const unsigned long long* dm = (const unsigned long long*)(a.pdesc + pi * 32);
  const unsigned long long d0 = dm[0], d1 = dm[1], d2 = dm[2], d3 = dm[3];
  uint32_t best = FUSE_NONE;
  int seq0 = 0;
  for (int ix = nMinCellX; ix <= nMaxCellX; ix++) {
    const int ca = s_cstart[ix * GRID_ROWS + nMinCellY], cb = s_cstart[ix * GRID_ROWS + nMaxCellY + 1];
    for (int e = ca + glane; e < cb; e += GL) {
      const int idx = s_key[e] & 2047;
      // everything a candidate needs is fetched at once, as in match_window
      const float kx = kps[idx].x, ky = kps[idx].y;
      const int koct = kps[idx].octave;
      const float kpr = uright[idx];
      const unsigned long long* dk = (const unsigned long long*)(desc + (size_t)idx * 32);
      const unsigned long long k0 = dk[0], k1 = dk[1], k2 = dk[2], k3 = dk[3];
      if (!(fabsf(kx - u) < radius && fabsf(ky - v) < radius)) continue;   // (rejected entries keep their place in the order: harmless)
      if (koct < lvl - 1 || koct > lvl) continue;
      if (!a.sim3) {
        const float ex = __fsub_rn(u, kx), ey = __fsub_rn(v, ky);
        float e2 = __fadd_rn(__fmul_rn(ex, ex), __fmul_rn(ey, ey));
        double limit = 5.99;
        if (kpr >= 0) {
          const float er = __fsub_rn(ur, kpr);
          e2 = __fadd_rn(e2, __fmul_rn(er, er));
          limit = 7.8;
        }
        if ((double)__fmul_rn(e2, a.inv_sigma2[min(max(koct, 0), a.nlevels - 1)]) > limit) continue;
      }
      const int dist = hamming256(k0, k1, k2, k3, d0, d1, d2, d3);
      best = min(best, ((uint32_t)dist << 22) | ((uint32_t)(seq0 + (e - ca)) << 11) | (uint32_t)idx);
    }
    seq0 += cb - ca;
  }
  return best;
}

// Dynamic LDS: LdsFuse (track_match_lds.h)
__global__ __launch_bounds__(64 * FUSE_WAVES) void k_fuse(FuseArgs a, TrackCam cam) {
  extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
  const LdsFuse L(a.KP2);
  uint32_t* s_key = lds_at<uint32_t>(smem, L.key);
  uint16_t* s_cstart = lds_at<uint16_t>(smem, L.cstart);
  double* s_pose = lds_at<double>(smem, L.pose);
  int* s_nfound = lds_at<int>(smem, L.nfound);
  const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, NT = 64 * FUSE_WAVES;
  const int cap = a.cap, M = a.max_points, KP2 = a.KP2;
  const int fk = a.kf_bcast >= 0 ? a.kf_bcast : f;
  const int row = a.point_row >= 0 ? a.point_row : f;
  const sd_keypoint* kps = a.kps + (size_t)fk * cap;
  const uint8_t* desc = a.desc + (size_t)fk * cap * 32;
  const float* uright = a.uright + (size_t)fk * cap;
  const int N = min(max(a.nkp[fk], 0), min(cap, KP2));
  const int n_pts = min(max(a.n_pts[row], 0), M);
  const uint8_t* cand = a.cand + (size_t)f * M;
  const float invW = (float)GRID_COLS / (float)(cam.max_x - cam.min_x);   // mfGridElementWidthInv
  const float invH = (float)GRID_ROWS / (float)(cam.max_y - cam.min_y);

  for (int i = tid; i < KP2; i += NT) s_key[i] = i < N ? grid_key(kps[i], cam, invW, invH, i) : 0xFFFFFFFFu;
  if (tid == 0) {   // the pose the slot projects with (operation order: the header of this file)
    const double* T = a.T + (size_t)f * 16;
    double R[9], t[3];
    double s = 1.0;
    if (a.sim3) s = (double)(float)sqrt(__dadd_rn(__dadd_rn(__dmul_rn(T[0], T[0]), __dmul_rn(T[4], T[4])), __dmul_rn(T[8], T[8])));
    for (int r = 0; r < 3; r++) {
      for (int c = 0; c < 3; c++) R[r * 3 + c] = a.sim3 ? __ddiv_rn(T[c * 4 + r], s) : T[c * 4 + r];
      t[r] = a.sim3 ? __ddiv_rn(T[12 + r], s) : T[12 + r];
    }
    for (int k = 0; k < 9; k++) s_pose[k] = R[k];
    for (int k = 0; k < 3; k++) {
      s_pose[9 + k] = t[k];
      s_pose[12 + k] = __dadd_rn(__dadd_rn(__dmul_rn(-R[k], t[0]), __dmul_rn(-R[3 + k], t[1])), __dmul_rn(-R[6 + k], t[2]));
    }
    *s_nfound = 0;
  }
  __syncthreads();
  grid_sort_and_starts(s_key, s_cstart, KP2, tid, NT);
  __syncthreads();
  if (tid < 15) a.pose[(size_t)f * 15 + tid] = s_pose[tid];

  constexpr int GL = FUSE_GL, PPW = 64 / GL;
  const SubWave<GL> g(lane);
  int32_t* o_idx = a.best_idx + (size_t)f * M;
  int32_t* o_dist = a.best_dist + (size_t)f * M;
  int found = 0;
  for (int i0 = 0; i0 < M; i0 += PPW * FUSE_WAVES) {   // (to M, not n_pts: the rest of the row reads "none"; i0 is uniform)
    const int i = i0 + PPW * wave + g.group;
    uint32_t best = FUSE_NONE;
    if (i < n_pts && cand[i]) best = fuse_point<GL>(a, cam, s_pose, row, i, kps, desc, uright, s_key, s_cstart, invW, invH, g.glane);
#pragma unroll
    for (int d = GL / 2; d > 0; d >>= 1) best = min(best, (uint32_t)__shfl_xor((int)best, d));   // the groups have reconverged here
    if (g.glane == 0 && i < M) {
      const int dist = best == FUSE_NONE ? 256 : (int)(best >> 22);
      const bool ok = dist <= FUSE_TH_LOW;
      o_idx[i] = ok ? (int32_t)(best & 2047u) : -1;
      o_dist[i] = dist;
      found += ok ? 1 : 0;
    }
  }
  if (found) atomicAdd(s_nfound, found);
  __syncthreads();
  if (tid == 0) a.n_found[f] = *s_nfound;
}

// KP2 = the power of two >= the keypoint capacity that the LDS sort runs on
static int launch_fuse_args(FuseArgs a, const TrackCam& cam, int n_frames, hipStream_t s) {
  a.KP2 = 64;
  while (a.KP2 < a.cap) a.KP2 <<= 1;
  SD_REQUIRE(a.KP2 <= 2048 && a.max_points <= 2048, SD_ERR_CAPACITY, "Fuse supports at most 2048 keypoints / map points per keyframe");
  hipLaunchKernelGGL(k_fuse, dim3(n_frames), dim3(64 * FUSE_WAVES), LdsFuse(a.KP2).bytes, s, a, cam);
  SD_HIP_CHECK(hipGetLastError());
  return SD_OK;
}

int launch_fuse(const sd_orb* cur, const sd_orb* ref, const TrackBuffers& tb, const FuseBuffers& fb, const TrackCam& cam, const float* d_sf,
                const float* d_inv_sigma2, const float* d_scale_thr, int n_frames, int kf_side, int point_row, float th, int sim3,
                hipStream_t s) {
  const sd_orb* kf = kf_side ? ref : cur;
  FuseArgs a{};
  a.kps = keys_un(kf);
  a.desc = kf->d_desc;
  a.nkp = kf->d_nout;
  a.uright = kf_side ? tb.uright_ref : tb.uright;
  a.T = sim3 ? fb.Scw : (kf_side ? tb.Tref : tb.Tcur);
  a.n_pts = tb.lm_n;
  a.cand = tb.lm_cand;
  a.Xw = tb.lm_Xw;
  a.normal = tb.lm_normal;
  a.dmin = tb.lm_min;
  a.dmax = tb.lm_max;
  a.mfmax = tb.lm_mfmax;
  a.pdesc = tb.lm_desc;
  a.sf = d_sf;
  a.inv_sigma2 = d_inv_sigma2;
  a.scale_thr = d_scale_thr;
  a.best_idx = fb.idx;
  a.best_dist = fb.dist;
  a.n_found = fb.n;
  a.pose = fb.pose;
  a.kf_bcast = kf_side ? -1 : tb.cur_bcast;
  a.point_row = point_row;
  a.cap = tb.kp_cap;
  a.max_points = tb.max_points;
  a.nlevels = kf->nlevels;   // (sd_track_create requires cur and ref to share nlevels and scaleFactor: d_scale_thr serves both sides)
  a.sim3 = sim3;
  a.th = th;
  return launch_fuse_args(a, cam, n_frames, s);
}

}  // namespace sd

using namespace sd;

extern "C" {

int sd_track_set_fuse_scw(sd_track* h, int frame0, int n_frames, const double* Scw_cm16) {
  QUEUE_RANGE(h, frame0, n_frames);
  SD_REQUIRE(Scw_cm16, SD_ERR_INVALID_ARG, "NULL argument");
  END_RESULTS(h, "sd_track_set_fuse_scw");
  SD_TRY(h->pose_ring.upload(h->fu.Scw + (size_t)frame0 * 16, Scw_cm16, (size_t)n_frames * 16, h->pnp_stream));
  std::fill(h->scw_set.begin() + frame0, h->scw_set.begin() + frame0 + n_frames, (uint8_t)1);
  return SD_OK;
}

int sd_track_fuse(sd_track* h, int n_frames, int kf_side, int point_row, float th, int sim3) {
  SD_REQUIRE(h, SD_ERR_INVALID_ARG, "handle is NULL");
  SD_REQUIRE(h->have_cam, SD_ERR_INVALID_ARG, "sd_track_set_camera has not been called");
  SD_REQUIRE(n_frames >= 1 && n_frames <= h->max_batch, SD_ERR_CAPACITY, "n_frames exceeds max_batch");
  SD_REQUIRE((kf_side == 0 || kf_side == 1) && (sim3 == 0 || sim3 == 1), SD_ERR_INVALID_ARG, "kf_side and sim3 must be 0 or 1");
  SD_REQUIRE(std::isfinite(th) && th > 0, SD_ERR_INVALID_ARG, "th must be finite and positive");
  SD_REQUIRE(point_row >= -1 && point_row < h->max_batch, SD_ERR_INVALID_ARG, "point_row outside [-1, max_batch)");
  if (kf_side) {
    SD_TRY(require_ref_frames(h, n_frames, false, true));
  } else {
    const int need = h->tb.cur_bcast >= 0 ? h->tb.cur_bcast + 1 : n_frames;
    SD_REQUIRE(h->cur->have_geom && h->cur->last_frames >= need, SD_ERR_INVALID_ARG, "current frames have not been extracted");
  }
  if (sim3)
    for (int f = 0; f < n_frames; f++)
      SD_REQUIRE(h->scw_set[f], SD_ERR_INVALID_ARG, "sim3 = 1, but sd_track_set_fuse_scw has not covered these slots");
  SD_HIP_CHECK(hipSetDevice(h->device));
  END_RESULTS(h, "sd_track_fuse");
  SD_TRY(run_stage(h, kf_side != 0, false, STAGE_NONE, [&](hipStream_t s) {
    return launch_fuse(h->cur, h->ref, h->tb, h->fu, h->cam, h->d_sf, h->d_inv_sigma2, h->d_scale_thr, n_frames, kf_side, point_row, th,
                       sim3, s);
  }));
  h->res.fuse.set(n_frames, bind_fuse(kf_side), inputs_now(h), kf_side);
  return SD_OK;
}

int sd_track_get_fuse(sd_track* h, int frame0, int n_frames, int32_t* best_idx, int32_t* best_dist, int cap, int32_t* n_found) {
  TRACK_RANGE(h, frame0, n_frames);
  SD_REQUIRE(h->res.fuse.live(frame0 + n_frames, inputs_now(h)), SD_ERR_INVALID_ARG,
             "sd_track_fuse has not run on these slots (or their keyframes, points, mvuRight, poses, Scw, the camera or the broadcast "
             "setting were replaced since)");
  SD_REQUIRE((!best_idx && !best_dist) || cap >= h->max_points, SD_ERR_CAPACITY, "cap smaller than max_points");
  hipStream_t s = h->cur->stream;
  SD_TRY(download_rows(best_idx, cap, h->fu.idx, frame0, n_frames, h->max_points, s));
  SD_TRY(download_rows(best_dist, cap, h->fu.dist, frame0, n_frames, h->max_points, s));
  SD_TRY(download(n_found, h->fu.n, frame0, n_frames, 1, s));
  return wait_for(s);
}

int sd_debug_fuse(int n_kp, const sd_keypoint* kps, const uint8_t* desc, const float* uright, int n_pts, const uint8_t* cand,
                  const double* Xw, const double* normal, const float* min_dist, const float* max_dist, const float* mf_max_dist,
                  const uint8_t* pt_desc, const double* T_cm16, int sim3, const float* cam9, const float* scale_factors,
                  const float* inv_level_sigma2, int nlevels, float scale_factor, float th, int kp_cap, int max_points,
                  int32_t* best_idx, int32_t* best_dist, int32_t* n_found, double* pose15) {
  SD_REQUIRE(kp_cap >= 1 && kp_cap <= 2048 && max_points >= 1 && max_points <= 2048 && n_kp >= 0 && n_kp <= kp_cap && n_pts >= 0 &&
                 n_pts <= max_points,
             SD_ERR_CAPACITY, "at most 2048 keypoints / map points, counts within their capacities");
  SD_REQUIRE((n_kp == 0 || (kps && desc && uright)) &&
                 (n_pts == 0 || (cand && Xw && normal && min_dist && max_dist && mf_max_dist && pt_desc)),
             SD_ERR_INVALID_ARG, "NULL keyframe or point array");
  SD_REQUIRE(T_cm16 && cam9 && scale_factors && inv_level_sigma2 && nlevels >= 1 && nlevels <= SD_MAX_LEVELS && scale_factor > 1.0f &&
                 best_idx && best_dist && n_found && (sim3 == 0 || sim3 == 1) && std::isfinite(th) && th > 0 && cam9[0] > 0 &&
                 cam9[1] > 0 && cam9[6] > cam9[5] && cam9[8] > cam9[7],
             SD_ERR_INVALID_ARG, "bad arguments");
  const TrackCam cam = make_cam(cam9[0], cam9[1], cam9[2], cam9[3], cam9[4], cam9[5], cam9[6], cam9[7], cam9[8]);
  float thr[SD_MAX_LEVELS];
  predict_scale_thresholds(scale_factor, thr);
  const size_t K = (size_t)kp_cap, M = (size_t)max_points;
  Blob b;
  const int32_t counts[4] = {n_kp, n_pts, 0, 0};
  const size_t o_k = b.reserve(K, kps, n_kp), o_d = b.reserve(K * 32, desc, (size_t)n_kp * 32), o_u = b.reserve(K, uright, n_kp);
  const size_t o_n = b.reserve(4, counts, 4), o_T = b.reserve(16, T_cm16, 16), o_c = b.reserve(M, cand, n_pts);
  const size_t o_X = b.reserve(M * 3, Xw, (size_t)n_pts * 3), o_N = b.reserve(M * 3, normal, (size_t)n_pts * 3);
  const size_t o_mn = b.reserve(M, min_dist, n_pts), o_mx = b.reserve(M, max_dist, n_pts), o_mf = b.reserve(M, mf_max_dist, n_pts);
  const size_t o_pd = b.reserve(M * 32, pt_desc, (size_t)n_pts * 32), o_sf = b.reserve(nlevels, scale_factors, nlevels);
  const size_t o_is = b.reserve(nlevels, inv_level_sigma2, nlevels), o_th = b.reserve(SD_MAX_LEVELS, thr, SD_MAX_LEVELS);
  const size_t o_bi = b.reserve<int32_t>(M), o_bd = b.reserve<int32_t>(M), o_p = b.reserve<double>(15);
  SD_TRY(b.run("sd_debug_fuse", [&] {
    FuseArgs a{};
    a.kps = b.dev<sd_keypoint>(o_k); a.desc = b.dev<uint8_t>(o_d); a.nkp = b.dev<int32_t>(o_n); a.uright = b.dev<float>(o_u);
    a.T = b.dev<double>(o_T); a.n_pts = b.dev<int32_t>(o_n) + 1; a.cand = b.dev<uint8_t>(o_c); a.Xw = b.dev<double>(o_X);
    a.normal = b.dev<double>(o_N); a.dmin = b.dev<float>(o_mn); a.dmax = b.dev<float>(o_mx); a.mfmax = b.dev<float>(o_mf);
    a.pdesc = b.dev<uint8_t>(o_pd); a.sf = b.dev<float>(o_sf); a.inv_sigma2 = b.dev<float>(o_is); a.scale_thr = b.dev<float>(o_th);
    a.best_idx = b.dev<int32_t>(o_bi); a.best_dist = b.dev<int32_t>(o_bd); a.n_found = b.dev<int32_t>(o_n) + 2;
    a.pose = b.dev<double>(o_p);
    a.kf_bcast = -1; a.point_row = -1; a.cap = kp_cap; a.max_points = max_points; a.nlevels = nlevels; a.sim3 = sim3; a.th = th;
    return launch_fuse_args(a, cam, 1, 0);
  }));
  b.take(best_idx, o_bi, M * 4);
  b.take(best_dist, o_bd, M * 4);
  b.take(n_found, o_n + 8, 4);
  if (pose15) b.take(pose15, o_p, 15 * 8);
  return SD_OK;
}

}  // extern "C"
