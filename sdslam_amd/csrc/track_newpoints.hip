// RGB-D map point creation on the device: Tracking::StereoInitialization (reference src/Tracking.cc:302-349),
// the RGB-D part of Tracking::CreateNewKeyFrame (:837-888) and the decision Tracking::NeedNewKeyFrame (:753-826).
// Everything they read is resident: mvDepth (tb.depth), mvKeysUn, the frame's final pose (tb.Tcur), mvpMapPoints
// (cur_match / un_match) and Observations() (tb.obs / tb.lm_obs).  The created points reach the next frame through
// k_advance (track_seq.hip); KeyFrame objects and the covisibility graph stay with the caller.
#include <hip/hip_runtime.h>

#include "orb_internal.h"
#include "sd_wave.h"
#include "track_internal.h"

namespace sd {

static constexpr int NP_KEYS = 2048;                      // capacity of the LDS sort (= the tracker's keypoint limit)
static constexpr unsigned long long NP_NONE = ~0ull;      // key of a keypoint that is no candidate: sorts behind every depth

// One 256-thread workgroup per slot.
// mode 1, CreateNewKeyFrame (:840-887), for keypoints i < N = min(nkp, kp_cap):
//   candidates: mvDepth[i] > 0 (NaN and non-positive depths are none), as 64-bit keys float_bits(z) << 32 | i -- positive
//   floats order like their bit patterns, so ascending keys are std::sort's order on pair<float, int>: a total order, the
//   result does not depend on the sort algorithm.  Bitonic sort in LDS over the next power of two >= N.
//   processed prefix P: both branches of the reference loop increment nPoints, so nPoints == j + 1 and the loop breaks after
//   the first j with z_j > th_depth && j + 1 > 100: P = that j + 1, or the number of candidates (ballot per wave, minimum
//   over the waves).  For j < P keypoint i = idx[j] gets a new point iff it holds none after "Clean VO matches" (:250-257)
//   BEFORE the outlier discard (:272-275): kept_point_obs(..., with_outliers) < 1.
//   ids: next_id + rank among the created points in sorted order (MapPoint::nNextId grows in creation order): ballot prefix
//   counts per wave, wave offsets through LDS, no atomics.  The slot's mnLastKeyFrameId (kf_state[2]) = frame_id (:894).
//   Slots whose tracking call `source` did not end tracked (the reference gets here under `if (bOK)`, :241) or whose
//   keyframe flag is clear (use_flags) create nothing.
// mode 2, StereoInitialization (:303-327): a slot with N > min_keypoints sets Tcur to the identity and every keypoint with
//   z > 0 gets a point, ids in keypoint order; a slot with N <= min_keypoints creates nothing.
// Frame::UnprojectStereo (src/Frame.cc:419-431): x = (u - cx) * z * invfx, y = (v - cy) * z * invfy in float, left to right;
//   Xw = Rwc * (x, y, z) + Ow in double with Rwc = Rcw^T, Ow = -Rwc * tcw, every row summed left to right, each product and
//   sum rounded on its own (the project's definition of the order: DESIGN.md §3).
__global__ __launch_bounds__(256) void k_new_points(const sd_keypoint* __restrict__ kps_un_all, const int32_t* __restrict__ nkp_all,
                                                    TrackBuffers tb, float fcx, float fcy, float inv_fx, float inv_fy, int mode, int source,
                                                    float th_depth, int use_flags, int frame_id, int min_keypoints) {
  __shared__ unsigned long long s_key[NP_KEYS];
  __shared__ uint8_t s_flag[NP_KEYS];
  __shared__ double s_R[9], s_Ow[3];
  __shared__ int s_cnt[4], s_min[4];
  const int f = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int cap = tb.kp_cap;
  const size_t o = (size_t)f * tb.max_points, ko = (size_t)f * cap;
  const int N = min(nkp_all[f], cap);
  const bool init = mode == 2;
  bool active;
  if (init) {
    active = N > min_keypoints;
  } else {
    const int status = (source == 0 ? tb.tw_info : tb.tl_info)[(size_t)f * 4];
    active = status == 2 && (!use_flags || (tb.kf_flags[f] & 1));
  }
  if (!active) {   // uniform over the workgroup
    for (int i = tid; i < cap; i += 256) tb.np_flag[ko + i] = 0;
    if (tid < 4) tb.np_info[(size_t)f * 4 + tid] = 0;
    return;
  }
  const int id0 = tb.next_id[f];
  // pose: Rwc[r][k] = Rcw[k][r] = T[r * 4 + k] (T column-major), tcw = T[12..14]
  double* T = tb.Tcur + (size_t)f * 16;
  if (init && tid < 16) T[tid] = (tid % 5 == 0) ? 1.0 : 0.0;
  if (tid < 3) {
    double R0, R1, R2, t0, t1, t2;
    if (init) {
      R0 = tid == 0; R1 = tid == 1; R2 = tid == 2;
      t0 = t1 = t2 = 0.0;
    } else {
      R0 = T[tid * 4]; R1 = T[tid * 4 + 1]; R2 = T[tid * 4 + 2];
      t0 = T[12]; t1 = T[13]; t2 = T[14];
    }
    s_R[tid * 3] = R0; s_R[tid * 3 + 1] = R1; s_R[tid * 3 + 2] = R2;
    s_Ow[tid] = -__dadd_rn(__dadd_rn(__dmul_rn(R0, t0), __dmul_rn(R1, t1)), __dmul_rn(R2, t2));
  }
  // candidate keys
  int KP2 = 2;
  while (KP2 < N) KP2 <<= 1;   // <= NP_KEYS: kp_cap <= 2048 (launch_new_points)
  const float* depth = tb.depth + ko;
  int ncand = 0;
  for (int i = tid; i < NP_KEYS; i += 256) s_flag[i] = 0;
  for (int base = 0; base < KP2; base += 256) {   // trip counts are uniform over the workgroup: the ballots see every lane
    const int i = base + tid;
    unsigned long long key = NP_NONE;
    if (i < N) {
      const float z = depth[i];
      if (z > 0) key = ((unsigned long long)__float_as_uint(z) << 32) | (unsigned)i;
    }
    if (i < KP2) s_key[i] = key;
    ncand += __popcll(__ballot(key != NP_NONE));
  }
  if (lane == 0) s_cnt[wave] = ncand;
  __syncthreads();
  ncand = s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
  int L = N;   // mode 2: keypoint order, non-candidates skipped
  if (!init) {
    for (int k = 2; k <= KP2; k <<= 1)
      for (int j = k >> 1; j > 0; j >>= 1) {
        for (int i = tid; i < KP2; i += 256) {
          const int ixj = i ^ j;
          if (ixj > i) {
            const unsigned long long a = s_key[i], b = s_key[ixj];
            const bool up = (i & k) == 0;
            if ((a > b) == up) {
              s_key[i] = b;
              s_key[ixj] = a;
            }
          }
        }
        __syncthreads();
      }
    // the first j with z_j > th_depth && j + 1 > 100 (strict: a point at exactly th_depth does not end the loop)
    int jmin = 0x7FFFFFFF;
    for (int base = 0; base < KP2; base += 256) {
      const int j = base + tid;
      const bool hit = j < ncand && j >= 100 && __uint_as_float((unsigned)(s_key[min(j, KP2 - 1)] >> 32)) > th_depth;
      const unsigned long long b = __ballot(hit);
      if (b && jmin == 0x7FFFFFFF) jmin = base + wave * 64 + __ffsll((long long)b) - 1;
    }
    if (lane == 0) s_min[wave] = jmin;
    __syncthreads();
    jmin = min(min(s_min[0], s_min[1]), min(s_min[2], s_min[3]));
    L = jmin == 0x7FFFFFFF ? ncand : jmin + 1;
  }
  const int32_t* match = (source == 0 ? tb.cur_match : tb.un_match) + ko;
  const uint8_t* outl = tb.po_outlier + ko;
  const sd_keypoint* kps = kps_un_all + ko;
  int total = 0;
  for (int base = 0; base < L; base += 256) {
    const int j = base + tid;
    bool create = false;
    int i = 0;
    float z = 0.f;
    if (j < L) {
      const unsigned long long key = s_key[j];
      if (key != NP_NONE) {
        i = (int)(unsigned)key;
        z = __uint_as_float((unsigned)(key >> 32));
        bool loc;
        size_t e;
        create = init || kept_point_obs(tb, source, match[i], outl + i, o, &e, &loc, true) < 1;
      }
    }
    const unsigned long long b = __ballot(create);
    __syncthreads();   // the previous round's s_cnt has been read
    if (lane == 0) s_cnt[wave] = __popcll(b);
    __syncthreads();
    int off = total;
    for (int w = 0; w < wave; w++) off += s_cnt[w];
    total += s_cnt[0] + s_cnt[1] + s_cnt[2] + s_cnt[3];
    if (create) {
      const int rank = off + __popcll(b & lanemask_lt(lane));
      const float x = __fmul_rn(__fmul_rn(__fsub_rn(kps[i].x, fcx), z), inv_fx);
      const float y = __fmul_rn(__fmul_rn(__fsub_rn(kps[i].y, fcy), z), inv_fy);
      const double xd = (double)x, yd = (double)y, zd = (double)z;
      double* X = tb.np_Xw + (ko + i) * 3;
      for (int r = 0; r < 3; r++)
        X[r] = __dadd_rn(__dadd_rn(__dadd_rn(__dmul_rn(s_R[r * 3], xd), __dmul_rn(s_R[r * 3 + 1], yd)), __dmul_rn(s_R[r * 3 + 2], zd)),
                         s_Ow[r]);
      tb.np_id[ko + i] = id0 + rank;
      tb.np_list[ko + rank] = i;
      s_flag[i] = 1;
    }
  }
  __syncthreads();
  for (int i = tid; i < cap; i += 256) tb.np_flag[ko + i] = s_flag[i];
  if (tid == 0) {
    int32_t* info = tb.np_info + (size_t)f * 4;
    info[0] = mode;
    info[1] = total;
    info[2] = init ? ncand : L;
    info[3] = ncand;
    tb.next_id[f] = id0 + total;
    if (!init) tb.kf_state[(size_t)f * 8 + 2] = frame_id;
  }
}

// Tracking::NeedNewKeyFrame (src/Tracking.cc:753-826), one lane per slot, on the close-point counts of k_close_points,
// mnMatchesInliers of TrackLocalMap (tl_info[2]) and the caller's state (kf_state).  The reference's arithmetic types are
// kept: mnMatchesInliers < nRefMatches * 0.25 compares in double, nRefMatches * thRefRatio in float.  A slot that
// TrackLocalMap did not leave tracked gets 0 (the reference decides under `if (bOK)`).
__global__ void k_need_keyframe(TrackBuffers tb, const int32_t* __restrict__ close, int n_frames, int rgbd, int frame_id, int min_frames,
                                int max_frames) {
  const int f = blockIdx.x * blockDim.x + threadIdx.x;
  if (f >= n_frames) return;
  const int32_t* st = tb.kf_state + (size_t)f * 8;
  const int nKFs = st[0], nRefMatches = st[1], last_kf = st[2], last_reloc = st[3], fl = st[4];
  const int inliers = tb.tl_info[(size_t)f * 4 + 2];
  uint8_t out = 0;
  const bool tracked = tb.tl_info[(size_t)f * 4] == 2;
  const bool stopped = fl & 2;
  const bool after_reloc = frame_id < last_reloc + max_frames && nKFs > max_frames;
  if (tracked && !stopped && !after_reloc) {
    const bool idle = fl & 1;
    const int n_tracked = rgbd ? close[(size_t)f * 2] : 0, n_non = rgbd ? close[(size_t)f * 2 + 1] : 0;
    const bool need_close = n_tracked < 100 && n_non > 70;
    float th_ref = 0.75f;
    if (nKFs < 2) th_ref = 0.4f;
    if (!rgbd) th_ref = 0.9f;
    const bool c1a = frame_id >= last_kf + max_frames;
    const bool c1b = frame_id >= last_kf + min_frames && idle;
    const bool c1c = rgbd && ((double)inliers < __dmul_rn((double)nRefMatches, 0.25) || need_close);
    const bool c2 = ((float)inliers < __fmul_rn((float)nRefMatches, th_ref) || need_close) && inliers > 15;
    if ((c1a || c1b || c1c) && c2) {
      if (idle) out = 1;
      else out = 2 | ((rgbd && (fl & 4)) ? 1 : 0);   // InterruptBA is the caller's; KeyframesInQueue() < 3 still inserts
    }
  }
  tb.kf_flags[f] = out;
}

__global__ void k_set_keyframe_state(TrackBuffers tb, const int32_t* __restrict__ staged, int frame0, int n) {
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= n * 8) return;
  const int32_t v = staged[t];
  if (v != INT32_MIN) tb.kf_state[(size_t)frame0 * 8 + t] = v;
}

int launch_new_points(const sd_orb* cur, const TrackBuffers& tb, const TrackCam& cam, float inv_fx, float inv_fy, int n_frames, int mode,
                      int source, float th_depth, int use_flags, int frame_id, int min_keypoints, hipStream_t s) {
  SD_REQUIRE(tb.kp_cap <= NP_KEYS, SD_ERR_CAPACITY, "map point creation sorts at most 2048 keypoints per frame");
  hipLaunchKernelGGL(k_new_points, dim3(n_frames), dim3(256), 0, s, keys_un(cur), cur->d_nout, tb, cam.fcx,
                     cam.fcy, inv_fx, inv_fy, mode, source, th_depth, use_flags, frame_id, min_keypoints);
  SD_HIP_CHECK(hipGetLastError());
  return SD_OK;
}

int launch_need_keyframe(const TrackBuffers& tb, const int32_t* d_close, int n_frames, int rgbd, int frame_id, int min_frames,
                         int max_frames, hipStream_t s) {
  hipLaunchKernelGGL(k_need_keyframe, dim3((n_frames + 63) / 64), dim3(64), 0, s, tb, d_close, n_frames, rgbd, frame_id, min_frames,
                     max_frames);
  SD_HIP_CHECK(hipGetLastError());
  return SD_OK;
}

int launch_set_keyframe_state(const TrackBuffers& tb, const int32_t* staged, int frame0, int n_frames, hipStream_t s) {
  hipLaunchKernelGGL(k_set_keyframe_state, dim3((n_frames * 8 + 255) / 256), dim3(256), 0, s, tb, staged, frame0, n_frames);
  SD_HIP_CHECK(hipGetLastError());
  return SD_OK;
}

}  // namespace sd
