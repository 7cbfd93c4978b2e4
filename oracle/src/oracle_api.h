// ORACLE (test infrastructure only -- never linked into the product path).
// C entry points of liboracle.so, bound with ctypes from tests/, __graft_entry__.smoke()
// and bench.py's cpu_baseline leg ONLY.  See oracle/README.md.
#pragma once
#include <cstdint>
extern "C" {
void* orc_orb_create(int nfeatures, float scaleFactor, int nlevels, int thFAST);
void orc_orb_destroy(void* h);
void orc_orb_tables(void* h, float* sf, float* inv_sf, float* sigma2, float* inv_sigma2, int* quota, int* umax16);
int orc_orb_extract(void* h, const uint8_t* img, int w, int hh, int stride, void* kps_out, uint8_t* desc_out, int cap);
// ImageAlign::ComputePose (align_oracle.cc); orc_align_trace is the same call with a per-level / per-iteration trace, a
// counterfactual (0: the reference) and the order in which H is formed (0: the reference's, 1: the device's)
int orc_align(int nlevels, const uint8_t* const* cur_lv, const uint8_t* const* ref_lv, const int* lv_w, const int* lv_h,
              const int* lv_step_cur, const int* lv_step_ref, const float* inv_sf, const float* sf, const double* Xw, int npts,
              const double* Tref_cm, double* Tcur_cm_inout, double fx, double fy, double cx, double cy, int mode, double* error_out,
              int* iters_out, double* chi2_out);
int orc_align_trace(int nlevels, const uint8_t* const* cur_lv, const uint8_t* const* ref_lv, const int* lv_w, const int* lv_h,
                    const int* lv_step_cur, const int* lv_step_ref, const float* inv_sf, const float* sf, const double* Xw, int npts,
                    const double* Tref_cm, double* Tcur_cm_inout, double fx, double fy, double cx, double cy, int mode, double* error_out,
                    int* iters_out, double* chi2_out, int* lv_i, double* lv_d, int* it_i, double* it_d, uint8_t* flags, int counterfactual,
                    int h_order);
}
