// tools/valu_microbench.hip -- what the vector ALUs of an MI355X really sustain for the instructions the FAST / pyramid /
// matcher kernels are made of, at 1, 2, 4 and 8 resident waves per SIMD (VERDICT r1 "next" 3.i), plus three streaming-read
// kernels of known byte counts for calibrating rocprofv3's FETCH_SIZE on narrow loads (3.ii).
//
//   hipcc -O3 --offload-arch=gfx950 tools/valu_microbench.hip -o tools/build/valu_microbench
//   tools/build/valu_microbench            # prints a JSON object (cycles per wave64 instruction per SIMD)
//   rocprofv3 --pmc FETCH_SIZE ... -- tools/build/valu_microbench --stream   # only the three stream kernels
//
// Method: every wave runs ITERS x 32 instructions of one kind (8 independent dependency chains, so latency never limits a
// single wave), stamped at both ends with s_memtime (tick = shader cycle, MI355X_MICROARCH.md) AND s_memrealtime (100 MHz,
// constant).  W waves per SIMD: 256 workgroups of 4 W waves (W <= 4; W = 8: 512 workgroups of 16 waves, 64 KB of LDS each so
// that two fit a CU and three do not); every wave also records where it ran (HW_ID / XCC_ID).
// Three figures per (instruction, W), round 3 (VERDICT r2 task 4: the round-2 tool's two methods disagreed up to 3 x):
//   simd_span   per SIMD: (last end stamp - first start stamp of the waves that ran there) / (instructions those waves
//               executed) -- the SIMD's real issue cost also when its waves did not run exactly side by side.  (The round-2
//               figure divided every wave's OWN elapsed time by the number of waves that ever shared its SIMD: waves that
//               start late or finish early run partly alone, so that quotient fell below the 2-cycle hardware floor.)
//   clock_GHz   shader clock DURING the loop = delta s_memtime / delta s_memrealtime x 100 MHz, median over waves (round 2
//               assumed 2.4 GHz when converting the kernel's event time; under an all-VALU load the chip holds less)
//   event       kernel time (HIP events) x measured clock / (instructions per wave x W): the same quantity from outside;
//               it contains launch ramp-up and tail, so it reads a few per cent above simd_span.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(1); } } while (0)

enum { OP_MAX3 = 0, OP_MIN3, OP_PERM, OP_MUL24, OP_MAD24, OP_CMP_SOR, OP_PKMAX16, OP_PKMIN16, OP_ADD, OP_BCNT, OP_ALIGNBYTE, OP_ANDOR, OP_LSHLADD,
       OP_CNDMASK, OP_SUBREV, OP_DS_READ_U8, OP_DS_READ_B32,
       OP_DOT4, OP_DOT2, OP_SATPK, OP_MULLO, OP_CMP, OP_AND, OP_LSHL, OP_BFE, OP_FMA32, OP_FMA64, OP_ADD64, OP_MUL64, OP_RCP32, OP_CVT, OP_MAXI, OP_MAXU, OP_MAXF, OP_MINF, OP_MAX3F, OP_MED3F, OP_ADDF, OP_SUBF, OP_MULF, OP_OR, OP_XOR, OP_OR3, OP_ADD3, OP_LSHR, OP_MOV, OP_CMPF, OP_CMPU, OP_CMPE64, OP_SAD8, OP_CVTUB, OP_PKMAXI16, OP_PKADD16, OP_PKFMAF16, OP_PKMAXF16, OP_MAX3F16, OP_MBCNT, OP_SUBU, OP_MAXI16, OP_MINU16, OP_SUBU16, OP_MIN3U16, OP_MAX3U16, OP_CMPSDWA, OP_CMPU16, OP_LSHLADD1, OP_MINU16_SDWA, OP_MAXU16_SDWA, OP_SUBU16_SDWA, OP_MOV_DPP_WSHR, OP_MOV_DPP_ROWSHR, OP_DS_READ2_B32, OP_MULHI, OP_MULHI_U24, OP_MUL_U24, OP_MED3I, OP_PKMAX3F16, OP_PKMIN3F16, OP_COUNT };
static const char* kNames[OP_COUNT] = {"v_max3_i32", "v_min3_i32", "v_perm_b32", "v_mul_i32_i24", "v_mad_i32_i24", "v_cmp_lt_i32+s_or_b64", "v_pk_max_u16",
                                       "v_pk_min_u16", "v_add_u32", "v_bcnt_u32_b32", "v_alignbyte_b32", "v_and_or_b32", "v_lshl_add_u32", "v_cndmask_b32",
                                       "v_subrev_u32", "ds_read_u8", "ds_read_b32",
                                       "v_dot4_u32_u8", "v_dot2_u32_u16", "v_sat_pk_u8_i16", "v_mul_lo_u32", "v_cmp_lt_i32 (vcc)", "v_and_b32", "v_lshlrev_b32",
                                       "v_bfe_u32", "v_fma_f32", "v_fma_f64", "v_add_f64", "v_mul_f64", "v_rcp_f32", "v_cvt_f32_u32",
                                       "v_max_i32", "v_max_u32", "v_max_f32", "v_min_f32", "v_max3_f32", "v_med3_f32", "v_add_f32", "v_sub_f32", "v_mul_f32", "v_or_b32", "v_xor_b32", "v_or3_b32", "v_add3_u32", "v_lshrrev_b32", "v_mov_b32", "v_cmp_lt_f32 (vcc)", "v_cmp_lt_u32 (vcc)", "v_cmp_lt_i32_e64 (sgpr pair)", "v_sad_u8", "v_cvt_f32_ubyte0", "v_pk_max_i16", "v_pk_add_u16", "v_pk_fma_f16", "v_pk_max_f16", "v_max3_f16", "v_mbcnt_lo_u32_b32", "v_sub_u32", "v_max_i16",
                                       "v_min_u16", "v_sub_u16", "v_min3_u16", "v_max3_u16", "v_cmp_lt_i32_sdwa (sgpr pair)", "v_cmp_gt_u16_e64 (sgpr pair)", "v_lshl_add_u32 (sgpr addend)",
                                       "v_min_u16_sdwa (byte selects)", "v_max_u16_sdwa (byte selects)", "v_sub_u16_sdwa (byte select)", "v_mov_b32_dpp wave_shr:1", "v_mov_b32_dpp row_shr:1", "ds_read2_b32", "v_mul_hi_u32", "v_mul_hi_u32_u24", "v_mul_u32_u24", "v_med3_i32", "v_pk_maximum3_f16", "v_pk_minimum3_f16"};

#define REP8(S)  S(0) S(1) S(2) S(3) S(4) S(5) S(6) S(7)

template <int OP>
__global__ __launch_bounds__(1024) void k_issue(unsigned long long* __restrict__ out, int iters, unsigned seed) {
  extern __shared__ unsigned char lds[];
  unsigned a[8];
  const unsigned t = threadIdx.x;
#pragma unroll
  for (int i = 0; i < 8; i++) a[i] = seed * (i + 3) + t * 2654435761u;
  unsigned b = seed ^ 0x9e3779b9u, c = t | 0x01020304u;
  if (OP == OP_DS_READ_U8 || OP == OP_DS_READ_B32 || OP == OP_DS_READ2_B32) {
    for (int i = t; i < 4096; i += blockDim.x) ((unsigned*)lds)[i] = i * 7u;
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 8; i++) a[i] = (t * 4 + i * 1024) & 16380;
  }
  unsigned long long sacc = 0;
  double da[8], db = 1.0000001 + 1e-9 * (double)seed, dc = 1e-30 * (double)t;
#pragma unroll
  for (int i = 0; i < 8; i++) da[i] = 1.0 + 1e-6 * (double)(a[i] & 1023);
  const unsigned long long r0 = __builtin_amdgcn_s_memrealtime();
  const unsigned long long t0 = __builtin_amdgcn_s_memtime();
  for (int it = 0; it < iters; it++) {
#pragma unroll
    for (int r = 0; r < 4; r++) {
      if (OP == OP_MAX3) {
#define S(i) asm volatile("v_max3_i32 %0, %0, %1, %2" : "+v"(a[i]) : "v"(b), "v"(c));
        REP8(S)
#undef S
      } else if (OP == OP_MIN3) {
#define S(i) asm volatile("v_min3_i32 %0, %0, %1, %2" : "+v"(a[i]) : "v"(b), "v"(c));
        REP8(S)
#undef S
      } else if (OP == OP_PERM) {
#define S(i) asm volatile("v_perm_b32 %0, %0, %1, %2" : "+v"(a[i]) : "v"(b), "v"(c));
        REP8(S)
#undef S
      } else if (OP == OP_MUL24) {
#define S(i) asm volatile("v_mul_i32_i24 %0, %0, %1" : "+v"(a[i]) : "v"(b));
        REP8(S)
#undef S
      } else if (OP == OP_MAD24) {
#define S(i) asm volatile("v_mad_i32_i24 %0, %0, %1, %2" : "+v"(a[i]) : "v"(b), "v"(c));
        REP8(S)
#undef S
      } else if (OP == OP_CMP_SOR) {
        // the FAST compass test's shape: a compare into an SGPR pair, combined on the scalar unit
#define S(i) asm volatile("v_cmp_lt_i32 vcc, %1, %2\n s_or_b64 %0, %0, vcc" : "+s"(sacc) : "v"(a[i]), "v"(b) : "vcc", "scc");
        REP8(S)
#undef S
      } else if (OP == OP_PKMAX16) {
#define S(i) asm volatile("v_pk_max_u16 %0, %0, %1" : "+v"(a[i]) : "v"(b));
        REP8(S)
#undef S
      } else if (OP == OP_PKMIN16) {
#define S(i) asm volatile("v_pk_min_u16 %0, %0, %1" : "+v"(a[i]) : "v"(b));
        REP8(S)
#undef S
      } else if (OP == OP_ADD) {
#define S(i) asm volatile("v_add_u32 %0, %0, %1" : "+v"(a[i]) : "v"(b));
        REP8(S)
#undef S
      } else if (OP == OP_BCNT) {
#define S(i) asm volatile("v_bcnt_u32_b32 %0, %1, %0" : "+v"(a[i]) : "v"(b));
        REP8(S)
#undef S
      } else if (OP == OP_ALIGNBYTE) {
#define S(i) asm volatile("v_alignbyte_b32 %0, %0, %1, %2" : "+v"(a[i]) : "v"(b), "v"(c));
        REP8(S)
#undef S
      } else if (OP == OP_ANDOR) {
#define S(i) asm volatile("v_and_or_b32 %0, %0, %1, %2" : "+v"(a[i]) : "v"(b), "v"(c));
        REP8(S)
#undef S
      } else if (OP == OP_LSHLADD) {
#define S(i) asm volatile("v_lshl_add_u32 %0, %0, 1, %1" : "+v"(a[i]) : "v"(b));
        REP8(S)
#undef S
      } else if (OP == OP_CNDMASK) {
#define S(i) asm volatile("v_cndmask_b32 %0, %0, %1, vcc" : "+v"(a[i]) : "v"(b) : "vcc");
        REP8(S)
#undef S
      } else if (OP == OP_SUBREV) {
#define S(i) asm volatile("v_subrev_u32 %0, %1, %0" : "+v"(a[i]) : "v"(b));
        REP8(S)
#undef S
      } else if (OP == OP_DOT4) {
#define S(i) asm volatile("v_dot4_u32_u8 %0, %0, %1, %2" : "+v"(a[i]) : "v"(b), "v"(c));
        REP8(S)
#undef S
      } else if (OP == OP_DOT2) {
#define S(i) asm volatile("v_dot2_u32_u16 %0, %0, %1, %2" : "+v"(a[i]) : "v"(b), "v"(c));
        REP8(S)
#undef S
      } else if (OP == OP_SATPK) {
#define S(i) asm volatile("v_sat_pk_u8_i16 %0, %0" : "+v"(a[i]));
        REP8(S)
#undef S
      } else if (OP == OP_MULLO) {
#define S(i) asm volatile("v_mul_lo_u32 %0, %0, %1" : "+v"(a[i]) : "v"(b));
        REP8(S)
#undef S
      } else if (OP == OP_CMP) {
#define S(i) asm volatile("v_cmp_lt_i32 vcc, %0, %1" : : "v"(a[i]), "v"(b) : "vcc");
        REP8(S)
#undef S
      } else if (OP == OP_AND) {
#define S(i) asm volatile("v_and_b32 %0, %0, %1" : "+v"(a[i]) : "v"(b));
        REP8(S)
#undef S
      } else if (OP == OP_LSHL) {
#define S(i) asm volatile("v_lshlrev_b32 %0, 1, %0" : "+v"(a[i]));
        REP8(S)
#undef S
      } else if (OP == OP_BFE) {
#define S(i) asm volatile("v_bfe_u32 %0, %0, 1, 31" : "+v"(a[i]));
        REP8(S)
#undef S
      } else if (OP == OP_FMA32) {
#define S(i) asm volatile("v_fma_f32 %0, %0, %1, %2" : "+v"(a[i]) : "v"(b), "v"(c));
        REP8(S)
#undef S
      } else if (OP == OP_FMA64) {
#define S(i) asm volatile("v_fma_f64 %0, %0, %1, %2" : "+v"(da[i]) : "v"(db), "v"(dc));
        REP8(S)
#undef S
      } else if (OP == OP_ADD64) {
#define S(i) asm volatile("v_add_f64 %0, %0, %1" : "+v"(da[i]) : "v"(db));
        REP8(S)
#undef S
      } else if (OP == OP_MUL64) {
#define S(i) asm volatile("v_mul_f64 %0, %0, %1" : "+v"(da[i]) : "v"(db));
        REP8(S)
#undef S
      } else if (OP == OP_RCP32) {
#define S(i) asm volatile("v_rcp_f32 %0, %0" : "+v"(a[i]));
        REP8(S)
#undef S
      } else if (OP == OP_CVT) {
#define S(i) asm volatile("v_cvt_f32_u32 %0, %0" : "+v"(a[i]));
        REP8(S)
#undef S
      } else if (OP == OP_MAXI) {
#define S(i) asm volatile("v_max_i32 %0, %0, %1" : "+v"(a[i]) : "v"(b));
        REP8(S)
#undef S
      } else if (OP == OP_MAXU) {
#define S(i) asm volatile("v_max_u32 %0, %0, %1" : "+v"(a[i]) : "v"(b));
        REP8(S)
#undef S
      } else if (OP == OP_MAXF) {
#define S(i) asm volatile("v_max_f32 %0, %0, %1" : "+v"(a[i]) : "v"(b));
        REP8(S)
#undef S
      } else if (OP == OP_MINF) {
#define S(i) asm volatile("v_min_f32 %0, %0, %1" : "+v"(a[i]) : "v"(b));
        REP8(S)
#undef S
      } else if (OP == OP_MAX3F) {
#define S(i) asm volatile("v_max3_f32 %0, %0, %1, %2" : "+v"(a[i]) : "v"(b), "v"(c));
        REP8(S)
#undef S
      } else if (OP == OP_MED3F) {
#define S(i) asm volatile("v_med3_f32 %0, %0, %1, %2" : "+v"(a[i]) : "v"(b), "v"(c));
        REP8(S)
#undef S
      } else if (OP == OP_ADDF) {
#define S(i) asm volatile("v_add_f32 %0, %0, %1" : "+v"(a[i]) : "v"(b));
        REP8(S)
#undef S
      } else if (OP == OP_SUBF) {
#define S(i) asm volatile("v_sub_f32 %0, %0, %1" : "+v"(a[i]) : "v"(b));
        REP8(S)
#undef S
      } else if (OP == OP_MULF) {
#define S(i) asm volatile("v_mul_f32 %0, %0, %1" : "+v"(a[i]) : "v"(b));
        REP8(S)
#undef S
      } else if (OP == OP_OR) {
#define S(i) asm volatile("v_or_b32 %0, %0, %1" : "+v"(a[i]) : "v"(b));
        REP8(S)
#undef S
      } else if (OP == OP_XOR) {
#define S(i) asm volatile("v_xor_b32 %0, %0, %1" : "+v"(a[i]) : "v"(b));
        REP8(S)
#undef S
      } else if (OP == OP_OR3) {
#define S(i) asm volatile("v_or3_b32 %0, %0, %1, %2" : "+v"(a[i]) : "v"(b), "v"(c));
        REP8(S)
#undef S
      } else if (OP == OP_ADD3) {
#define S(i) asm volatile("v_add3_u32 %0, %0, %1, %2" : "+v"(a[i]) : "v"(b), "v"(c));
        REP8(S)
#undef S
      } else if (OP == OP_LSHR) {
#define S(i) asm volatile("v_lshrrev_b32 %0, 1, %0" : "+v"(a[i]));
        REP8(S)
#undef S
      } else if (OP == OP_MOV) {
#define S(i) asm volatile("v_mov_b32 %0, %1" : "=v"(a[i]) : "v"(b));
        REP8(S)
#undef S
      } else if (OP == OP_CMPF) {
#define S(i) asm volatile("v_cmp_lt_f32 vcc, %0, %1" : : "v"(a[i]), "v"(b) : "vcc");
        REP8(S)
#undef S
      } else if (OP == OP_CMPU) {
#define S(i) asm volatile("v_cmp_lt_u32 vcc, %0, %1" : : "v"(a[i]), "v"(b) : "vcc");
        REP8(S)
#undef S
      } else if (OP == OP_CMPE64) {
#define S(i) asm volatile("v_cmp_lt_i32_e64 %0, %1, %2" : "=s"(sacc) : "v"(a[i]), "v"(b));
        REP8(S)
#undef S
      } else if (OP == OP_SAD8) {
#define S(i) asm volatile("v_sad_u8 %0, %0, %1, %2" : "+v"(a[i]) : "v"(b), "v"(c));
        REP8(S)
#undef S
      } else if (OP == OP_CVTUB) {
#define S(i) asm volatile("v_cvt_f32_ubyte0 %0, %0" : "+v"(a[i]));
        REP8(S)
#undef S
      } else if (OP == OP_PKMAXI16) {
#define S(i) asm volatile("v_pk_max_i16 %0, %0, %1" : "+v"(a[i]) : "v"(b));
        REP8(S)
#undef S
      } else if (OP == OP_PKADD16) {
#define S(i) asm volatile("v_pk_add_u16 %0, %0, %1" : "+v"(a[i]) : "v"(b));
        REP8(S)
#undef S
      } else if (OP == OP_PKFMAF16) {
#define S(i) asm volatile("v_pk_fma_f16 %0, %0, %1, %2" : "+v"(a[i]) : "v"(b), "v"(c));
        REP8(S)
#undef S
      } else if (OP == OP_PKMAXF16) {
#define S(i) asm volatile("v_pk_max_f16 %0, %0, %1" : "+v"(a[i]) : "v"(b));
        REP8(S)
#undef S
      } else if (OP == OP_MAX3F16) {
#define S(i) asm volatile("v_max3_f16 %0, %0, %1, %2" : "+v"(a[i]) : "v"(b), "v"(c));
        REP8(S)
#undef S
      } else if (OP == OP_PKMAX3F16) {   // gfx950: two 16-bit lanes of a three-input max per instruction
#define S(i) asm volatile("v_pk_maximum3_f16 %0, %0, %1, %2" : "+v"(a[i]) : "v"(b), "v"(c));
        REP8(S)
#undef S
      } else if (OP == OP_PKMIN3F16) {
#define S(i) asm volatile("v_pk_minimum3_f16 %0, %0, %1, %2" : "+v"(a[i]) : "v"(b), "v"(c));
        REP8(S)
#undef S
      } else if (OP == OP_MBCNT) {
#define S(i) asm volatile("v_mbcnt_lo_u32_b32 %0, %1, %0" : "+v"(a[i]) : "v"(b));
        REP8(S)
#undef S
      } else if (OP == OP_SUBU) {
#define S(i) asm volatile("v_sub_u32 %0, %0, %1" : "+v"(a[i]) : "v"(b));
        REP8(S)
#undef S
      } else if (OP == OP_MAXI16) {
#define S(i) asm volatile("v_max_i16 %0, %0, %1" : "+v"(a[i]) : "v"(b));
        REP8(S)
#undef S
      } else if (OP == OP_MINU16) {
#define S(i) asm volatile("v_min_u16 %0, %0, %1" : "+v"(a[i]) : "v"(b));
        REP8(S)
#undef S
      } else if (OP == OP_SUBU16) {
#define S(i) asm volatile("v_sub_u16 %0, %0, %1" : "+v"(a[i]) : "v"(b));
        REP8(S)
#undef S
      } else if (OP == OP_MIN3U16) {
#define S(i) asm volatile("v_min3_u16 %0, %0, %1, %2" : "+v"(a[i]) : "v"(b), "v"(c));
        REP8(S)
#undef S
      } else if (OP == OP_MAX3U16) {
#define S(i) asm volatile("v_max3_u16 %0, %0, %1, %2" : "+v"(a[i]) : "v"(b), "v"(c));
        REP8(S)
#undef S
      } else if (OP == OP_CMPSDWA) {
#define S(i) asm volatile("v_cmp_lt_i32_sdwa %0, %1, sext(%2) src0_sel:DWORD src1_sel:WORD_0" : "=s"(sacc) : "v"(a[i]), "v"(b));
        REP8(S)
#undef S
      } else if (OP == OP_CMPU16) {
#define S(i) asm volatile("v_cmp_gt_u16_e64 %0, %1, %2" : "=s"(sacc) : "v"(a[i]), "v"(b));
        REP8(S)
#undef S
      } else if (OP == OP_LSHLADD1) {
#define S(i) asm volatile("v_lshl_add_u32 %0, %0, 1, %1" : "+v"(a[i]) : "s"(seed));
        REP8(S)
#undef S
      } else if (OP == OP_MINU16_SDWA) {
#define S(i) asm volatile("v_min_u16_sdwa %0, %0, %1 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_1 src1_sel:BYTE_3" : "+v"(a[i]) : "v"(b));
        REP8(S)
#undef S
      } else if (OP == OP_MAXU16_SDWA) {
#define S(i) asm volatile("v_max_u16_sdwa %0, %0, %1 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_0 src1_sel:BYTE_2" : "+v"(a[i]) : "v"(b));
        REP8(S)
#undef S
      } else if (OP == OP_SUBU16_SDWA) {
#define S(i) asm volatile("v_sub_u16_sdwa %0, %0, %1 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:WORD_0 src1_sel:BYTE_2" : "+v"(a[i]) : "v"(b));
        REP8(S)
#undef S
      } else if (OP == OP_MOV_DPP_WSHR) {
#define S(i) asm volatile("s_nop 1\n\tv_mov_b32_dpp %0, %0 wave_shr:1 row_mask:0xf bank_mask:0xf" : "+v"(a[i]));
        REP8(S)
#undef S
      } else if (OP == OP_MOV_DPP_ROWSHR) {
#define S(i) asm volatile("s_nop 1\n\tv_mov_b32_dpp %0, %0 row_shr:1 row_mask:0xf bank_mask:0xf" : "+v"(a[i]));
        REP8(S)
#undef S
      } else if (OP == OP_MULHI) {
#define S(i) asm volatile("v_mul_hi_u32 %0, %0, %1" : "+v"(a[i]) : "v"(b));
        REP8(S)
#undef S
      } else if (OP == OP_MULHI_U24) {
#define S(i) asm volatile("v_mul_hi_u32_u24 %0, %0, %1" : "+v"(a[i]) : "v"(b));
        REP8(S)
#undef S
      } else if (OP == OP_MUL_U24) {
#define S(i) asm volatile("v_mul_u32_u24 %0, %0, %1" : "+v"(a[i]) : "v"(b));
        REP8(S)
#undef S
      } else if (OP == OP_MED3I) {
#define S(i) asm volatile("v_med3_i32 %0, %0, %1, %2" : "+v"(a[i]) : "v"(b), "v"(c));
        REP8(S)
#undef S
      } else if (OP == OP_DS_READ2_B32) {
        unsigned long long v[8];
#define S(i) asm volatile("ds_read2_b32 %0, %1 offset1:33" : "=v"(v[i]) : "v"(a[i]));
        REP8(S)
#undef S
        asm volatile("s_waitcnt lgkmcnt(0)");
#pragma unroll
        for (int i = 0; i < 8; i++) c ^= (unsigned)v[i] ^ (unsigned)(v[i] >> 32);
      } else if (OP == OP_DS_READ_U8) {
        unsigned v[8];
#define S(i) asm volatile("ds_read_u8 %0, %1" : "=v"(v[i]) : "v"(a[i]));
        REP8(S)
#undef S
        asm volatile("s_waitcnt lgkmcnt(0)");
#pragma unroll
        for (int i = 0; i < 8; i++) c ^= v[i];
      } else {
        unsigned v[8];
#define S(i) asm volatile("ds_read_b32 %0, %1" : "=v"(v[i]) : "v"(a[i]));
        REP8(S)
#undef S
        asm volatile("s_waitcnt lgkmcnt(0)");
#pragma unroll
        for (int i = 0; i < 8; i++) c ^= v[i];
      }
    }
  }
  const unsigned long long t1 = __builtin_amdgcn_s_memtime();
  const unsigned long long r1 = __builtin_amdgcn_s_memrealtime();
  unsigned s = c ^ (unsigned)sacc;
#pragma unroll
  for (int i = 0; i < 8; i++) s ^= a[i] ^ (unsigned)__double2loint(da[i]);
  if ((t & 63) == 0) {
    unsigned hw, xcc;
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
    asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
    const size_t w = (size_t)blockIdx.x * (blockDim.x >> 6) + (t >> 6);
    out[5 * w] = t0 + (s == 0x12345u);
    out[5 * w + 1] = t1;
    out[5 * w + 2] = r0;
    out[5 * w + 3] = r1;
    out[5 * w + 4] = ((unsigned long long)(xcc & 0xf) << 32) | (hw & 0xfff0u);   // simd [5:4], pipe [7:6], cu [11:8], sh [12], se [15:13]
  }
}

// ---- streaming reads of known size (FETCH_SIZE calibration): every byte of `n` bytes is read exactly once
__global__ void k_stream_dwordx4(const uint4* __restrict__ p, size_t n16, unsigned* __restrict__ sink) {
  unsigned acc = 0;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n16; i += (size_t)gridDim.x * blockDim.x) {
    const uint4 v = p[i];
    acc ^= v.x ^ v.y ^ v.z ^ v.w;
  }
  if (acc == 0x1234567u) *sink = acc;
}
__global__ void k_stream_dword(const unsigned* __restrict__ p, size_t n4, unsigned* __restrict__ sink) {
  unsigned acc = 0;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n4; i += (size_t)gridDim.x * blockDim.x) acc ^= p[i];
  if (acc == 0x1234567u) *sink = acc;
}
__global__ void k_stream_byte(const unsigned char* __restrict__ p, size_t n, unsigned* __restrict__ sink) {
  unsigned acc = 0;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) acc ^= p[i];
  if (acc == 0x1234567u) *sink = acc;
}
// the FAST tile-staging shape: rows of `roww` aligned dwords out of a pitch-`pitch` image, one 2-D tile per workgroup, tiles
// overlap by `halo` rows/columns (re-reads that L2 should absorb)
__global__ void k_stream_tiles(const unsigned* __restrict__ p, int pitch_w, int tile_w, int tile_h, int step_w, int step_h, int ntx, unsigned* __restrict__ sink) {
  const int tx = blockIdx.x % ntx, ty = blockIdx.x / ntx;
  const unsigned* g = p + (size_t)blockIdx.y * pitch_w * 4096 + (size_t)ty * step_h * pitch_w + tx * step_w;
  unsigned acc = 0;
  for (int i = threadIdx.x; i < tile_w * tile_h; i += blockDim.x) acc ^= g[(size_t)(i / tile_w) * pitch_w + (i % tile_w)];
  if (acc == 0x1234567u) *sink = acc;
}

struct IssueResult { double simd_span, clock_ghz, event, share; };

template <int OP>
static IssueResult run_issue(int W, int iters, unsigned long long* d_out, std::vector<unsigned long long>& h) {
  const int wpb = W <= 4 ? 4 * W : 16, nblk = W <= 4 ? 256 : 512;
  const size_t lds = 64 * 1024;
  fprintf(stderr, "op %d W %d ...", OP, W);
  fflush(stderr);
  hipLaunchKernelGGL(k_issue<OP>, dim3(nblk), dim3(64 * wpb), lds, 0, d_out, 64, 1u);   // warm-up (clocks, code)
  CK(hipDeviceSynchronize());
  static hipEvent_t e0 = nullptr, e1 = nullptr;
  if (!e0) { CK(hipEventCreate(&e0)); CK(hipEventCreate(&e1)); }
  CK(hipEventRecord(e0));
  hipLaunchKernelGGL(k_issue<OP>, dim3(nblk), dim3(64 * wpb), lds, 0, d_out, iters, 2u);
  CK(hipEventRecord(e1));
  CK(hipGetLastError());
  CK(hipDeviceSynchronize());
  float ms = 0;
  CK(hipEventElapsedTime(&ms, e0, e1));
  const size_t nw = (size_t)nblk * wpb;
  h.resize(nw * 5);
  CK(hipMemcpy(h.data(), d_out, h.size() * 8, hipMemcpyDeviceToHost));
  // per SIMD: first start, last end, waves (s_memtime is one counter per XCD: stamps of one SIMD are comparable)
  std::vector<std::pair<unsigned long long, size_t>> order(nw);
  for (size_t i = 0; i < nw; i++) order[i] = {h[5 * i + 4], i};
  std::sort(order.begin(), order.end());
  std::vector<double> per_simd, clocks;
  double share = 0;
  for (size_t a = 0; a < nw;) {
    size_t b = a;
    unsigned long long first = ~0ull, last = 0;
    while (b < nw && order[b].first == order[a].first) {
      const size_t i = order[b].second;
      first = std::min(first, h[5 * i]);
      last = std::max(last, h[5 * i + 1]);
      b++;
    }
    per_simd.push_back((double)(last - first) / ((double)(b - a) * iters * 32.0));
    share += (double)(b - a) * (b - a);
    a = b;
  }
  for (size_t i = 0; i < nw; i++) {
    const double dt = (double)(h[5 * i + 1] - h[5 * i]), dr = (double)(h[5 * i + 3] - h[5 * i + 2]);
    if (dr > 0) clocks.push_back(dt / dr * 0.1);   // ticks per 10 ns -> GHz
  }
  std::sort(per_simd.begin(), per_simd.end());
  std::sort(clocks.begin(), clocks.end());
  IssueResult r;
  r.simd_span = per_simd[per_simd.size() / 2];
  r.clock_ghz = clocks.empty() ? 0.0 : clocks[clocks.size() / 2];
  r.event = (double)ms * 1e-3 * r.clock_ghz * 1e9 / ((double)iters * 32.0 * W);
  r.share = share / nw;
  fprintf(stderr, " done\n");
  return r;
}

int main(int argc, char** argv) {
  const bool stream_only = argc > 1 && !strcmp(argv[1], "--stream");
  CK(hipSetDevice(0));
  unsigned long long* d_out;
  CK(hipMalloc(&d_out, 512 * 16 * 5 * 8));
  std::vector<unsigned long long> h;
  if (!stream_only) {
    printf("{\"unit\": \"shader cycles per wave64 instruction per SIMD, W waves resident per SIMD: simd_span = (last end - first start) / instructions "
           "of the waves of one SIMD, median over SIMDs; event = kernel time x measured clock / (instructions per wave x W); clock_GHz = delta s_memtime / "
           "delta s_memrealtime\",\n \"ops\": {\n");
    const int Ws[4] = {1, 2, 4, 8};
    const int op_first = (argc > 1 && !strcmp(argv[1], "--new")) ? (int)OP_MAXI : ((argc > 1 && !strcmp(argv[1], "--new2")) ? (int)OP_MINU16 : ((argc > 1 && !strcmp(argv[1], "--new3")) ? (int)OP_MINU16_SDWA : ((argc > 1 && !strcmp(argv[1], "--new4")) ? (int)OP_MULHI : ((argc > 1 && !strcmp(argv[1], "--pk3")) ? (int)OP_PKMAX3F16 : 0))));   // --new ... --new4: only the round-3 additions; --pk3: the packed f16 min3 / max3
    for (int op = op_first; op < OP_COUNT; op++) {
      printf("  \"%s\": {", kNames[op]);
      for (int wi = 0; wi < 4; wi++) {
        const int W = Ws[wi], iters = (op == OP_MULLO || op >= OP_FMA64) ? 4096 : 16384;   // slow ops: shorter runs
        IssueResult r{};
        switch (op) {
#define C(O) case O: r = run_issue<O>(W, iters, d_out, h); break;
          C(OP_MAX3) C(OP_MIN3) C(OP_PERM) C(OP_MUL24) C(OP_MAD24) C(OP_CMP_SOR) C(OP_PKMAX16) C(OP_PKMIN16) C(OP_ADD) C(OP_BCNT) C(OP_ALIGNBYTE)
          C(OP_ANDOR) C(OP_LSHLADD) C(OP_CNDMASK) C(OP_SUBREV) C(OP_DS_READ_U8) C(OP_DS_READ_B32) C(OP_DOT4) C(OP_DOT2) C(OP_SATPK) C(OP_MULLO)
          C(OP_CMP) C(OP_AND) C(OP_LSHL) C(OP_BFE) C(OP_FMA32) C(OP_FMA64) C(OP_ADD64) C(OP_MUL64) C(OP_RCP32) C(OP_CVT)
          C(OP_MAXI) C(OP_MAXU) C(OP_MAXF) C(OP_MINF) C(OP_MAX3F) C(OP_MED3F) C(OP_ADDF) C(OP_SUBF) C(OP_MULF) C(OP_OR) C(OP_XOR) C(OP_OR3) C(OP_ADD3) C(OP_LSHR) C(OP_MOV) C(OP_CMPF) C(OP_CMPU) C(OP_CMPE64) C(OP_SAD8) C(OP_CVTUB) C(OP_PKMAXI16) C(OP_PKADD16) C(OP_PKFMAF16) C(OP_PKMAXF16) C(OP_MAX3F16) C(OP_MBCNT) C(OP_SUBU) C(OP_MAXI16) C(OP_MINU16) C(OP_SUBU16) C(OP_MIN3U16) C(OP_MAX3U16) C(OP_CMPSDWA) C(OP_CMPU16) C(OP_LSHLADD1) C(OP_MINU16_SDWA) C(OP_MAXU16_SDWA) C(OP_SUBU16_SDWA) C(OP_MOV_DPP_WSHR) C(OP_MOV_DPP_ROWSHR) C(OP_DS_READ2_B32) C(OP_MULHI) C(OP_MULHI_U24) C(OP_MUL_U24) C(OP_MED3I) C(OP_PKMAX3F16) C(OP_PKMIN3F16)
#undef C
        }
        printf("\"W%d\": {\"simd_span\": %.3f, \"event\": %.3f, \"clock_GHz\": %.3f, \"waves_sharing_simd\": %.2f}%s", W, r.simd_span, r.event,
               r.clock_ghz, r.share, wi < 3 ? ", " : "");
        fflush(stdout);
      }
      printf("}%s\n", op + 1 < OP_COUNT ? "," : "");
    }
    printf(" },\n");
  } else {
    printf("{\n");
  }
  // ---- streaming reads: 1 GiB each (past the 256 MiB Infinity Cache), every byte once
  const size_t n = (size_t)1 << 30;
  unsigned char* buf;
  unsigned* sink;
  CK(hipMalloc(&buf, n));
  CK(hipMalloc(&sink, 4));
  CK(hipMemset(buf, 1, n));
  CK(hipDeviceSynchronize());
  hipEvent_t e0, e1;
  CK(hipEventCreate(&e0));
  CK(hipEventCreate(&e1));
  float ms[4];
  for (int k = 0; k < 4; k++) {
    CK(hipEventRecord(e0));
    if (k == 0) hipLaunchKernelGGL(k_stream_dwordx4, dim3(256 * 32), dim3(256), 0, 0, (const uint4*)buf, n / 16, sink);
    if (k == 1) hipLaunchKernelGGL(k_stream_dword, dim3(256 * 32), dim3(256), 0, 0, (const unsigned*)buf, n / 4, sink);
    if (k == 2) hipLaunchKernelGGL(k_stream_byte, dim3(256 * 32), dim3(256), 0, 0, buf, n / 4, sink);   // 256 MiB of bytes
    if (k == 3)   // 1024 "frames" of 4096 rows x 1024 B pitch... : tiles of 33 x 80 dwords stepping 30 x 74 (FAST level-0 cell + halo)
      hipLaunchKernelGGL(k_stream_tiles, dim3(5 * 6, 1024 / 16), dim3(256), 0, 0, (const unsigned*)buf, 192, 33, 80, 30, 74, 5, sink);
    CK(hipEventRecord(e1));
    CK(hipEventSynchronize(e1));
    CK(hipEventElapsedTime(&ms[k], e0, e1));
  }
  const double tiles_unique = 64.0 * (4 * 30 + 33) * (5 * 74 + 80) * 4, tiles_issued = 64.0 * 30 * 33 * 80 * 4;
  printf(" \"stream\": {\"k_stream_dwordx4\": {\"bytes\": %zu, \"ms\": %.3f, \"GBps\": %.1f},\n"
         "            \"k_stream_dword\": {\"bytes\": %zu, \"ms\": %.3f, \"GBps\": %.1f},\n"
         "            \"k_stream_byte\": {\"bytes\": %zu, \"ms\": %.3f, \"GBps\": %.1f},\n"
         "            \"k_stream_tiles\": {\"bytes_unique\": %.0f, \"bytes_issued\": %.0f, \"ms\": %.3f}}\n}\n",
         n, ms[0], n / ms[0] / 1e6, n, ms[1], n / ms[1] / 1e6, n / 4, ms[2], n / 4 / ms[2] / 1e6, tiles_unique, tiles_issued, ms[3]);
  return 0;
}
