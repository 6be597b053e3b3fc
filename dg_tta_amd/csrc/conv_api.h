// Pointer-level functions of the network building blocks that are defined in one translation unit and called from another:
// each is declared here, once; the defining file includes this header too, so the compiler sees declaration and definition
// together.  (The View / Taps-level launchers of the MFMA units and their launch descriptor are in conv_common.h.)
// Also the small host helpers those units share: the dtype fan-out, element / granule / output sizes.  Needs only common.h.
#pragma once
#include "common.h"

// ---------------------------------------------------------------------------------------------------- host helpers
// runs CALL with T = the storage type of `dtype`; an unknown dtype returns DGTTA_ERR_BADARG from the enclosing function
#define DISPATCH_T(dtype, CALL)                                                        \
  do {                                                                                 \
    if ((dtype) == DGTTA_F32) {                                                        \
      typedef float T;                                                                 \
      CALL;                                                                            \
    } else if ((dtype) == DGTTA_BF16) {                                                \
      typedef bf16_t T;                                                                \
      CALL;                                                                            \
    } else if ((dtype) == DGTTA_F16) {                                                 \
      typedef f16_t T;                                                                 \
      CALL;                                                                            \
    } else {                                                                           \
      dgtta_set_error("bad dtype %d", (int)(dtype));                                   \
      return DGTTA_ERR_BADARG;                                                         \
    }                                                                                  \
  } while (0)

static inline bool dtype_ok(int dtype) { return dtype == DGTTA_F32 || dtype == DGTTA_BF16 || dtype == DGTTA_F16; }
static inline size_t esize(int dtype) { return dtype == DGTTA_F32 ? 4 : 2; }      // bytes per stored element

static inline int conv_granule(int dtype) { return dtype == DGTTA_F32 ? 8 : 16; } // padded channel counts of the MFMA kernels: 32 bytes
static inline size_t n32(int c) { return (size_t)(c + 31) / 32 * 32; }            // weight images: whole 32-channel N blocks

static inline int out_dim(int i, int s, int k = 3) { return (i + 2 * (k / 2) - k) / s + 1; }   // extent-k conv, padding k / 2, stride s

static inline int gs_blocks(int64_t total, int cap = 16384) {                     // grid of a grid-stride loop, 256 threads
  int64_t b = (total + 255) / 256;
  return (int)(b < cap ? (b > 0 ? b : 1) : cap);
}

// per-channel reductions: >= 32 rows per block (small volumes used to run on 1-4 workgroups) and about 4096 workgroups
// per launch over the whole batch: 16 per CU keep an HBM stream saturated, while the finalize kernels that read the
// B x nblk partial rows stay short (with 2048 blocks per SAMPLE at batch 8 they took 30-84 us each, ~5 ms per epoch)
static inline int reduce_blocks(int64_t V, int B) {
  int64_t b = cdiv64(V, 32);
  int64_t cap = 4096 / (B > 0 ? B : 1);
  if (cap < 128) cap = 128;
  if (cap > 2048) cap = 2048;
  return (int)(b < cap ? (b > 0 ? b : 1) : cap);
}

// ---------------------------------------------------------------------------------------------------- conv_mfma.hip
// MFMA implementations; return DGTTA_ERR_UNSUPPORTED when the shape is not covered.
int conv3_fwd_mfma(const void *x, int ldx, const void *w_kmajor, int mirror, const float *bias, void *y, int ldy, int B,
                   int Cin, int Cout, int CinP, int CoutP, int Di, int Hi, int Wi, int stride, int dtype,
                   hipStream_t st, double *stats, RowsGstCtx *gst, long long xkh, bool dry);
int conv3_dgrad_s2_mfma(const void *dy, int lddy, const void *w_kmajor, void *dx, int lddx, int B, int Cin, int Cout,
                        int CinP, int CoutP, int Di, int Hi, int Wi, int accumulate, int dtype, hipStream_t st);
int64_t conv3_mfma_max_tiles(int Do, int Ho, int Wo);
size_t conv_image_bytes(int CinP, int CoutP, int dtype);
size_t conv_imgB_offset_bytes(int CinP, int CoutP, int dtype);
// torch [Cout][Cin][ntaps] fp32 -> image-ordered [imgF | imgB] (ntaps = 27, or kd * 9 for the anisotropic kernels)
int conv_pack_images(const float *w_t, void *img, int ntaps, int Cin, int Cout, int CinP, int CoutP, int dtype, hipStream_t st);
size_t convT_packed_bytes(int CinP, int CoutP, int dtype);
// workspace region of a transposed conv's packed weights (channel counts padded to the granule)
static inline size_t convT_pack_region(int Cin, int Cout, int dtype) {
  const int g = conv_granule(dtype);
  return align_up(convT_packed_bytes((Cin + g - 1) / g * g, (Cout + g - 1) / g * g, dtype), 256);
}
int convT_fwd_mfma(const void *x, int ldx, const float *w_t, const float *bias, void *out, int ldo, void *ws, int B, int Cin,
                   int Cout, int Di, int Hi, int Wi, int dtype, hipStream_t st);
int convT_dgrad_mfma(const void *dout, int lddo, const float *w_t, void *dx, int lddx, void *ws, int B, int Cin, int Cout,
                     int Di, int Hi, int Wi, int dtype, hipStream_t st);
int convTa_run(int mode, const void *in, int ldin, const float *w_t, const float *bias, void *out, int ldout, void *ws, int B,
               int Cin, int Cout, int Di, int Hi, int Wi, int sd, int sh, int sw, int dtype, hipStream_t st);

// ---------------------------------------------------------------------------------------------------- convt_gemm.hip
// register-operand kernels of the two large decoder stages
bool convT_gemm_eligible(int mode, const void *in, int ldin, const void *out, int ldout, int Cin, int Cout, int Wi, int dtype);
int convT_gemm_run(int mode, const void *in, int ldin, const float *w_t, const float *bias, void *out, int ldout, void *ws, int B,
                   int Cin, int Cout, int Di, int Hi, int Wi, int dtype, hipStream_t st);

// ---------------------------------------------------------------------------------------------------- conv_wgrad.hip
// weight gradients on the matrix cores (the View-level launchers of these units are in conv_wgrad_common.h)
int conv3_wgrad_mfma(const void *x, int ldx, const void *dy, int lddy, float *dw_t, void *ws, size_t ws_bytes, int B, int Cin,
                     int Cout, int Di, int Hi, int Wi, int stride, int accumulate, int dtype, hipStream_t st, long long xkh);
size_t conv3_wgrad_mfma_ws_bytes(int B, int Cin, int Cout, int D, int H, int W);
size_t conv3_wgrad_split_extra_bytes(int B, int Cin, int Cout, int D, int H, int W, int stride);
bool conv3_wgrad_blocked_ok(int B, int Cin, int Cout, int D, int H, int W, int dtype);
size_t conva_wgrad_ws_bytes(int B, int Cin, int Cout, int D, int H, int W);
int conva_wgrad_mfma(const void *x, int ldx, const void *dy, int lddy, float *dw_t, void *ws, size_t ws_bytes, int B, int Cin,
                     int Cout, int Di, int Hi, int Wi, int kd, int sd, int sh, int sw, int accumulate, int dtype, hipStream_t st);

// ---------------------------------------------------------------------------------------------------- convt_wgrad.hip
int convT_wgrad_mfma(const void *x, int ldx, const void *dout, int lddo, float *dw_t, void *ws, size_t ws_bytes, int B,
                     int Cin, int Cout, int Di, int Hi, int Wi, int accumulate, int dtype, hipStream_t st, float *bias_part,
                     size_t bias_part_bytes, int *bias_units);
int convT_bias_finalize(const float *part, int units, int Cout, float *db, int accumulate, hipStream_t st);
size_t convT_wgrad_split_extra_bytes(int B, int Cin, int Cout, int Di, int Hi, int Wi);
int convTa_wgrad_mfma(const void *x, int ldx, const void *dout, int lddo, float *dw_t, void *ws, size_t ws_bytes, int B, int Cin,
                      int Cout, int Di, int Hi, int Wi, int sd, int sh, int sw, int accumulate, int dtype, hipStream_t st);

// ---------------------------------------------------------------------------------------------------- head_wgrad.hip
size_t head_wgrad_mfma_ws_bytes(int Cin, int nsel, int64_t rows);
int head_wgrad_mfma(const void *x, int ldx, const float *dout, int lddo, float *dw_sel, void *ws, size_t ws_bytes, int Cin,
                    int nsel, int64_t rows, int accumulate, int dtype, hipStream_t st, bool have_d16);

// ---------------------------------------------------------------------------------------------------- seghead_mfma.hip
// 1x1x1 heads with Cin a multiple of 32 (32..320), nsel <= 128, 16-bit storage; DGTTA_ERR_UNSUPPORTED for anything else
int head_fwd_mfma(const void *x, int ldx, const float *w, const float *bias, const int *sel, int nsel, float *out, int ldo, int Cin,
                  int64_t rows, int dtype, hipStream_t st);
int head_dgrad_mfma(const float *dout, int lddo, const float *w, const int *sel, int nsel, void *dx, int lddx, int Cin, int64_t rows,
                    int accumulate_dx, int dtype, hipStream_t st);
int head_wgrad_rows_mfma(const void *x, int ldx, const float *dout, int lddo, float *part, int nsplit, int nsel, int Cin, int64_t rows,
                         int dtype, hipStream_t st);

// ---------------------------------------------------------------------------------------------------- conv_ref.hip
// launchers of the general-shape VALU kernels: every Cin / Cout / ld; the weight gradients leave nsplit partial sums in
// `part` and add them up in order into dw_t
int conv3_pack_weights_ref(const float *w_t, void *wf, void *wb, int Cin, int Cout, int CinP, int CoutP, int dtype,
                           hipStream_t st);
int conv3_fwd_ref(const void *x, int ldx, const void *wf, const float *bias, void *y, int ldy, int B, int Cin, int Cout,
                  int CinP, int CoutP, int Di, int Hi, int Wi, int stride, int dtype, hipStream_t st);
int conv3_dgrad_ref(const void *dy, int lddy, const void *wb, void *dx, int lddx, int B, int Cin, int Cout, int CinP,
                    int CoutP, int Di, int Hi, int Wi, int stride, int accumulate, int dtype, hipStream_t st);
int conv3_wgrad_ref(const void *x, int ldx, const void *dy, int lddy, float *part, int nsplit, float *dw_t, int B, int Cin,
                    int Cout, int Di, int Hi, int Wi, int stride, int accumulate, int dtype, hipStream_t st);
int convT_fwd_ref(const void *x, int ldx, const float *w_t, const float *bias, void *out, int ldo, int B, int Cin, int Cout,
                  int Di, int Hi, int Wi, int dtype, hipStream_t st);
int convT_dgrad_ref(const void *dout, int lddo, const float *w_t, void *dx, int lddx, int B, int Cin, int Cout, int Di,
                    int Hi, int Wi, int dtype, hipStream_t st);
int convT_wgrad_ref(const void *x, int ldx, const void *dout, int lddo, float *part, int nsplit, float *dw_t, int B, int Cin,
                    int Cout, int Di, int Hi, int Wi, int accumulate, int dtype, hipStream_t st);
// out[i] (+)= sum over k < nsplit of part[k][i], in order
int reduce_splits(const float *part, float *out, int64_t n, int nsplit, int accumulate, hipStream_t st);

// ---------------------------------------------------------------------------------------------------- instnorm.hip
// InstanceNorm statistics of y by a reduction pass of their own, in the layout of dgtta_conv3d_stats_bytes
int conv_stats_ref(const void *y, int ldy, void *stats, int B, int C, int64_t V, int dtype, hipStream_t st);
// db[c] (+)= sum over the B x V rows of dy, fixed order
size_t conv_bias_grad_ws_bytes(int B, int C, int64_t V);
int conv_bias_grad(const void *dy, int lddy, float *db, void *ws, int B, int C, int64_t V, int accumulate, int dtype,
                   hipStream_t st);
