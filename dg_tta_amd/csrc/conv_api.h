// Pointer-level functions of the network building blocks that are defined in one translation unit and called from another:
// each is declared here, once; the defining file includes this header too, so the compiler sees declaration and definition
// together.  (The View / Taps-level launchers of the MFMA units and their launch descriptor are in conv_common.h.)
// The convolution functions take one problem descriptor (ConvProblem, which the extern "C" entry points fill once) plus their
// operands (Src / Dst / Region).  Also what those entry points share: the argument checks (CONV_REQUIRE_*), the workspace layouts
// (one function each for the size query and the launcher that carves the workspace), and the small host helpers: element /
// granule / output sizes (the dtype fan-out, DISPATCH_T, is in common.h).  Needs only common.h.
#pragma once
#include "common.h"

// ---------------------------------------------------------------------------------------------------- host helpers
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

// ---------------------------------------------------------------------------------------------------- problem descriptor
// One convolution as the entry points hand it down.  [kd, 3, 3] kernel with padding (kd / 2, 1, 1) and strides (sd, sh, sw); the
// 3x3x3 family fills kd = 3, sd = sh = sw = stride.  Transposed convs (kernel = stride): Di, Hi, Wi is the INPUT lattice, the output
// lattice is s * Di (Dt / Ht / Wt), kd = sd.  Cin / Cout are always the layer's; CinP / CoutP the padded counts of its weight blob
// (the layer's own where there is no blob).  dry: no launch, DGTTA_OK iff the ring kernel would take the call
// (dgtta_conv3d_k3_blocked_supported).
struct ConvProblem {
  int B, Cin, Cout, CinP, CoutP, Di, Hi, Wi, kd, sd, sh, sw, dtype;
  hipStream_t st;
  bool dry = false;
  int Do() const { return out_dim(Di, sd, kd); }
  int Ho() const { return out_dim(Hi, sh); }
  int Wo() const { return out_dim(Wi, sw); }
  int64_t in_vox() const { return (int64_t)Di * Hi * Wi; }          // voxels per sample
  int64_t out_vox() const { return (int64_t)Do() * Ho() * Wo(); }
  int ntaps() const { return kd * 9; }
  // transposed conv: output lattice and output offsets per input voxel
  int Dt() const { return sd * Di; }
  int Ht() const { return sh * Hi; }
  int Wt() const { return sw * Wi; }
  int noff() const { return sd * sh * sw; }
  int64_t t_vox() const { return in_vox() * noff(); }
  bool even_strided() const { return (sd == 1 || Di % 2 == 0) && (sh == 1 || Hi % 2 == 0) && (sw == 1 || Wi % 2 == 0); }
};
// A stride-1 data gradient is the forward conv of dy with the mirrored, transposed weights, and every data-gradient launch is a
// GEMM whose K is the layer's Cout and whose N is its Cin: the problem as the forward-shaped code below wants it.
static inline ConvProblem dgrad_as_fwd(const ConvProblem &P) {
  ConvProblem Q = P;
  Q.Cin = P.Cout, Q.Cout = P.Cin, Q.CinP = P.CoutP, Q.CoutP = P.CinP;
  return Q;
}

// operands: channels-last rows of ld elements.  kh != 0: the rows hold one 32-channel block (ld = 32) and the blocks lie as dense
// planes kh elements apart - only the ring kernels read that layout
struct Src { const void *p; int ld; long long kh = 0; };
struct Dst { void *p; int ld; };
struct Region { void *p; size_t bytes; };      // a piece of workspace

// ---------------------------------------------------------------------------------------------------- argument checks
// What the conv entry points test, each in the words it is reported with; fn: the entry point's name without the dgtta_ prefix.
// A failed check leaves its message in dgtta_last_error() and returns its code from the entry point.
static inline bool stride_ok(int s) { return s == 1 || s == 2; }
static inline bool kernel_ok(const ConvProblem &P) { return (P.kd == 1 || P.kd == 3) && stride_ok(P.sd) && stride_ok(P.sh) && stride_ok(P.sw); }
static inline bool convt_strides_ok(const ConvProblem &P) { return stride_ok(P.sd) && stride_ok(P.sh) && stride_ok(P.sw) && P.noff() > 1; }
// positive extents, padded channel counts that hold the real ones; cap: the general family also bounds the channel counts (the
// size queries answer 0 where this fails)
static inline bool conv_dims_ok(const ConvProblem &P, bool cap) {
  return P.B > 0 && P.Cin > 0 && P.Cout > 0 && P.Di > 0 && P.Hi > 0 && P.Wi > 0 && P.CinP >= P.Cin && P.CoutP >= P.Cout &&
         (!cap || (P.Cin <= (1 << 16) && P.Cout <= (1 << 16)));
}
#define CONV_REQUIRE_PTRS(fn, all) DG_REQUIRE(all, DGTTA_ERR_BADARG, "%s: null pointer", fn)
// lds: the rows of the operands, for the entry points that report short rows as bad dims (the others: CONV_REQUIRE_LD)
#define CONV_REQUIRE_DIMS(fn, P, cap, lds) DG_REQUIRE(conv_dims_ok(P, cap) && (lds), DGTTA_ERR_BADARG, "%s: bad dims", fn)
#define CONV_REQUIRE_LD(fn, ok) DG_REQUIRE(ok, DGTTA_ERR_BADARG, "%s: ld < C", fn)
#define CONV_REQUIRE_K3_STRIDE(fn, P) DG_REQUIRE(stride_ok((P).sd), DGTTA_ERR_UNSUPPORTED, "%s: stride %d", fn, (P).sd)
#define CONV_REQUIRE_KERNEL(fn, P)                                                                                                     \
  DG_REQUIRE(kernel_ok(P) && dtype_ok((P).dtype), DGTTA_ERR_UNSUPPORTED, "%s: kernel %dx3x3, stride (%d,%d,%d), dtype %d not supported", fn, \
             (P).kd, (P).sd, (P).sh, (P).sw, (P).dtype)
#define CONV_REQUIRE_CONVT_STRIDES(fn, P)                                                                                            \
  DG_REQUIRE(convt_strides_ok(P) && dtype_ok((P).dtype), DGTTA_ERR_UNSUPPORTED, "%s: kernel = stride (%d,%d,%d), dtype %d not supported", fn, \
             (P).sd, (P).sh, (P).sw, (P).dtype)
#define CONV_REQUIRE_EVEN(fn, P)                                                                                                      \
  DG_REQUIRE((P).even_strided(), DGTTA_ERR_UNSUPPORTED, "%s: strided axes need even input extents (%dx%dx%d)", fn, (P).Di, (P).Hi, (P).Wi)
#define CONV_REQUIRE_WS(fn, have, need) DG_REQUIRE((have) >= (need), DGTTA_ERR_WORKSPACE, "%s: workspace too small", fn)

// ---------------------------------------------------------------------------------------------------- conv_mfma.hip
// MFMA implementations; return DGTTA_ERR_UNSUPPORTED when the shape is not covered.
// conv3_fwd_mfma: w_kmajor is the forward or (mirror) the backward weight image; gst: the InstanceNorm-backward context of
// dgtta_conv3d_k3_dgrad_gstats or null
int conv3_fwd_mfma(const ConvProblem &P, Src x, const void *w_kmajor, int mirror, const float *bias, Dst y, double *stats,
                   RowsGstCtx *gst);
int conv3_dgrad_s2_mfma(const ConvProblem &P, Src dy, const void *w_kmajor, Dst dx, int accumulate);
int64_t conv3_mfma_max_tiles(int Do, int Ho, int Wo);
size_t conv_image_bytes(int CinP, int CoutP, int dtype);
size_t conv_imgB_offset_bytes(int CinP, int CoutP, int dtype);
// torch [Cout][Cin][ntaps] fp32 -> image-ordered [imgF | imgB] (P.ntaps(): 27, or kd * 9 for the anisotropic kernels)
int conv_pack_images(const ConvProblem &P, const float *w_t, void *img);
size_t convT_packed_bytes(int CinP, int CoutP, int dtype);
// workspace region of a transposed conv's packed weights (channel counts padded to the granule)
static inline size_t convT_pack_region(int Cin, int Cout, int dtype) {
  const int g = conv_granule(dtype);
  return align_up(convT_packed_bytes((Cin + g - 1) / g * g, (Cout + g - 1) / g * g, dtype), 256);
}
// transposed convs; mode 0: forward (in = x, out), mode 1: data gradient (in = dout, out = dx); ws: the packed-weights region
int convT_fwd_mfma(const ConvProblem &P, Src x, const float *w_t, const float *bias, Dst out, void *ws);
int convT_dgrad_mfma(const ConvProblem &P, Src dout, const float *w_t, Dst dx, void *ws);
int convTa_run(const ConvProblem &P, int mode, Src in, const float *w_t, const float *bias, Dst out, void *ws);

// ---------------------------------------------------------------------------------------------------- convt_gemm.hip
// register-operand kernels of the two large decoder stages
bool convT_gemm_eligible(const ConvProblem &P, Src in, Dst out);
int convT_gemm_run(const ConvProblem &P, int mode, Src in, const float *w_t, const float *bias, Dst out, void *ws);

// ---------------------------------------------------------------------------------------------------- conv_wgrad.hip
// weight gradients on the matrix cores (the View-level launchers of these units are in conv_wgrad_common.h); ws: the main region
int conv3_wgrad_mfma(const ConvProblem &P, Src x, Src dy, float *dw_t, Region ws, int accumulate);
size_t conv3_wgrad_mfma_ws_bytes(int B, int Cin, int Cout, int D, int H, int W);
size_t conv3_wgrad_split_extra_bytes(int B, int Cin, int Cout, int D, int H, int W, int stride);
bool conv3_wgrad_blocked_ok(const ConvProblem &P);
size_t conva_wgrad_ws_bytes(int B, int Cin, int Cout, int D, int H, int W);
int conva_wgrad_mfma(const ConvProblem &P, Src x, Src dy, float *dw_t, Region ws, int accumulate);

// ---------------------------------------------------------------------------------------------------- convt_wgrad.hip
// bias_part / bias_units (optional): room for the bias gradient's partial sums, see the definition
int convT_wgrad_mfma(const ConvProblem &P, Src x, Src dout, float *dw_t, Region ws, int accumulate, Region bias_part, int *bias_units);
int convT_bias_finalize(const float *part, int units, int Cout, float *db, int accumulate, hipStream_t st);
size_t convT_wgrad_split_extra_bytes(int B, int Cin, int Cout, int Di, int Hi, int Wi);
int convTa_wgrad_mfma(const ConvProblem &P, Src x, Src dout, float *dw_t, Region ws, int accumulate);

// ---------------------------------------------------------------------------------------------------- head_wgrad.hip
size_t head_wgrad_mfma_ws_bytes(int Cin, int nsel, int64_t rows);
int head_wgrad_mfma(const void *x, int ldx, const float *dout, int lddo, float *dw_sel, void *ws, size_t ws_bytes, int Cin,
                    int nsel, int64_t rows, int accumulate, int dtype, hipStream_t st, bool have_d16,
                    const unsigned short *d16_ext = nullptr);

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
int conv3_pack_weights_ref(const ConvProblem &P, const float *w_t, void *wf, void *wb);
int conv3_fwd_ref(const ConvProblem &P, Src x, const void *wf, const float *bias, Dst y);
int conv3_dgrad_ref(const ConvProblem &P, Src dy, const void *wb, Dst dx, int accumulate);
int conv3_wgrad_ref(const ConvProblem &P, Src x, Src dy, float *part, int nsplit, float *dw_t, int accumulate);
int convT_fwd_ref(const ConvProblem &P, Src x, const float *w_t, const float *bias, Dst out);
int convT_dgrad_ref(const ConvProblem &P, Src dout, const float *w_t, Dst dx);
int convT_wgrad_ref(const ConvProblem &P, Src x, Src dout, float *part, int nsplit, float *dw_t, int accumulate);
// out[i] (+)= sum over k < nsplit of part[k][i], in order
int reduce_splits(const float *part, float *out, int64_t n, int nsplit, int accumulate, hipStream_t st);

// ---------------------------------------------------------------------------------------------------- instnorm.hip
// InstanceNorm statistics of y by a reduction pass of their own, in the layout of dgtta_conv3d_stats_bytes
int conv_stats_ref(const void *y, int ldy, void *stats, int B, int C, int64_t V, int dtype, hipStream_t st);
// db[c] (+)= sum over the B x V rows of dy, fixed order
size_t conv_bias_grad_ws_bytes(int B, int C, int64_t V);
int conv_bias_grad(const void *dy, int lddy, float *db, void *ws, int B, int C, int64_t V, int accumulate, int dtype,
                   hipStream_t st);

// ---------------------------------------------------------------------------------------------------- workspace layouts
// [bias partials][packed weights][main]: region sizes, each a multiple of 256 bytes, in the order they lie in the workspace.  The
// size queries return total(), the launchers carve their pointers with the accessors: one layout serves both.
struct ConvWsLayout {
  size_t bias, pack, main;
  size_t total() const { return bias + pack + main; }
  void *pack_of(void *ws) const { return (char *)ws + bias; }
  // the launchers hand the main region everything the caller gave beyond it (the fp32 split planes, when offered)
  Region main_of(void *ws, size_t ws_bytes) const { return {(char *)ws + bias + pack, ws_bytes - bias - pack}; }
};
// split partials of the VALU weight-gradient kernels: one per 4096 voxels, at most 64
static inline int wgrad_splits(int64_t nvox) {
  int64_t s = cdiv64(nvox, 4096);
  return (int)(s < 64 ? (s > 0 ? s : 1) : 64);
}
static inline size_t conv_bias_region(int B, int Cout, int64_t V) { return align_up(conv_bias_grad_ws_bytes(B, Cout, V), 256); }
// Conv weight gradient, [bias partials][main].  3x3x3 family: main = split partials of the VALU kernel | slabs of the MFMA kernel;
// split_stride != 0: followed by the room that lets an fp32 gradient of a layer of that stride run as six 16-bit launches on bf16
// split planes (three planes of x, split_stride x the output extent, and three of dy behind the 256-aligned slab region,
// conv_wgrad.hip).  General family: main = the slabs of any class count.  (The size queries of the 3x3x3 family are given the
// OUTPUT extent: they ask with it as a stride-1 problem.)
static inline ConvWsLayout conv_wgrad_ws_layout(const ConvProblem &P, bool general, int split_stride = 0) {
  const int Do = P.Do(), Ho = P.Ho(), Wo = P.Wo();
  const size_t bias = conv_bias_region(P.B, P.Cout, P.out_vox());
  if (general) return {bias, 0, align_up(conva_wgrad_ws_bytes(P.B, P.Cin, P.Cout, Do, Ho, Wo), 256)};
  const size_t a = align_up((size_t)wgrad_splits(P.B * P.out_vox()) * P.Cout * P.Cin * 27 * sizeof(float), 256);
  const size_t c = align_up(conv3_wgrad_mfma_ws_bytes(P.B, P.Cin, P.Cout, Do, Ho, Wo), 256);
  return {bias, 0, (a > c ? a : c) + (split_stride ? 256 + conv3_wgrad_split_extra_bytes(P.B, P.Cin, P.Cout, Do, Ho, Wo, split_stride) : 0)};
}
// Transposed conv backward, [bias partials][packed weights][main].  k2s2 (general = false): main = split partials (VALU) | slabs
// (MFMA), with `split` the slabs followed by the fp32 gradient's bf16 split planes.  Kernel = stride: main = the slabs.
static inline ConvWsLayout convT_bwd_ws_layout(const ConvProblem &P, bool general, bool split = false) {
  const size_t bias = conv_bias_region(P.B, P.Cout, P.t_vox()), pack = convT_pack_region(P.Cin, P.Cout, DGTTA_F32);
  if (general) return {bias, pack, align_up(conva_wgrad_ws_bytes(P.B, P.Cin, P.Cout, P.Di, P.Hi, P.Wi), 256)};
  const size_t a = align_up((size_t)wgrad_splits(P.B * P.in_vox()) * P.Cin * P.Cout * 8 * sizeof(float), 256);
  const size_t c = align_up(conv3_wgrad_mfma_ws_bytes(P.B, P.Cin, P.Cout, P.Di, P.Hi, P.Wi), 256) +
                   (split ? convT_wgrad_split_extra_bytes(P.B, P.Cin, P.Cout, P.Di, P.Hi, P.Wi) : 0);
  return {bias, pack, a > c ? a : c};
}
