// C ABI of the 3x3x3 convolutions and the 2x2x2 transposed convolutions (dgtta_conv3d_*, dgtta_convT3d_*): argument
// checks, weight-blob and workspace layout, and the choice of kernel - the MFMA implementations (conv_mfma.hip,
// conv_wgrad.hip, which pick between the ring / row-reuse / generic tile kernels themselves) first, the general-shape
// VALU kernels of conv_ref.hip for what they return DGTTA_ERR_UNSUPPORTED for (impl 0), or one of the two alone
// (impl 2 / impl 1: the tests' cross-check).  Host code only: every kernel lives in the unit its launcher is declared for.
#include "conv_api.h"

static int wgrad_splits(int64_t nvox) {
  int64_t s = cdiv64(nvox, 4096);
  return (int)(s < 64 ? (s > 0 ? s : 1) : 64);
}

static const void *wb_of(const void *wpack, int CinP, int CoutP, int dtype) {
  return (const char *)wpack + (size_t)27 * CinP * CoutP * esize(dtype);
}

// blob = [wf | wb] (general kernels) followed by [imgF | imgB] (LDS-image order for the MFMA kernels)
static const void *img_of(const void *wpack, int CinP, int CoutP, int dtype) {
  return (const char *)wpack + (size_t)2 * 27 * CinP * CoutP * esize(dtype);
}
static const void *imgB_of(const void *wpack, int CinP, int CoutP, int dtype) {
  return (const char *)img_of(wpack, CinP, CoutP, dtype) + conv_imgB_offset_bytes(CinP, CoutP, dtype);
}

extern "C" size_t dgtta_conv3d_packed_bytes(int CinP, int CoutP, int dtype) {
  if (CinP <= 0 || CoutP <= 0) return 0;      // a size query of an empty problem (the launchers reject it with DGTTA_ERR_BADARG)
  return (size_t)2 * 27 * CinP * CoutP * esize(dtype) + conv_image_bytes(CinP, CoutP, dtype);
}

extern "C" int dgtta_conv3d_pack_weights(const float *w_t, void *wpack, int Cin, int Cout, int CinP, int CoutP,
                                         int dtype, void *stream) {
  DG_REQUIRE(w_t && wpack, DGTTA_ERR_BADARG, "pack_weights: null pointer");
  void *wf = wpack;
  void *wb = const_cast<void *>(wb_of(wpack, CinP, CoutP, dtype));
  DG_REQUIRE(Cin > 0 && Cout > 0 && CinP >= Cin && CoutP >= Cout, DGTTA_ERR_BADARG, "pack_weights: bad channel counts");
  const int rc = conv3_pack_weights_ref(w_t, wf, wb, Cin, Cout, CinP, CoutP, dtype, (hipStream_t)stream);
  if (rc != DGTTA_OK) return rc;
  if (CinP % conv_granule(dtype) == 0 && CoutP % conv_granule(dtype) == 0)
    return conv_pack_images(w_t, const_cast<void *>(img_of(wpack, CinP, CoutP, dtype)), 27, Cin, Cout, CinP, CoutP, dtype,
                            (hipStream_t)stream);
  return DGTTA_OK;
}

// statistics buffer: [256-byte header: int64 nblk][partial sums: B x nblk x Cout x 2 doubles]
extern "C" size_t dgtta_conv3d_stats_bytes(int B, int Cout, int Do, int Ho, int Wo) {
  if (B <= 0 || Cout <= 0 || Do <= 0 || Ho <= 0 || Wo <= 0) return 0;      // a size query of an empty problem (the launchers reject it with DGTTA_ERR_BADARG)
  int64_t nb = conv3_mfma_max_tiles(Do, Ho, Wo);
  const int64_t rb = reduce_blocks((int64_t)Do * Ho * Wo, B);
  if (rb > nb) nb = rb;
  return 256 + (size_t)B * nb * Cout * 2 * sizeof(double);
}

static int k3_fwd(const void *x, int ldx, long long x_block_stride, const void *wpack, const float *bias, void *y, int ldy,
                  void *stats, int B, int Cin, int Cout, int CinP, int CoutP, int Di, int Hi, int Wi, int stride, int dtype, int impl,
                  void *stream) {
  DG_REQUIRE(x && wpack && y, DGTTA_ERR_BADARG, "conv3d_k3_fwd: null pointer");
  const void *wf = wpack;
  DG_REQUIRE(B > 0 && Cin > 0 && Cout > 0 && CinP >= Cin && CoutP >= Cout && Di > 0 && Hi > 0 && Wi > 0,
             DGTTA_ERR_BADARG, "conv3d_k3_fwd: bad dims");
  DG_REQUIRE(stride == 1 || stride == 2, DGTTA_ERR_UNSUPPORTED, "conv3d_k3_fwd: stride %d", stride);
  DG_REQUIRE((x_block_stride ? 2 * ldx : ldx) >= Cin && ldy >= Cout, DGTTA_ERR_BADARG, "conv3d_k3_fwd: ld < C");
  hipStream_t st = (hipStream_t)stream;
  if (impl != 1) {
    int rc = conv3_fwd_mfma(x, ldx, img_of(wpack, CinP, CoutP, dtype), 0, bias, y, ldy, B, Cin, Cout, CinP, CoutP, Di, Hi,
                            Wi, stride, dtype, st, (double *)stats, nullptr, x_block_stride, false);
    if (rc != DGTTA_ERR_UNSUPPORTED) return rc;
    DG_REQUIRE(x_block_stride == 0, DGTTA_ERR_UNSUPPORTED,
               "conv3d_k3_fwd_blocked: only the D-ring kernel reads x as 32-channel planes (ask dgtta_conv3d_k3_blocked_supported)");
    DG_REQUIRE(impl == 0, DGTTA_ERR_UNSUPPORTED, "conv3d_k3_fwd: shape not covered by the MFMA kernel");
  }
  int rc = conv3_fwd_ref(x, ldx, wf, bias, y, ldy, B, Cin, Cout, CinP, CoutP, Di, Hi, Wi, stride, dtype, st);
  if (rc != DGTTA_OK) return rc;
  if (stats) {   // general kernel: statistics by a separate reduction pass, same buffer layout
    const int64_t V = (int64_t)out_dim(Di, stride) * out_dim(Hi, stride) * out_dim(Wi, stride);
    return conv_stats_ref(y, ldy, stats, B, Cout, V, dtype, st);
  }
  return DGTTA_OK;
}

extern "C" int dgtta_conv3d_k3_fwd(const void *x, int ldx, const void *wpack, const float *bias, void *y, int ldy,
                                   void *stats, int B, int Cin, int Cout, int CinP, int CoutP, int Di, int Hi, int Wi,
                                   int stride, int dtype, int impl, void *stream) {
  return k3_fwd(x, ldx, 0, wpack, bias, y, ldy, stats, B, Cin, Cout, CinP, CoutP, Di, Hi, Wi, stride, dtype, impl, stream);
}

// Round 6: x as 32-channel BLOCKS - block c of the input channels is a dense tensor [B][D][H][W][32] (ldx = 32) at element
// offset c * x_block_stride from x.  The level-0 concat buffer of the U-Net is kept that way ([up | skip] as two planes): the
// kernels that read ONE half of it (the stride-2 conv of the skip, the transposed conv's backward) then use whole 128-byte lines.
// Only the D-ring kernels read this layout (64 input channels, 16-bit storage, launches they take): ask
// dgtta_conv3d_k3_blocked_supported first; anything else returns DGTTA_ERR_UNSUPPORTED and launches nothing.
extern "C" int dgtta_conv3d_k3_blocked_supported(int B, int Cin, int Cout, int D, int H, int W, int dtype) {
  if (B <= 0 || Cin != 64 || Cout <= 0 || Cout % 32 || D <= 0 || H <= 0 || W <= 0) return 0;
  if (dtype != DGTTA_BF16 && dtype != DGTTA_F16) return 0;
  const int rc = conv3_fwd_mfma((const void *)16, 32, (const void *)16, 0, nullptr, (void *)16, Cout, B, Cin, Cout, Cin, Cout, D, H, W, 1,
                                dtype, nullptr, nullptr, nullptr, (long long)B * D * H * W * 32, true);
  return rc == DGTTA_OK && conv3_wgrad_blocked_ok(B, Cin, Cout, D, H, W, dtype);
}

extern "C" int dgtta_conv3d_k3_fwd_blocked(const void *x, long long x_block_stride, const void *wpack, const float *bias, void *y,
                                           int ldy, void *stats, int B, int Cin, int Cout, int CinP, int CoutP, int Di, int Hi,
                                           int Wi, int dtype, void *stream) {
  DG_REQUIRE(x_block_stride > 0 && x_block_stride % 8 == 0, DGTTA_ERR_BADARG, "conv3d_k3_fwd_blocked: block stride must be a positive multiple of 8 elements");
  return k3_fwd(x, 32, x_block_stride, wpack, bias, y, ldy, stats, B, Cin, Cout, CinP, CoutP, Di, Hi, Wi, 1, dtype, 0, stream);
}

// gst: the InstanceNorm-backward context of dgtta_conv3d_k3_dgrad_gstats (null for the plain data gradient); it travels down
// the dispatch chain as an argument and only the ring / row-reuse launchers act on it
static int k3_dgrad(const void *dy, int lddy, const void *wpack, void *dx, int lddx, int B, int Cin, int Cout, int CinP, int CoutP,
                    int Di, int Hi, int Wi, int stride, int accumulate, int dtype, int impl, void *stream, RowsGstCtx *gst) {
  DG_REQUIRE(dy && wpack && dx, DGTTA_ERR_BADARG, "conv3d_k3_dgrad: null pointer");
  const void *wb = wb_of(wpack, CinP, CoutP, dtype);
  DG_REQUIRE(B > 0 && Cin > 0 && Cout > 0 && CinP >= Cin && CoutP >= Cout && Di > 0 && Hi > 0 && Wi > 0,
             DGTTA_ERR_BADARG, "conv3d_k3_dgrad: bad dims");
  DG_REQUIRE(stride == 1 || stride == 2, DGTTA_ERR_UNSUPPORTED, "conv3d_k3_dgrad: stride %d", stride);
  DG_REQUIRE(lddx >= Cin && lddy >= Cout, DGTTA_ERR_BADARG, "conv3d_k3_dgrad: ld < C");
  hipStream_t st = (hipStream_t)stream;
  if (impl != 1 && stride == 1 && !accumulate) {
    // stride-1 data gradient == forward conv of dy with the mirrored, transposed weights (wb)
    // (imgB: N = ci, K = co; taps mirrored)
    int rc = conv3_fwd_mfma(dy, lddy, imgB_of(wpack, CinP, CoutP, dtype), 1, nullptr, dx, lddx, B, Cout, Cin, CoutP, CinP, Di,
                            Hi, Wi, 1, dtype, st, nullptr, gst, 0, false);
    if (rc != DGTTA_ERR_UNSUPPORTED) return rc;
    DG_REQUIRE(impl == 0, DGTTA_ERR_UNSUPPORTED, "conv3d_k3_dgrad: shape not covered by the MFMA kernel");
  }
  if (impl != 1 && stride == 2 && !((Di | Hi | Wi) & 1)) {
    int rc = conv3_dgrad_s2_mfma(dy, lddy, imgB_of(wpack, CinP, CoutP, dtype), dx, lddx, B, Cin, Cout, CinP, CoutP, Di, Hi, Wi,
                                 accumulate, dtype, st);
    if (rc != DGTTA_ERR_UNSUPPORTED) return rc;
    DG_REQUIRE(impl == 0, DGTTA_ERR_UNSUPPORTED, "conv3d_k3_dgrad: shape not covered by the MFMA kernel");
  }
  return conv3_dgrad_ref(dy, lddy, wb, dx, lddx, B, Cin, Cout, CinP, CoutP, Di, Hi, Wi, stride, accumulate, dtype, st);
}

extern "C" int dgtta_conv3d_k3_dgrad(const void *dy, int lddy, const void *wpack, void *dx, int lddx, int B, int Cin,
                                     int Cout, int CinP, int CoutP, int Di, int Hi, int Wi, int stride, int accumulate,
                                     int dtype, int impl, void *stream) {
  return k3_dgrad(dy, lddy, wpack, dx, lddx, B, Cin, Cout, CinP, CoutP, Di, Hi, Wi, stride, accumulate, dtype, impl, stream, nullptr);
}

extern "C" int dgtta_conv3d_k3_dgrad_gstats(const void *dy, int lddy, const void *wpack, void *dx, int lddx, int B, int Cin,
                                            int Cout, int CinP, int CoutP, int Di, int Hi, int Wi, const void *y_prev,
                                            int ldy_prev, const float *mean_rstd_prev, const float *gamma_prev,
                                            const float *beta_prev, float slope, void *gstats, size_t gstats_bytes,
                                            int *h_produced, int dtype, int impl, void *stream) {
  DG_REQUIRE(y_prev && mean_rstd_prev && gamma_prev && beta_prev && gstats && h_produced, DGTTA_ERR_BADARG,
             "conv3d_k3_dgrad_gstats: null pointer");
  DG_REQUIRE(ldy_prev >= Cin, DGTTA_ERR_BADARG, "conv3d_k3_dgrad_gstats: ldy_prev < Cin");
  DG_REQUIRE(B > 0 && Cin > 0 && Di > 0 && Hi > 0 && Wi > 0 && gstats_bytes >= dgtta_conv3d_stats_bytes(B, Cin, Di, Hi, Wi),
             DGTTA_ERR_WORKSPACE, "conv3d_k3_dgrad_gstats: statistics buffer too small");
  RowsGstCtx ctx{y_prev, ldy_prev, mean_rstd_prev, gamma_prev, beta_prev, slope, (double *)gstats, 0};
  // only the row-reuse kernel (16-bit storage, large whole-tile volumes) knows the fused form; any other dispatch ignores
  // the context and *h_produced stays 0: the caller then runs the plain dgtta_instnorm_lrelu_bwd
  const bool fuse = dtype != DGTTA_F32 && impl != 1 && dgtta_switches().in_gstats != '0';
  const int rc = k3_dgrad(dy, lddy, wpack, dx, lddx, B, Cin, Cout, CinP, CoutP, Di, Hi, Wi, 1, 0, dtype, impl, stream,
                          fuse ? &ctx : nullptr);
  *h_produced = rc == DGTTA_OK ? ctx.produced : 0;
  return rc;
}

// workspace layout: [bias partials][main: split partials of the VALU kernel | slabs of the MFMA kernel]
static size_t wgrad_bias_bytes(int B, int Cout, int Do, int Ho, int Wo) {
  return align_up((size_t)B * reduce_blocks((int64_t)Do * Ho * Wo, B) * Cout * 2 * sizeof(double), 256);
}

extern "C" size_t dgtta_conv3d_wgrad_ws_bytes(int B, int Cin, int Cout, int Do, int Ho, int Wo) {
  if (B <= 0 || Cin <= 0 || Cout <= 0 || Do <= 0 || Ho <= 0 || Wo <= 0) return 0;      // a size query of an empty problem (the launchers reject it with DGTTA_ERR_BADARG)
  const int64_t nvox = (int64_t)B * Do * Ho * Wo;
  size_t a = align_up((size_t)wgrad_splits(nvox) * Cout * Cin * 27 * sizeof(float), 256);
  size_t c = align_up(conv3_wgrad_mfma_ws_bytes(B, Cin, Cout, Do, Ho, Wo), 256);   // stride 1: input dims == output dims
  return wgrad_bias_bytes(B, Cout, Do, Ho, Wo) + (a > c ? a : c);
}

// workspace that lets an fp32 stride-1 weight gradient run as six 16-bit launches on bf16 split planes (conv_wgrad.hip): the
// plain workspace followed by three planes of x and three of dy
extern "C" size_t dgtta_conv3d_wgrad_split_ws_bytes(int B, int Cin, int Cout, int Do, int Ho, int Wo, int stride) {
  if (B <= 0 || Cin <= 0 || Cout <= 0 || Do <= 0 || Ho <= 0 || Wo <= 0 || (stride != 1 && stride != 2)) return 0;
  const size_t base = dgtta_conv3d_wgrad_ws_bytes(B, Cin, Cout, Do, Ho, Wo);
  // the split planes start behind the 256-aligned slab region of the MAIN part (workspace = [bias partials][main])
  return base + 256 + conv3_wgrad_split_extra_bytes(B, Cin, Cout, Do, Ho, Wo, stride);
}

static int k3_wgrad(const void *x, int ldx, long long x_block_stride, const void *dy, int lddy, float *dw_t, float *db, void *ws,
                    size_t ws_bytes, int B, int Cin, int Cout, int Di, int Hi, int Wi, int stride, int accumulate, int dtype, int impl,
                    void *stream) {
  DG_REQUIRE(x && dy && dw_t && ws, DGTTA_ERR_BADARG, "conv3d_k3_wgrad: null pointer");
  DG_REQUIRE(B > 0 && Cin > 0 && Cout > 0 && Di > 0 && Hi > 0 && Wi > 0, DGTTA_ERR_BADARG, "conv3d_k3_wgrad: bad dims");
  DG_REQUIRE(stride == 1 || stride == 2, DGTTA_ERR_UNSUPPORTED, "conv3d_k3_wgrad: stride %d", stride);
  const int Do = out_dim(Di, stride), Ho = out_dim(Hi, stride), Wo = out_dim(Wi, stride);
  DG_REQUIRE(ws_bytes >= dgtta_conv3d_wgrad_ws_bytes(B, Cin, Cout, Do, Ho, Wo), DGTTA_ERR_WORKSPACE,
             "conv3d_k3_wgrad: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  const int64_t nvox = (int64_t)B * Do * Ho * Wo;
  const int nsplit = wgrad_splits(nvox);
  const size_t bias_bytes = wgrad_bias_bytes(B, Cout, Do, Ho, Wo);
  void *ws2 = ws;                                   // bias partials
  float *part = (float *)((char *)ws + bias_bytes); // main region
  bool done = false;
  if (impl != 1) {
    int rc = conv3_wgrad_mfma(x, ldx, dy, lddy, dw_t, part, ws_bytes - bias_bytes, B, Cin, Cout, Di, Hi, Wi,
                              stride, accumulate, dtype, st, x_block_stride);
    if (rc == DGTTA_OK) done = true;
    else if (rc != DGTTA_ERR_UNSUPPORTED) return rc;
    else DG_REQUIRE(impl == 0 && x_block_stride == 0, DGTTA_ERR_UNSUPPORTED,
                    "conv3d_k3_wgrad: shape not covered by the MFMA kernel (x as 32-channel planes: only the ring sweep, ask dgtta_conv3d_k3_blocked_supported)");
  }
  if (!done) {
    const int rc = conv3_wgrad_ref(x, ldx, dy, lddy, part, nsplit, dw_t, B, Cin, Cout, Di, Hi, Wi, stride, accumulate, dtype, st);
    if (rc != DGTTA_OK) return rc;
  }
  if (db) return conv_bias_grad(dy, lddy, db, ws2, B, Cout, (int64_t)Do * Ho * Wo, accumulate, dtype, st);
  return DGTTA_OK;
}

extern "C" int dgtta_conv3d_k3_wgrad(const void *x, int ldx, const void *dy, int lddy, float *dw_t, float *db, void *ws,
                                     size_t ws_bytes, int B, int Cin, int Cout, int Di, int Hi, int Wi, int stride,
                                     int accumulate, int dtype, int impl, void *stream) {
  return k3_wgrad(x, ldx, 0, dy, lddy, dw_t, db, ws, ws_bytes, B, Cin, Cout, Di, Hi, Wi, stride, accumulate, dtype, impl, stream);
}

// weight gradient of a stride-1 conv whose x lies as 32-channel blocks (see dgtta_conv3d_k3_fwd_blocked); same workspace
extern "C" int dgtta_conv3d_k3_wgrad_blocked(const void *x, long long x_block_stride, const void *dy, int lddy, float *dw_t, float *db,
                                             void *ws, size_t ws_bytes, int B, int Cin, int Cout, int Di, int Hi, int Wi,
                                             int accumulate, int dtype, void *stream) {
  DG_REQUIRE(x_block_stride > 0 && x_block_stride % 8 == 0, DGTTA_ERR_BADARG, "conv3d_k3_wgrad_blocked: block stride must be a positive multiple of 8 elements");
  return k3_wgrad(x, 32, x_block_stride, dy, lddy, dw_t, db, ws, ws_bytes, B, Cin, Cout, Di, Hi, Wi, 1, accumulate, dtype, 0, stream);
}

extern "C" size_t dgtta_convT3d_fwd_ws_bytes(int Cin, int Cout, int dtype) {
  if (Cin <= 0 || Cout <= 0) return 0;
  return convT_pack_region(Cin, Cout, dtype);
}

extern "C" int dgtta_convT3d_k2s2_fwd(const void *x, int ldx, const float *w_t, const float *bias, void *out, int ldo,
                                      void *ws, size_t ws_bytes, int B, int Cin, int Cout, int Di, int Hi, int Wi,
                                      int dtype, int impl, void *stream) {
  DG_REQUIRE(x && w_t && out, DGTTA_ERR_BADARG, "convT3d_k2s2_fwd: null pointer");
  DG_REQUIRE(B > 0 && Cin > 0 && Cout > 0 && Di > 0 && Hi > 0 && Wi > 0 && ldx >= Cin && ldo >= Cout, DGTTA_ERR_BADARG,
             "convT3d_k2s2_fwd: bad dims");
  hipStream_t st = (hipStream_t)stream;
  if (impl != 1 && ws && ws_bytes >= convT_pack_region(Cin, Cout, dtype)) {
    int rc = convT_fwd_mfma(x, ldx, w_t, bias, out, ldo, ws, B, Cin, Cout, Di, Hi, Wi, dtype, st);
    if (rc != DGTTA_ERR_UNSUPPORTED) return rc;
  }
  DG_REQUIRE(impl != 2, DGTTA_ERR_UNSUPPORTED, "convT3d_k2s2_fwd: shape not covered by the MFMA kernel");
  return convT_fwd_ref(x, ldx, w_t, bias, out, ldo, B, Cin, Cout, Di, Hi, Wi, dtype, st);
}

// workspace layout: [bias partials][packed weights][main: split partials (VALU) | slabs (MFMA)]
static size_t convT_bias_region(int B, int Cout, int Di, int Hi, int Wi) {
  return align_up((size_t)B * reduce_blocks((int64_t)Di * Hi * Wi * 8, B) * Cout * 2 * sizeof(double), 256);
}

extern "C" size_t dgtta_convT3d_bwd_ws_bytes(int B, int Cin, int Cout, int Di, int Hi, int Wi) {
  if (B <= 0 || Cin <= 0 || Cout <= 0 || Di <= 0 || Hi <= 0 || Wi <= 0) return 0;      // a size query of an empty problem (the launchers reject it with DGTTA_ERR_BADARG)
  const int64_t nvox = (int64_t)B * Di * Hi * Wi;
  size_t a = align_up((size_t)wgrad_splits(nvox) * Cin * Cout * 8 * sizeof(float), 256);
  size_t c = align_up(conv3_wgrad_mfma_ws_bytes(B, Cin, Cout, Di, Hi, Wi), 256);
  return convT_bias_region(B, Cout, Di, Hi, Wi) + convT_pack_region(Cin, Cout, DGTTA_F32) + (a > c ? a : c);
}

// ... with room for the fp32 weight gradient as six 16-bit launches on three-term bf16 splits (conv_wgrad.hip)
extern "C" size_t dgtta_convT3d_bwd_split_ws_bytes(int B, int Cin, int Cout, int Di, int Hi, int Wi) {
  if (B <= 0 || Cin <= 0 || Cout <= 0 || Di <= 0 || Hi <= 0 || Wi <= 0) return 0;
  const int64_t nvox = (int64_t)B * Di * Hi * Wi;
  size_t a = align_up((size_t)wgrad_splits(nvox) * Cin * Cout * 8 * sizeof(float), 256);
  size_t c = align_up(conv3_wgrad_mfma_ws_bytes(B, Cin, Cout, Di, Hi, Wi), 256) + convT_wgrad_split_extra_bytes(B, Cin, Cout, Di, Hi, Wi);
  return convT_bias_region(B, Cout, Di, Hi, Wi) + convT_pack_region(Cin, Cout, DGTTA_F32) + (a > c ? a : c);
}

extern "C" int dgtta_convT3d_k2s2_bwd(const void *x, int ldx, const void *dout, int lddo, const float *w_t, void *dx,
                                      int lddx, float *dw_t, float *db, void *ws, size_t ws_bytes, int B, int Cin,
                                      int Cout, int Di, int Hi, int Wi, int accumulate, int dtype, int impl,
                                      void *stream) {
  DG_REQUIRE(x && dout && w_t && ws, DGTTA_ERR_BADARG, "convT3d_k2s2_bwd: null pointer");
  DG_REQUIRE(B > 0 && Cin > 0 && Cout > 0 && Di > 0 && Hi > 0 && Wi > 0 && ldx >= Cin && lddo >= Cout,
             DGTTA_ERR_BADARG, "convT3d_k2s2_bwd: bad dims");
  DG_REQUIRE(ws_bytes >= dgtta_convT3d_bwd_ws_bytes(B, Cin, Cout, Di, Hi, Wi), DGTTA_ERR_WORKSPACE,
             "convT3d_k2s2_bwd: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  const int64_t nvox = (int64_t)B * Di * Hi * Wi;
  void *ws_bias = ws;
  void *ws_pack = (char *)ws + convT_bias_region(B, Cout, Di, Hi, Wi);
  void *ws_main = (char *)ws_pack + convT_pack_region(Cin, Cout, DGTTA_F32);
  const size_t main_bytes = ws_bytes - ((char *)ws_main - (char *)ws);
  int bias_units = 0;
  if (dx) {
    DG_REQUIRE(lddx >= Cin, DGTTA_ERR_BADARG, "convT3d_k2s2_bwd: lddx < Cin");
    int rc = DGTTA_ERR_UNSUPPORTED;
    if (impl != 1) rc = convT_dgrad_mfma(dout, lddo, w_t, dx, lddx, ws_pack, B, Cin, Cout, Di, Hi, Wi, dtype, st);
    if (rc == DGTTA_ERR_UNSUPPORTED) {
      DG_REQUIRE(impl != 2, DGTTA_ERR_UNSUPPORTED, "convT3d_k2s2_bwd: dgrad shape not covered by the MFMA kernel");
      rc = convT_dgrad_ref(dout, lddo, w_t, dx, lddx, B, Cin, Cout, Di, Hi, Wi, dtype, st);
      if (rc != DGTTA_OK) return rc;
    } else if (rc != DGTTA_OK) {
      return rc;
    }
  }
  if (dw_t) {
    int rc = DGTTA_ERR_UNSUPPORTED;
    if (impl != 1)      // (the one-pass kernel also leaves the bias gradient's partial sums in the bias region when asked)
      rc = convT_wgrad_mfma(x, ldx, dout, lddo, dw_t, ws_main, main_bytes, B, Cin, Cout, Di, Hi, Wi, accumulate, dtype, st,
                            db ? (float *)ws_bias : nullptr, convT_bias_region(B, Cout, Di, Hi, Wi), &bias_units);
    if (rc == DGTTA_ERR_UNSUPPORTED) {
      DG_REQUIRE(impl != 2, DGTTA_ERR_UNSUPPORTED, "convT3d_k2s2_bwd: wgrad shape not covered by the MFMA kernel");
      rc = convT_wgrad_ref(x, ldx, dout, lddo, (float *)ws_main, wgrad_splits(nvox), dw_t, B, Cin, Cout, Di, Hi, Wi, accumulate,
                           dtype, st);
      if (rc != DGTTA_OK) return rc;
    } else if (rc != DGTTA_OK) {
      return rc;
    }
  }
  if (db && bias_units > 0) {
    DG_REQUIRE(convT_bias_finalize((const float *)ws_bias, bias_units, Cout, db, accumulate, st) == DGTTA_OK, DGTTA_ERR_LAUNCH,
               "convT3d_k2s2_bwd: bias finalize launch failed");
    return DGTTA_OK;
  }
  if (db) return conv_bias_grad(dout, lddo, db, ws_bias, B, Cout, (int64_t)Di * Hi * Wi * 8, accumulate, dtype, st);
  return DGTTA_OK;
}
