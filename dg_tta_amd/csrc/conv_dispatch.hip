// C ABI of the 3x3x3 convolutions and the 2x2x2 transposed convolutions (dgtta_conv3d_*, dgtta_convT3d_*): argument
// checks, weight-blob and workspace layout, and the choice of kernel - the MFMA implementations (conv_mfma.hip,
// conv_wgrad.hip, which pick between the ring / row-reuse / generic tile kernels themselves) first, the general-shape
// VALU kernels of conv_ref.hip for what they return DGTTA_ERR_UNSUPPORTED for (impl 0), or one of the two alone
// (impl 2 / impl 1: the tests' cross-check).  Host code only: every kernel lives in the unit its launcher is declared for.
// Every entry point fills one ConvProblem (kd = 3, sd = sh = sw = stride; the transposed convs kd = sd = sh = sw = 2); the checks
// and the workspace layouts are those of conv_api.h, shared with the general family of conv_aniso.hip.
#include "conv_api.h"

// blob = [wf | wb] (general kernels) followed by [imgF | imgB] (LDS-image order for the MFMA kernels)
static const void *wb_of(const void *wpack, const ConvProblem &P) { return (const char *)wpack + (size_t)27 * P.CinP * P.CoutP * esize(P.dtype); }
static const void *img_of(const void *wpack, const ConvProblem &P) { return (const char *)wpack + (size_t)2 * 27 * P.CinP * P.CoutP * esize(P.dtype); }
static const void *imgB_of(const void *wpack, const ConvProblem &P) {
  return (const char *)img_of(wpack, P) + conv_imgB_offset_bytes(P.CinP, P.CoutP, P.dtype);
}

extern "C" size_t dgtta_conv3d_packed_bytes(int CinP, int CoutP, int dtype) {
  if (CinP <= 0 || CoutP <= 0) return 0;      // a size query of an empty problem (the launchers reject it with DGTTA_ERR_BADARG)
  return (size_t)2 * 27 * CinP * CoutP * esize(dtype) + conv_image_bytes(CinP, CoutP, dtype);
}

extern "C" int dgtta_conv3d_pack_weights(const float *w_t, void *wpack, int Cin, int Cout, int CinP, int CoutP,
                                         int dtype, void *stream) {
  const ConvProblem P{0, Cin, Cout, CinP, CoutP, 0, 0, 0, 3, 1, 1, 1, dtype, (hipStream_t)stream};
  DG_REQUIRE(w_t && wpack, DGTTA_ERR_BADARG, "pack_weights: null pointer");
  DG_REQUIRE(Cin > 0 && Cout > 0 && CinP >= Cin && CoutP >= Cout, DGTTA_ERR_BADARG, "pack_weights: bad channel counts");
  const int rc = conv3_pack_weights_ref(P, w_t, wpack, const_cast<void *>(wb_of(wpack, P)));
  if (rc != DGTTA_OK) return rc;
  if (CinP % conv_granule(dtype) == 0 && CoutP % conv_granule(dtype) == 0)
    return conv_pack_images(P, w_t, const_cast<void *>(img_of(wpack, P)));
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

// x.kh != 0: dgtta_conv3d_k3_fwd_blocked
static int k3_fwd(const ConvProblem &P, Src x, const void *wpack, const float *bias, Dst y, void *stats, int impl) {
  static const char fn[] = "conv3d_k3_fwd";
  CONV_REQUIRE_PTRS(fn, x.p && wpack && y.p);
  CONV_REQUIRE_DIMS(fn, P, false, true);
  CONV_REQUIRE_K3_STRIDE(fn, P);
  CONV_REQUIRE_LD(fn, (x.kh ? 2 * x.ld : x.ld) >= P.Cin && y.ld >= P.Cout);
  if (impl != 1) {
    const int rc = conv3_fwd_mfma(P, x, img_of(wpack, P), 0, bias, y, (double *)stats, nullptr);
    if (rc != DGTTA_ERR_UNSUPPORTED) return rc;
    DG_REQUIRE(x.kh == 0, DGTTA_ERR_UNSUPPORTED,
               "conv3d_k3_fwd_blocked: only the D-ring kernel reads x as 32-channel planes (ask dgtta_conv3d_k3_blocked_supported)");
    DG_REQUIRE(impl == 0, DGTTA_ERR_UNSUPPORTED, "conv3d_k3_fwd: shape not covered by the MFMA kernel");
  }
  const int rc = conv3_fwd_ref(P, x, wpack, bias, y);      // (wf: the head of the blob)
  if (rc != DGTTA_OK) return rc;
  // general kernel: statistics by a separate reduction pass, same buffer layout
  if (stats) return conv_stats_ref(y.p, y.ld, stats, P.B, P.Cout, P.out_vox(), P.dtype, P.st);
  return DGTTA_OK;
}

extern "C" int dgtta_conv3d_k3_fwd(const void *x, int ldx, const void *wpack, const float *bias, void *y, int ldy,
                                   void *stats, int B, int Cin, int Cout, int CinP, int CoutP, int Di, int Hi, int Wi,
                                   int stride, int dtype, int impl, void *stream) {
  const ConvProblem P{B, Cin, Cout, CinP, CoutP, Di, Hi, Wi, 3, stride, stride, stride, dtype, (hipStream_t)stream};
  return k3_fwd(P, Src{x, ldx}, wpack, bias, Dst{y, ldy}, stats, impl);
}

// Round 6: x as 32-channel BLOCKS - block c of the input channels is a dense tensor [B][D][H][W][32] (ldx = 32) at element
// offset c * x_block_stride from x.  The level-0 concat buffer of the U-Net is kept that way ([up | skip] as two planes): the
// kernels that read ONE half of it (the stride-2 conv of the skip, the transposed conv's backward) then use whole 128-byte lines.
// Only the D-ring kernels read this layout (64 input channels, 16-bit storage, launches they take): ask
// dgtta_conv3d_k3_blocked_supported first; anything else returns DGTTA_ERR_UNSUPPORTED and launches nothing.
extern "C" int dgtta_conv3d_k3_blocked_supported(int B, int Cin, int Cout, int D, int H, int W, int dtype) {
  if (B <= 0 || Cin != 64 || Cout <= 0 || Cout % 32 || D <= 0 || H <= 0 || W <= 0) return 0;
  if (dtype != DGTTA_BF16 && dtype != DGTTA_F16) return 0;
  const ConvProblem P{B, Cin, Cout, Cin, Cout, D, H, W, 3, 1, 1, 1, dtype, nullptr, /*dry*/ true};
  const int rc = conv3_fwd_mfma(P, Src{(const void *)16, 32, P.B * P.in_vox() * 32}, (const void *)16, 0, nullptr, Dst{(void *)16, Cout},
                                nullptr, nullptr);
  return rc == DGTTA_OK && conv3_wgrad_blocked_ok(P);
}

extern "C" int dgtta_conv3d_k3_fwd_blocked(const void *x, long long x_block_stride, const void *wpack, const float *bias, void *y,
                                           int ldy, void *stats, int B, int Cin, int Cout, int CinP, int CoutP, int Di, int Hi,
                                           int Wi, int dtype, void *stream) {
  DG_REQUIRE(x_block_stride > 0 && x_block_stride % 8 == 0, DGTTA_ERR_BADARG, "conv3d_k3_fwd_blocked: block stride must be a positive multiple of 8 elements");
  const ConvProblem P{B, Cin, Cout, CinP, CoutP, Di, Hi, Wi, 3, 1, 1, 1, dtype, (hipStream_t)stream};
  return k3_fwd(P, Src{x, 32, x_block_stride}, wpack, bias, Dst{y, ldy}, stats, 0);
}

// gst: the InstanceNorm-backward context of dgtta_conv3d_k3_dgrad_gstats (null for the plain data gradient); it travels down
// the dispatch chain as an argument and only the ring / row-reuse launchers act on it
static int k3_dgrad(const ConvProblem &P, Src dy, const void *wpack, Dst dx, int accumulate, int impl, RowsGstCtx *gst) {
  static const char fn[] = "conv3d_k3_dgrad";
  CONV_REQUIRE_PTRS(fn, dy.p && wpack && dx.p);
  CONV_REQUIRE_DIMS(fn, P, false, true);
  CONV_REQUIRE_K3_STRIDE(fn, P);
  CONV_REQUIRE_LD(fn, dx.ld >= P.Cin && dy.ld >= P.Cout);
  // stride 1: the forward conv of dy with the mirrored, transposed weights (imgB: N = ci, K = co; taps mirrored); stride 2 with
  // even extents: the parity classes
  const bool as_fwd = P.sd == 1 && !accumulate, classes = P.sd == 2 && P.even_strided();
  if (impl != 1 && (as_fwd || classes)) {
    const int rc = as_fwd ? conv3_fwd_mfma(dgrad_as_fwd(P), dy, imgB_of(wpack, P), 1, nullptr, dx, nullptr, gst)
                          : conv3_dgrad_s2_mfma(P, dy, imgB_of(wpack, P), dx, accumulate);
    if (rc != DGTTA_ERR_UNSUPPORTED) return rc;
    DG_REQUIRE(impl == 0, DGTTA_ERR_UNSUPPORTED, "conv3d_k3_dgrad: shape not covered by the MFMA kernel");
  }
  return conv3_dgrad_ref(P, dy, wb_of(wpack, P), dx, accumulate);
}

extern "C" int dgtta_conv3d_k3_dgrad(const void *dy, int lddy, const void *wpack, void *dx, int lddx, int B, int Cin,
                                     int Cout, int CinP, int CoutP, int Di, int Hi, int Wi, int stride, int accumulate,
                                     int dtype, int impl, void *stream) {
  const ConvProblem P{B, Cin, Cout, CinP, CoutP, Di, Hi, Wi, 3, stride, stride, stride, dtype, (hipStream_t)stream};
  return k3_dgrad(P, Src{dy, lddy}, wpack, Dst{dx, lddx}, accumulate, impl, nullptr);
}

extern "C" int dgtta_conv3d_k3_dgrad_gstats(const void *dy, int lddy, const void *wpack, void *dx, int lddx, int B, int Cin,
                                            int Cout, int CinP, int CoutP, int Di, int Hi, int Wi, const void *y_prev,
                                            int ldy_prev, const float *mean_rstd_prev, const float *gamma_prev,
                                            const float *beta_prev, float slope, void *gstats, size_t gstats_bytes,
                                            int *h_produced, int dtype, int impl, void *stream) {
  CONV_REQUIRE_PTRS("conv3d_k3_dgrad_gstats", y_prev && mean_rstd_prev && gamma_prev && beta_prev && gstats && h_produced);
  DG_REQUIRE(ldy_prev >= Cin, DGTTA_ERR_BADARG, "conv3d_k3_dgrad_gstats: ldy_prev < Cin");
  DG_REQUIRE(B > 0 && Cin > 0 && Di > 0 && Hi > 0 && Wi > 0 && gstats_bytes >= dgtta_conv3d_stats_bytes(B, Cin, Di, Hi, Wi),
             DGTTA_ERR_WORKSPACE, "conv3d_k3_dgrad_gstats: statistics buffer too small");
  RowsGstCtx ctx{y_prev, ldy_prev, mean_rstd_prev, gamma_prev, beta_prev, slope, (double *)gstats, 0};
  // only the row-reuse kernel (16-bit storage, large whole-tile volumes) knows the fused form; any other dispatch ignores
  // the context and *h_produced stays 0: the caller then runs the plain dgtta_instnorm_lrelu_bwd
  const bool fuse = dtype != DGTTA_F32 && impl != 1 && dgtta_switches().in_gstats != '0';
  const ConvProblem P{B, Cin, Cout, CinP, CoutP, Di, Hi, Wi, 3, 1, 1, 1, dtype, (hipStream_t)stream};
  const int rc = k3_dgrad(P, Src{dy, lddy}, wpack, Dst{dx, lddx}, 0, impl, fuse ? &ctx : nullptr);
  *h_produced = rc == DGTTA_OK ? ctx.produced : 0;
  return rc;
}

// The size queries of the weight gradient are given the OUTPUT extent: they ask the layout with it as a stride-1 problem.
// split_stride != 0: with the room that lets an fp32 weight gradient of that stride run as six 16-bit launches (conv_wgrad.hip)
static size_t k3_wgrad_ws_bytes(int B, int Cin, int Cout, int Do, int Ho, int Wo, int split_stride) {
  if (B <= 0 || Cin <= 0 || Cout <= 0 || Do <= 0 || Ho <= 0 || Wo <= 0) return 0;      // a size query of an empty problem (the launchers reject it with DGTTA_ERR_BADARG)
  const ConvProblem P{B, Cin, Cout, Cin, Cout, Do, Ho, Wo, 3, 1, 1, 1, DGTTA_F32, nullptr};
  return conv_wgrad_ws_layout(P, false, split_stride).total();
}
extern "C" size_t dgtta_conv3d_wgrad_ws_bytes(int B, int Cin, int Cout, int Do, int Ho, int Wo) {
  return k3_wgrad_ws_bytes(B, Cin, Cout, Do, Ho, Wo, 0);
}
extern "C" size_t dgtta_conv3d_wgrad_split_ws_bytes(int B, int Cin, int Cout, int Do, int Ho, int Wo, int stride) {
  return stride_ok(stride) ? k3_wgrad_ws_bytes(B, Cin, Cout, Do, Ho, Wo, stride) : 0;
}

// x.kh != 0: dgtta_conv3d_k3_wgrad_blocked
static int k3_wgrad(const ConvProblem &P, Src x, Src dy, float *dw_t, float *db, Region ws, int accumulate, int impl) {
  static const char fn[] = "conv3d_k3_wgrad";
  CONV_REQUIRE_PTRS(fn, x.p && dy.p && dw_t && ws.p);
  CONV_REQUIRE_DIMS(fn, P, false, true);
  CONV_REQUIRE_K3_STRIDE(fn, P);
  const ConvWsLayout lay = conv_wgrad_ws_layout(P, false);
  CONV_REQUIRE_WS(fn, ws.bytes, lay.total());
  const Region main = lay.main_of(ws.p, ws.bytes);
  int rc = impl != 1 ? conv3_wgrad_mfma(P, x, dy, dw_t, main, accumulate) : DGTTA_ERR_UNSUPPORTED;
  if (rc == DGTTA_ERR_UNSUPPORTED) {
    DG_REQUIRE(impl == 1 || (impl == 0 && x.kh == 0), DGTTA_ERR_UNSUPPORTED,
               "conv3d_k3_wgrad: shape not covered by the MFMA kernel (x as 32-channel planes: only the ring sweep, ask dgtta_conv3d_k3_blocked_supported)");
    rc = conv3_wgrad_ref(P, x, dy, (float *)main.p, wgrad_splits(P.B * P.out_vox()), dw_t, accumulate);
  }
  if (rc != DGTTA_OK) return rc;
  if (db) return conv_bias_grad(dy.p, dy.ld, db, ws.p, P.B, P.Cout, P.out_vox(), accumulate, P.dtype, P.st);
  return DGTTA_OK;
}

extern "C" int dgtta_conv3d_k3_wgrad(const void *x, int ldx, const void *dy, int lddy, float *dw_t, float *db, void *ws,
                                     size_t ws_bytes, int B, int Cin, int Cout, int Di, int Hi, int Wi, int stride,
                                     int accumulate, int dtype, int impl, void *stream) {
  const ConvProblem P{B, Cin, Cout, Cin, Cout, Di, Hi, Wi, 3, stride, stride, stride, dtype, (hipStream_t)stream};
  return k3_wgrad(P, Src{x, ldx}, Src{dy, lddy}, dw_t, db, Region{ws, ws_bytes}, accumulate, impl);
}

// weight gradient of a stride-1 conv whose x lies as 32-channel blocks (see dgtta_conv3d_k3_fwd_blocked); same workspace
extern "C" int dgtta_conv3d_k3_wgrad_blocked(const void *x, long long x_block_stride, const void *dy, int lddy, float *dw_t, float *db,
                                             void *ws, size_t ws_bytes, int B, int Cin, int Cout, int Di, int Hi, int Wi,
                                             int accumulate, int dtype, void *stream) {
  DG_REQUIRE(x_block_stride > 0 && x_block_stride % 8 == 0, DGTTA_ERR_BADARG, "conv3d_k3_wgrad_blocked: block stride must be a positive multiple of 8 elements");
  const ConvProblem P{B, Cin, Cout, Cin, Cout, Di, Hi, Wi, 3, 1, 1, 1, dtype, (hipStream_t)stream};
  return k3_wgrad(P, Src{x, 32, x_block_stride}, Src{dy, lddy}, dw_t, db, Region{ws, ws_bytes}, accumulate, 0);
}

extern "C" size_t dgtta_convT3d_fwd_ws_bytes(int Cin, int Cout, int dtype) {
  if (Cin <= 0 || Cout <= 0) return 0;
  return convT_pack_region(Cin, Cout, dtype);
}

extern "C" int dgtta_convT3d_k2s2_fwd(const void *x, int ldx, const float *w_t, const float *bias, void *out, int ldo,
                                      void *ws, size_t ws_bytes, int B, int Cin, int Cout, int Di, int Hi, int Wi,
                                      int dtype, int impl, void *stream) {
  static const char fn[] = "convT3d_k2s2_fwd";
  const ConvProblem P{B, Cin, Cout, Cin, Cout, Di, Hi, Wi, 2, 2, 2, 2, dtype, (hipStream_t)stream};
  const Src xs{x, ldx};
  const Dst os{out, ldo};
  CONV_REQUIRE_PTRS(fn, x && w_t && out);
  CONV_REQUIRE_DIMS(fn, P, false, ldx >= Cin && ldo >= Cout);
  if (impl != 1 && ws && ws_bytes >= convT_pack_region(Cin, Cout, dtype)) {
    const int rc = convT_fwd_mfma(P, xs, w_t, bias, os, ws);
    if (rc != DGTTA_ERR_UNSUPPORTED) return rc;
  }
  DG_REQUIRE(impl != 2, DGTTA_ERR_UNSUPPORTED, "convT3d_k2s2_fwd: shape not covered by the MFMA kernel");
  return convT_fwd_ref(P, xs, w_t, bias, os);
}

// split: with room for the fp32 weight gradient as six 16-bit launches on three-term bf16 splits (conv_wgrad.hip)
static size_t convT_bwd_ws_bytes(int B, int Cin, int Cout, int Di, int Hi, int Wi, bool split) {
  if (B <= 0 || Cin <= 0 || Cout <= 0 || Di <= 0 || Hi <= 0 || Wi <= 0) return 0;      // a size query of an empty problem (the launchers reject it with DGTTA_ERR_BADARG)
  const ConvProblem P{B, Cin, Cout, Cin, Cout, Di, Hi, Wi, 2, 2, 2, 2, DGTTA_F32, nullptr};
  return convT_bwd_ws_layout(P, false, split).total();
}
extern "C" size_t dgtta_convT3d_bwd_ws_bytes(int B, int Cin, int Cout, int Di, int Hi, int Wi) {
  return convT_bwd_ws_bytes(B, Cin, Cout, Di, Hi, Wi, false);
}
extern "C" size_t dgtta_convT3d_bwd_split_ws_bytes(int B, int Cin, int Cout, int Di, int Hi, int Wi) {
  return convT_bwd_ws_bytes(B, Cin, Cout, Di, Hi, Wi, true);
}

extern "C" int dgtta_convT3d_k2s2_bwd(const void *x, int ldx, const void *dout, int lddo, const float *w_t, void *dx,
                                      int lddx, float *dw_t, float *db, void *ws, size_t ws_bytes, int B, int Cin,
                                      int Cout, int Di, int Hi, int Wi, int accumulate, int dtype, int impl,
                                      void *stream) {
  static const char fn[] = "convT3d_k2s2_bwd";
  const ConvProblem P{B, Cin, Cout, Cin, Cout, Di, Hi, Wi, 2, 2, 2, 2, dtype, (hipStream_t)stream};
  const Src xs{x, ldx}, dos{dout, lddo};
  CONV_REQUIRE_PTRS(fn, x && dout && w_t && ws);
  CONV_REQUIRE_DIMS(fn, P, false, ldx >= Cin && lddo >= Cout);
  const ConvWsLayout lay = convT_bwd_ws_layout(P, false);
  CONV_REQUIRE_WS(fn, ws_bytes, lay.total());
  const Region ws_bias{ws, lay.bias}, ws_main = lay.main_of(ws, ws_bytes);
  int bias_units = 0;
  if (dx) {
    DG_REQUIRE(lddx >= Cin, DGTTA_ERR_BADARG, "convT3d_k2s2_bwd: lddx < Cin");
    int rc = impl != 1 ? convT_dgrad_mfma(P, dos, w_t, Dst{dx, lddx}, lay.pack_of(ws)) : DGTTA_ERR_UNSUPPORTED;
    if (rc == DGTTA_ERR_UNSUPPORTED) {
      DG_REQUIRE(impl != 2, DGTTA_ERR_UNSUPPORTED, "convT3d_k2s2_bwd: dgrad shape not covered by the MFMA kernel");
      rc = convT_dgrad_ref(P, dos, w_t, Dst{dx, lddx});
    }
    if (rc != DGTTA_OK) return rc;
  }
  if (dw_t) {
    // (the one-pass kernel also leaves the bias gradient's partial sums in the bias region when asked)
    int rc = impl != 1 ? convT_wgrad_mfma(P, xs, dos, dw_t, ws_main, accumulate, db ? ws_bias : Region{}, &bias_units) : DGTTA_ERR_UNSUPPORTED;
    if (rc == DGTTA_ERR_UNSUPPORTED) {
      DG_REQUIRE(impl != 2, DGTTA_ERR_UNSUPPORTED, "convT3d_k2s2_bwd: wgrad shape not covered by the MFMA kernel");
      rc = convT_wgrad_ref(P, xs, dos, (float *)ws_main.p, wgrad_splits(P.B * P.in_vox()), dw_t, accumulate);
    }
    if (rc != DGTTA_OK) return rc;
  }
  if (db && bias_units > 0) {
    DG_REQUIRE(convT_bias_finalize((const float *)ws_bias.p, bias_units, Cout, db, accumulate, P.st) == DGTTA_OK, DGTTA_ERR_LAUNCH,
               "convT3d_k2s2_bwd: bias finalize launch failed");
    return DGTTA_OK;
  }
  if (db) return conv_bias_grad(dout, lddo, db, ws_bias.p, B, Cout, P.t_vox(), accumulate, dtype, P.st);
  return DGTTA_OK;
}
