// Weight gradients of the 3x3x3 convolutions on the matrix cores: the host side.  Launch plans, workspace sizes, the choice of
// the kernel (conv_wgrad_ring.hip, conv_wgrad_flat.hip, conv_wgrad_rows.hip, conv_wgrad_s2.hip) and of the slab reduction
// (conv_wgrad_reduce.hip) for one WgradLaunch, and the fp32 weight gradient as six 16-bit launches.  The pointer-level entry
// points fill a WgradLaunch / WgradOut pair and a class table (wgrad_single_class, wgrad_parity_classes); convt_wgrad.hip
// (transposed convs) and head_wgrad.hip (1x1x1 head) come in through wgrad_launch_classes with theirs.
#include "conv_wgrad_common.h"

WgradPlan wgrad_plan(int B, int Cin, int Cout, int D, int H, int W, int ncls, int tileW, int tileH) {
  WgradPlan p;
  p.tW = cdiv(W, tileW);
  p.tH = cdiv(H, tileH);
  p.cibs = cdiv(Cin, 32);
  p.cobs = cdiv(Cout, 32);
  const int64_t base = (int64_t)B * p.tW * p.tH * p.cibs * p.cobs * ncls;
  int want = (int)cdiv64(512, base > 0 ? base : 1);   // aim for >= ~512 workgroups (2 per CU) over all classes
  int maxsplit = D / 4 > 0 ? D / 4 : 1;
  p.nsd = want < 1 ? 1 : (want > maxsplit ? maxsplit : want);
  p.DR = cdiv(D, p.nsd);
  p.nsd = cdiv(D, p.DR);
  p.units = (int64_t)B * p.tW * p.tH * p.nsd;
  return p;
}

// sized for the 8-class launches (stride-2 conv, transposed conv) and the one-pass stride-2 plan; single-class launches
// use the first part
size_t conv3_wgrad_mfma_ws_bytes(int B, int Cin, int Cout, int D, int H, int W) {
  WgradPlan p1 = wgrad_plan(B, Cin, Cout, D, H, W, 1, 32, WT::TH), p8 = wgrad_plan(B, Cin, Cout, D, H, W, 8, 32, WT::TH),
            p2 = wgrad_plan(B, Cin, Cout, D, H, W, 1, WT2::TWO, WT2::TH);
  const size_t a = wgrad_slab_bytes(p1, 1), b = wgrad_slab_bytes(p8, 8), c = wgrad_slab_bytes(p2, 1);
  return a > b ? (a > c ? a : c) : (b > c ? b : c);
}

// units a workgroup sweeps into one slab: as many as keep >= `slots` workgroups in the launch (at most 4; DGTTA_WGRAD_UPW=1:
// one unit per workgroup, the round-2a partition; =2..4: forced, for the tests)
static int units_per_workgroup(int64_t units, int64_t gy, int slots) {
  const int sw = dgtta_switches().wgrad_upw;
  if (sw == '1') return 1;
  if (sw >= '2' && sw <= '4') return (int)(units < sw - '0' ? units : sw - '0');      // forced (tests)
  int64_t u = units * gy / slots;
  if (u > 4) u = 4;
  if (u > units) u = units;
  return u < 1 ? 1 : (int)u;
}

int wgrad_launch_classes(const WgradLaunch &L, const WgradOut &out, const WgradClasses &wc, const RealTaps &reals) {
  if (!dtype_ok(L.dtype)) return DGTTA_ERR_UNSUPPORTED;      // (esize() below takes every other dtype for 16-bit)
  const int esz = (int)esize(L.dtype), EPV = 16 / esz;
  const View &xv = L.xv, &yv = L.yv;
  // Cin may be ragged (first layer: 12 channels in rows of 16): the pad channels only feed gradient rows ci >= Cin,
  // which the reduction never writes.  The rows must be long enough to be read in whole 16-byte groups.
  if (L.Cout % EPV || xv.sw % EPV || yv.sw % EPV || ((uintptr_t)L.x & 15) || ((uintptr_t)L.dy & 15) ||
      xv.sw < (L.xkh ? 32 : (L.Cin + EPV - 1) / EPV * EPV))      // (x as 32-channel planes: rows of one block)
    return DGTTA_ERR_UNSUPPORTED;
  for (int c = 0; c < wc.n; ++c)
    if ((wc.xoff[c] * (long long)esz) % 16 || (wc.yoff[c] * (long long)esz) % 16) return DGTTA_ERR_UNSUPPORTED;
  const DgttaSwitches &sw = dgtta_switches();
  if (L.xkh && (esz != 2 || sw.wgrad_tr == '0' || sw.wgrad_ring == '0')) return DGTTA_ERR_UNSUPPORTED;
  WgradPlan p = wgrad_plan(L.B, L.Cin, L.Cout, yv.D, yv.H, yv.W, wc.n, 32, WT::TH);
  if (L.ws_bytes < wgrad_slab_bytes(p, wc.n) || p.units >= (1ll << 31) || p.cibs * p.cobs > 65535) return DGTTA_ERR_UNSUPPORTED;
  int64_t nslab = p.units;            // partial slabs per (channel-block pair, class)
  int rc = DGTTA_OK;
  if (esz == 2 && sw.wgrad_tr != '0') {        // DGTTA_WGRAD_TR=0 (tests): the register-transpose predecessor
    const bool plain = wc.n == 1 && wc.mask[0] == 0x7ffffffu && wc.xoff[0] == 0 && wc.yoff[0] == 0;
    // planes of W <= 16 as flat runs (DGTTA_WGRAD_FLAT=0: the kernels below).  Not for the six launches of an fp32 weight
    // gradient (split_leg): that path's fixtures compare label maps and Adam update signs of near-tied values bit for bit
    // with the reference run, i.e. they are pinned on the summation order of the kernels below
    int64_t g = 0;
    if (plain && !L.xkh && !L.split_leg && sw.wgrad_flat != '0') {
      g = wgrad_flat_launch(L, &rc);
      if (rc != DGTTA_OK) return rc;
    }
    if (g == 0 && plain && sw.wgrad_ring != '0') {      // the persistent ring sweep (conv_wgrad_ring.hip; DGTTA_WGRAD_RING=0: its predecessors)
      g = conv3_wgrad_ring_launch(L, &rc);
      if (rc != DGTTA_OK) return rc;
    }
    if (g > 0) {
      nslab = g;
    } else if (L.xkh) {
      return DGTTA_ERR_UNSUPPORTED;      // only the ring sweep reads x as 32-channel planes
    } else if (plain && L.Cout >= 64 && sw.wgrad_tr8 != '0') {      // DGTTA_WGRAD_TR8=0 (tests): always the 4-wave kernel
      const int upw = units_per_workgroup(p.units, (int64_t)p.cibs * ((p.cobs + 1) / 2), 256);      // one 8-wave workgroup per CU
      nslab = cdiv64(p.units, upw);
      rc = conv3_wgrad_tr8_launch(L, p, upw, nslab);
    } else {
      // two 4-wave workgroups per CU; class launches keep one unit per workgroup (their classes carry 1..8 taps: many
      // small workgroups balance that, 4 units each measured 1.5x slower)
      const int upw = plain ? units_per_workgroup(p.units, (int64_t)p.cibs * p.cobs, 512) : 1;
      nslab = cdiv64(p.units, upw);
      rc = conv3_wgrad_tr_launch(L, p, wc, plain, upw, nslab);
    }
  } else {
    rc = conv3_wgrad_mfma_launch(L, p, wc);
  }
  if (rc != DGTTA_OK) return rc;
  return wgrad_reduce_launch(L, out, p, wc.n, nslab, reals);
}

// 3x3x3 conv P, stride 1 or 2 (even extents).  L.xv: x at full resolution, L.yv: dy
static int wgrad_conv(const ConvProblem &P, const WgradLaunch &L, const WgradOut &out) {
  RealTaps reals;
  if (P.sd == 1) return wgrad_launch_classes(L, out, wgrad_single_class(0x7ffffffu, identity_taps(0), &reals), reals);
  if (L.xkh) return DGTTA_ERR_UNSUPPORTED;
  if (L.dtype != DGTTA_F32) {
    // one pass over x (full resolution tile) and dy with all 27 taps: conv3_wgrad_tr_s2_kernel
    const int one = dgtta_switches().wgrad_s2_onepass;      // DGTTA_WGRAD_S2_ONEPASS=0 (tests): the 8-class launch
    WgradPlan p = wgrad_plan(L.B, L.Cin, L.Cout, L.yv.D, L.yv.H, L.yv.W, 1, WT2::TWO, WT2::TH);
    if (wgrad_onepass_ok(L, p) && one != '0') {
      // two output-channel blocks share the x tile (DGTTA_WGRAD_S2_ONEPASS=1: one)
      const int rc = conv3_wgrad_s2_launch(L, p, p.cobs % 2 == 0 && L.Cout % 64 == 0 && one != '1');
      if (rc != DGTTA_OK) return rc;
      reals.t[0] = identity_taps(0);
      return wgrad_reduce_launch(L, out, p, 1, p.units, reals);
    }
  }
  // x[2*vo + tap - 1] lives on the parity sub-lattices of x: 8 classes of a stride-1 problem
  WgradLaunch C = L;
  const WgradClasses wc = wgrad_parity_classes(P, (int)L.xv.sw, &reals, &C.xv);
  return wgrad_launch_classes(C, out, wc, reals);
}

// ---------------------------------------------------------------------------------------------------------------------
// fp32 weight gradient on the 16-bit matrix-core kernels (round 5).  The reference computes in fp32
// (dg_tta/tta/tta.py:560 never autocasts) and fp32 is what `dgtta run_tta` defaults to; the fp32 MFMA weight-gradient kernel
// (v_mfma_f32_32x32x2_f32, 157 TFLOP/s peak) took 40 % of an fp32 epoch at 0.48 of that peak.  An fp32 number is EXACTLY the
// sum of three bf16 numbers (3 x 8 significand bits, same exponent range):  x = x0 + x1 + x2,  dy = g0 + g1 + g2, and a
// bf16 x bf16 product is exact in the fp32 accumulator of v_mfma_f32_*_bf16.  So
//     dW = sum_v x dy = sum over (i, j) of [sum_v x_i g_j]:  the six products with i + j <= 2 carry everything above 2^-24 of the
// largest term (what fp32 rounding leaves anyway); each is ONE launch of the 16-bit weight-gradient kernels (ring sweep,
// tr, tr8) on the split planes, accumulated into dW in a fixed order (0,0) (0,1) (1,0) (0,2) (1,1) (2,0).  The split is one
// streaming pass per operand (4 B read, 6 B written per element).  Six launches at 0.40 of the 2.5 PF peak = 167 TFLOP/s
// fp32-equivalent before the split passes, against 75 for the kernel it replaces.
// Workspace: [slab region of the 16-bit plan][x planes 3 x B V ldxs][dy planes 3 x B V ldys] (dgtta_conv3d_wgrad_split_ws_bytes).
namespace {
__device__ __forceinline__ void split3(float v, bf16_t &a0, bf16_t &a1, bf16_t &a2) {
  a0 = f32_to_bf16(v);
  const float r1 = v - bf16_to_f32(a0);          // exact
  a1 = f32_to_bf16(r1);
  const float r2 = r1 - bf16_to_f32(a1);         // exact
  a2 = f32_to_bf16(r2);
}

// rows [n][ld] fp32 (C used channels) -> three planes [n][lds] bf16 (channels >= C zero); one thread = 8 channels of a row
__global__ __launch_bounds__(256) void split3_bf16_kernel(const float *__restrict__ x, int ld, int C, int lds, int64_t n,
                                                        bf16_t *__restrict__ p0, bf16_t *__restrict__ p1,
                                                        bf16_t *__restrict__ p2) {
  const int groups = lds >> 3;
  const int64_t total = n * groups;
  const bool vec = (ld & 3) == 0 && (C & 7) == 0 && (((uintptr_t)x) & 15) == 0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / groups;
    const int g = (int)(i - r * groups);
    float v[8];
    if (vec) {
      const float4 lo = *reinterpret_cast<const float4 *>(x + r * ld + 8 * g), hi = *reinterpret_cast<const float4 *>(x + r * ld + 8 * g + 4);
      v[0] = lo.x, v[1] = lo.y, v[2] = lo.z, v[3] = lo.w, v[4] = hi.x, v[5] = hi.y, v[6] = hi.z, v[7] = hi.w;
    } else {
#pragma unroll
      for (int k = 0; k < 8; ++k) v[k] = (8 * g + k) < C ? x[r * ld + 8 * g + k] : 0.f;
    }
    bf16_t a[3][8];
#pragma unroll
    for (int k = 0; k < 8; ++k) split3(v[k], a[0][k], a[1][k], a[2][k]);
    bf16_t *dst[3] = {p0, p1, p2};
#pragma unroll
    for (int q = 0; q < 3; ++q) {
      uint4 w;
      w.x = (unsigned)a[q][0] | ((unsigned)a[q][1] << 16);
      w.y = (unsigned)a[q][2] | ((unsigned)a[q][3] << 16);
      w.z = (unsigned)a[q][4] | ((unsigned)a[q][5] << 16);
      w.w = (unsigned)a[q][6] | ((unsigned)a[q][7] << 16);
      *reinterpret_cast<uint4 *>(dst[q] + r * lds + 8 * g) = w;
    }
  }
}
}  // namespace

size_t wgrad_split_plane_bytes(int B, int C, int D, int H, int W) {
  return align_up((size_t)B * D * H * W * ((C + 7) / 8 * 8) * sizeof(bf16_t), 256);
}
// extra bytes behind the slab region: 3 planes of x (input extent = stride x output extent) and 3 of dy (output extent D, H, W)
size_t conv3_wgrad_split_extra_bytes(int B, int Cin, int Cout, int D, int H, int W, int stride) {
  return 3 * wgrad_split_plane_bytes(B, Cin, D * stride, H * stride, W * stride) + 3 * wgrad_split_plane_bytes(B, Cout, D, H, W);
}

// carves the three x planes and the three dy planes out of the workspace behind the slab region, fills them (one streaming pass
// per operand) and runs the six products in their fixed order
int wgrad_f32_split(const SplitOperand &x, const SplitOperand &dy, void *ws, size_t ws_bytes, size_t slab_bytes, int accumulate,
                    hipStream_t st, const WgradSplitLeg &leg) {
  const size_t px = wgrad_split_plane_bytes(x.B, x.C, x.D, x.H, x.W), py = wgrad_split_plane_bytes(dy.B, dy.C, dy.D, dy.H, dy.W);
  if (dy.C % 8 || dgtta_switches().wgrad_f32_split == '0' || ws_bytes < slab_bytes + 3 * px + 3 * py) return DGTTA_ERR_UNSUPPORTED;
  const int ldxs = (x.C + 7) / 8 * 8, ldys = (dy.C + 7) / 8 * 8;
  const int64_t rows_x = (int64_t)x.B * x.D * x.H * x.W, rows_y = (int64_t)dy.B * dy.D * dy.H * dy.W;
  char *planes = (char *)ws + slab_bytes;
  bf16_t *xs[3], *gs[3];
  for (int i = 0; i < 3; ++i) {
    xs[i] = (bf16_t *)(planes + i * px);
    gs[i] = (bf16_t *)(planes + 3 * px + i * py);
  }
  const int64_t tx = rows_x * (ldxs / 8), ty = rows_y * (ldys / 8);
  hipLaunchKernelGGL(split3_bf16_kernel, dim3((unsigned)(cdiv64(tx, 256) < 8192 ? cdiv64(tx, 256) : 8192)), dim3(256), 0, st, x.p, x.ld,
                     x.C, ldxs, rows_x, xs[0], xs[1], xs[2]);
  hipLaunchKernelGGL(split3_bf16_kernel, dim3((unsigned)(cdiv64(ty, 256) < 8192 ? cdiv64(ty, 256) : 8192)), dim3(256), 0, st, dy.p,
                     dy.ld, dy.C, ldys, rows_y, gs[0], gs[1], gs[2]);
  DG_CHECK_LAUNCH("split3_bf16_kernel");
  constexpr int PAIRS[6][2] = {{0, 0}, {0, 1}, {1, 0}, {0, 2}, {1, 1}, {2, 0}};      // (x plane, dy plane), in this order
  for (int q = 0; q < 6; ++q) {
    const int rc = leg(xs[PAIRS[q][0]], ldxs, gs[PAIRS[q][1]], ldys, (accumulate || q > 0) ? 1 : 0);
    if (rc != DGTTA_OK) return rc;        // (q == 0: nothing written yet, the caller falls back to the fp32 kernel)
  }
  return DGTTA_OK;
}

int conv3_wgrad_mfma(const ConvProblem &P, Src x, Src dy, float *dw_t, Region ws, int accumulate) {
  const int B = P.B, Di = P.Di, Hi = P.Hi, Wi = P.Wi;
  if (!stride_ok(P.sd)) return DGTTA_ERR_UNSUPPORTED;
  if (P.sd == 2 && ((Di | Hi | Wi) & 1)) return DGTTA_ERR_UNSUPPORTED;   // odd extents: leave to the general kernel
  const int Do = P.Do(), Ho = P.Ho(), Wo = P.Wo();
  WgradLaunch L{x.p, dense_view(B, Di, Hi, Wi, x.ld), dy.p, dense_view(B, Do, Ho, Wo, dy.ld), B, P.Cin, P.Cout, P.dtype, ws.p, ws.bytes, P.st};
  L.xkh = x.kh;
  const WgradOut out{dw_t, (long long)P.Cin * 27, 27, 1, accumulate};
  if (P.dtype == DGTTA_F32) {
    if (x.kh) return DGTTA_ERR_UNSUPPORTED;      // (x as 32-channel planes: 16-bit storage only)
    // the caller offered the split workspace (dgtta_conv3d_wgrad_split_ws_bytes) behind the plain one: six 16-bit launches
    // (DGTTA_WGRAD_F32_SPLIT=0: the fp32 MFMA kernel, its predecessor)
    const size_t slab = align_up(conv3_wgrad_mfma_ws_bytes(B, P.Cin, P.Cout, Do, Ho, Wo), 256);
    const SplitOperand sx{(const float *)x.p, x.ld, P.Cin, B, Di, Hi, Wi}, sy{(const float *)dy.p, dy.ld, P.Cout, B, Do, Ho, Wo};
    const int rc = wgrad_f32_split(sx, sy, ws.p, ws.bytes, slab, accumulate, P.st,
                                   [&](const bf16_t *xs, int ldxs, const bf16_t *gs, int ldys, int acc) {
      WgradLaunch leg = L;
      leg.x = xs, leg.xv = dense_view(B, Di, Hi, Wi, ldxs), leg.dy = gs, leg.yv = dense_view(B, Do, Ho, Wo, ldys);
      leg.dtype = DGTTA_BF16, leg.ws_bytes = slab, leg.split_leg = true;
      return wgrad_conv(P, leg, WgradOut{dw_t, out.s_co, out.s_ci, out.s_tap, acc});
    });
    if (rc != DGTTA_ERR_UNSUPPORTED) return rc;
  } else if (!dtype_ok(P.dtype)) {
    return DGTTA_ERR_UNSUPPORTED;
  }
  return wgrad_conv(P, L, out);
}
// would the weight gradient of the stride-1 conv P take x as 32-channel planes (only the ring sweep does)?
bool conv3_wgrad_blocked_ok(const ConvProblem &P) {
  if ((P.dtype != DGTTA_BF16 && P.dtype != DGTTA_F16) || P.Cin % 32 || P.Cout % 8) return false;
  if (dgtta_switches().wgrad_tr == '0' || dgtta_switches().wgrad_ring == '0') return false;
  const View xv = dense_view(P.B, P.Di, P.Hi, P.Wi, 32), yv = dense_view(P.B, P.Di, P.Hi, P.Wi, P.Cout);
  int rc = DGTTA_OK;
  const size_t ws_bytes = conv3_wgrad_mfma_ws_bytes(P.B, P.Cin, P.Cout, P.Di, P.Hi, P.Wi);
  WgradLaunch L{(const void *)16, xv, (const void *)16, yv, P.B, P.Cin, P.Cout, P.dtype, nullptr, ws_bytes, nullptr};
  L.xkh = P.B * P.in_vox() * 32, L.dry = true;
  const int g = conv3_wgrad_ring_launch(L, &rc);
  return rc == DGTTA_OK && g > 0;
}

// ---------------------------------------------------------------------------------------------------------------------
// Weight gradients of the anisotropic layers (conv_aniso.hip) on the class-masked kernels (conv_wgrad_rows.hip): the classes of
// wgrad_parity_classes - the kernels multiply only the virtual taps with a real tap, and the fixed-order slab reduction writes
// them into torch layout [Cout][Cin][kd * 9].
size_t wgrad_classes_bytes(int B, int Cin, int Cout, int D, int H, int W, int ncls) {
  const WgradPlan p = wgrad_plan(B, Cin, Cout, D, H, W, ncls, 32, WT::TH);
  return wgrad_slab_bytes(p, ncls);
}

// slabs for any class count 1..8 on a dy lattice of D x H x W (the plan's D split depends on the class count)
size_t conva_wgrad_ws_bytes(int B, int Cin, int Cout, int D, int H, int W) {
  size_t best = conv3_wgrad_mfma_ws_bytes(B, Cin, Cout, D, H, W);
  for (int n = 1; n <= 8; ++n) {
    const size_t b = wgrad_classes_bytes(B, Cin, Cout, D, H, W, n);
    best = b > best ? b : best;
  }
  return best;
}

int conva_wgrad_mfma(const ConvProblem &P, Src x, Src dy, float *dw_t, Region ws, int accumulate) {
  const int Do = P.Do(), Ho = P.Ho(), Wo = P.Wo();
  WgradLaunch L{x.p, View{}, dy.p, dense_view(P.B, Do, Ho, Wo, dy.ld), P.B, P.Cin, P.Cout, P.dtype, ws.p, ws.bytes, P.st};
  RealTaps reals;
  const WgradClasses wc = wgrad_parity_classes(P, x.ld, &reals, &L.xv);
  if (ws.bytes < wgrad_classes_bytes(P.B, P.Cin, P.Cout, Do, Ho, Wo, wc.n)) return DGTTA_ERR_WORKSPACE;
  return wgrad_launch_classes(L, WgradOut{dw_t, (long long)P.Cin * P.ntaps(), P.ntaps(), 1, accumulate}, wc, reals);
}
