// Weight gradient of the transposed convolutions (kernel = stride) on the matrix cores.
#include "conv_wgrad_common.h"

namespace {

// ---------------------------------------------------------------------------------------------------------------------
// bf16 weight gradient of ConvTranspose3d(k2,s2) in one pass:  dW[ci][co][o] = sum_v x[v][ci] * dout[2v + o][co].
// Tile = 2 rows x 16 voxels of the INPUT lattice; the dout tile is kept at full resolution (4 rows x 32 voxels, slices 2d and
// 2d+1) and read with a 2-voxel row stride, the x fragment of a row is shared by the 8 offsets (2 per wave).  x and dout are
// read once, instead of 8 single-tap class launches that each re-read x and gathered a dout parity sub-lattice.
template <int NCI>
struct WT3 {
  static constexpr int TH = 2, TWI = 16;
  static constexpr int X_ROW_B = TWI * 64, X_BLK_B = TH * X_ROW_B;               // one 32-channel block of an x slice: 2 KiB
  static constexpr int X_SLICE_B = NCI * X_BLK_B;
  static constexpr int Y_ROW_B = 2 * TWI * 64, Y_SLICE_B = 2 * TH * Y_ROW_B;     // one dout slice: 4 rows x 2 KiB
  static constexpr int Y_PAIR_B = 2 * Y_SLICE_B;                                 // dout slices 2d, 2d+1
  static constexpr int LDS_BYTES = 2 * X_SLICE_B + 2 * Y_PAIR_B;
  static constexpr int NPY = 2 * 2 * TH * 2;                                     // dout pieces per x slice (16 KiB)
};

// NCI (round 4): input-channel blocks of 32 per workgroup.  With one block per workgroup a 64-channel layer read dout - four
// times the bytes of x, the whole traffic of this HBM-bound kernel - once per block: 2.4 GB instead of 1.3 GB at the
// 64^3 -> 128^3 stage (836 us at 2.9 TB/s).  NCI = 2 shares the dout tile between two blocks of x.
template <typename T16 = bf16_t, int NCI = 1>
__global__ __launch_bounds__(256, 2) void convT_wgrad_tr_kernel(const bf16_t *__restrict__ x, View xv,
                                                                const bf16_t *__restrict__ dout, View yv,
                                                                float *__restrict__ slabs, int Cin, int Cout, int tilesW,
                                                                int tilesH, int nsd, int DR, int cobs, int cibs,
                                                                float *__restrict__ bias_part) {
  typedef WT3<NCI> WT;
  const int D = xv.D, H = xv.H, W = xv.W;                  // input lattice; yv = dense view of dout (2D x 2H x 2W)
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char *sX = smem;                                // 2 slots
  unsigned char *sY = smem + 2 * WT::X_SLICE_B;            // 2 slots of a slice pair
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  int t = xcd_unit(1);
  const int tw = t % tilesW;
  t /= tilesW;
  const int th = t % tilesH;
  t /= tilesH;
  const int ds = t % nsd;
  const int b = t / nsd;
  const int cig = blockIdx.y / cobs, cob = blockIdx.y % cobs;      // group of NCI input-channel blocks
  const int h0 = th * WT::TH, w0 = tw * WT::TWI;
  const int d_begin = ds * DR, d_end = (d_begin + DR < D) ? d_begin + DR : D;
  const bf16_t *xb = x + b * xv.sb + cig * NCI * 32;
  const bf16_t *yb = dout + b * yv.sb + cob * 32;
  const int cin_lim = (Cin + 7) / 8 * 8;
  const int l_vox = lane >> 2, l_chunk = lane & 3;

  // pieces of x slice d: NCI blocks x 2 rows (one per wave while they last); pieces of the dout pair: 2 slices x 4 rows x 2
  // halves = 16 (4 per wave)
  auto issue = [&](int d) __attribute__((always_inline)) {
    if (wave < WT::TH * NCI) {
      const int row = wave % WT::TH, blk = wave / WT::TH;
      const int gh = h0 + row, gw = w0 + l_vox;
      const bool ok = (unsigned)d < (unsigned)D && gh < H && gw < W && (cig * NCI + blk) * 32 + l_chunk * 8 < cin_lim;
      const void *src = ok ? (const void *)(xb + d * xv.sd + gh * xv.sh + gw * xv.sw + blk * 32 + l_chunk * 8)
                           : (const void *)&g_zero16;
      dma16_to_lds(src, lds_addr_of(sX + (d & 1) * WT::X_SLICE_B + blk * WT::X_BLK_B + row * WT::X_ROW_B));
    }
#pragma unroll
    for (int i = 0; i < WT::NPY / 4; ++i) {
      const int idx = wave + 4 * i;                     // (slice s, row r, half pi)
      const int sl = idx >> 3, r = (idx >> 1) & 3, pi = idx & 1;
      const int gd = 2 * d + sl, gh = 2 * h0 + r, gw = 2 * w0 + 16 * pi + l_vox;
      const bool ok = (unsigned)d < (unsigned)D && gd < yv.D && gh < yv.H && gw < yv.W && cob * 32 + l_chunk * 8 < Cout;
      const void *src = ok ? (const void *)(yb + gd * yv.sd + gh * yv.sh + gw * yv.sw + l_chunk * 8) : (const void *)&g_zero16;
      dma16_to_lds(src, lds_addr_of(sY + (d & 1) * WT::Y_PAIR_B + sl * WT::Y_SLICE_B + r * WT::Y_ROW_B + pi * 1024));
    }
  };

  const int kq = (lane >> 5) * 8 + ((lane & 15) >> 2), cpart = ((lane >> 4) & 1) * 32 + (lane & 3) * 8;
  const int lane_off_x = kq * 64 + cpart, lane_off_y = kq * 128 + cpart;
  // this wave's two output offsets o = 2 wave, 2 wave + 1  (o = od*4 + oh*2 + ow), for every input-channel block
  f32x16_t acc[NCI][2];
#pragma unroll
  for (int c = 0; c < NCI; ++c)
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int q = 0; q < 16; ++q) acc[c][i][q] = 0.f;
  int ooff[2];
#pragma unroll
  for (int i = 0; i < 2; ++i) {
    const int o = 2 * wave + i;
    ooff[i] = (o >> 2) * WT::Y_SLICE_B + ((o >> 1) & 1) * WT::Y_ROW_B + (o & 1) * 64;
  }
  // bias gradient sum_v dout[v][co] on the side (round 4; the first input-channel group's workgroups only): an x operand that is 1
  // in row 0 and 0 elsewhere leaves the column sums of the dout fragments in row 0 of a third accumulator pair - the pass
  // over dout that chan_reduce_vec_kernel<., 2> made for them (1.5 ms per epoch) is not needed
  const bool do_bias = bias_part != nullptr && cig == 0;
  const short one16 = sizeof(T16) == 2 && std::is_same<T16, f16_t>::value ? (short)0x3C00 : (short)0x3F80;
  const short o1 = (lane & 31) == 0 ? one16 : (short)0;
  const s16x8_t onesv = {o1, o1, o1, o1, o1, o1, o1, o1};
  const bf16x8_t ones = __builtin_bit_cast(bf16x8_t, onesv);
  f32x16_t bacc[2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int q = 0; q < 16; ++q) bacc[i][q] = 0.f;

  issue(d_begin);
  dma_wait_all();
  lds_barrier();
  for (int d = d_begin; d < d_end; ++d) {
    if (d + 1 < d_end) issue(d + 1);
    const unsigned char *xs = sX + (d & 1) * WT::X_SLICE_B + lane_off_x;
    const unsigned char *ys = sY + (d & 1) * WT::Y_PAIR_B + lane_off_y;
#pragma unroll
    for (int r = 0; r < WT::TH; ++r) {
      bf16x8_t bfr[2];
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const unsigned char *pb = ys + ooff[i] + 2 * r * WT::Y_ROW_B;
        const s16x4_t blo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_t *)pb);
        const s16x4_t bhi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_t *)(pb + 4 * 128));
        const s16x8_t bv = {blo[0], blo[1], blo[2], blo[3], bhi[0], bhi[1], bhi[2], bhi[3]};
        bfr[i] = __builtin_bit_cast(bf16x8_t, bv);
      }
      if (do_bias) {
#pragma unroll
        for (int i = 0; i < 2; ++i) bacc[i] = mfma32_tr<T16>(ones, bfr[i], bacc[i]);
      }
#pragma unroll
      for (int c = 0; c < NCI; ++c) {
        const unsigned char *pa = xs + c * WT::X_BLK_B + r * WT::X_ROW_B;
        const s16x4_t alo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_t *)pa);
        const s16x4_t ahi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_t *)(pa + 4 * 64));
        const s16x8_t av = {alo[0], alo[1], alo[2], alo[3], ahi[0], ahi[1], ahi[2], ahi[3]};
        const bf16x8_t afr = __builtin_bit_cast(bf16x8_t, av);
#pragma unroll
        for (int i = 0; i < 2; ++i) acc[c][i] = mfma32_tr<T16>(afr, bfr[i], acc[c][i]);
      }
    }
    dma_wait_all();
    lds_barrier();
  }
  // slab "tap" slot = output offset o; one slab per (input-channel block, output-channel block) pair and unit
  const int co = lane & 31, hh = lane >> 5;
#pragma unroll
  for (int c = 0; c < NCI; ++c) {
    const int cib = cig * NCI + c;
    if (cib < cibs) {
      float *slab = slabs + ((int64_t)(cib * cobs + cob) * gridDim.x + blockIdx.x) * (27 * 1024);
#pragma unroll
      for (int i = 0; i < 2; ++i) {
        const int o = 2 * wave + i;
#pragma unroll
        for (int q = 0; q < 16; ++q) slab[(o * 32 + (q & 3) + 8 * (q >> 2) + 4 * hh) * 32 + co] = acc[c][i][q];
      }
    }
  }
  if (do_bias) {      // row 0 of the accumulator = lanes 0..31, element 0; offsets, then waves, in order
    float *red = reinterpret_cast<float *>(smem);
    if (lane < 32) red[wave * 32 + lane] = bacc[0][0] + bacc[1][0];
    __syncthreads();
    if (tid < 32) bias_part[(int64_t)blockIdx.x * (cobs * 32) + cob * 32 + tid] = ((red[tid] + red[32 + tid]) + red[64 + tid]) + red[96 + tid];
  }
}

// sums the per-unit bias partials of convT_wgrad_tr_kernel: one workgroup per 32 output channels, 8 unit groups (unit mod 8)
// with eight loads in flight each, the groups added in order (double): a fixed summation order
__global__ __launch_bounds__(256) void convT_bias_finalize_kernel(const float *__restrict__ part, int units, int ldp, int Cout,
                                                                  float *__restrict__ db, int accumulate) {
  __shared__ double red[8][32];
  const int co = blockIdx.x * 32 + (threadIdx.x & 31), grp = threadIdx.x >> 5;
  double s = 0.0;
  for (int u = grp; u < units; u += 64) {
    float v[8];
#pragma unroll
    for (int j = 0; j < 8; ++j) v[j] = u + 8 * j < units ? part[(int64_t)(u + 8 * j) * ldp + co] : 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j)
      if (u + 8 * j < units) s += (double)v[j];
  }
  red[grp][threadIdx.x & 31] = s;
  __syncthreads();
  if (threadIdx.x < 32 && co < Cout) {
    double t = 0.0;
#pragma unroll
    for (int g = 0; g < 8; ++g) t += red[g][threadIdx.x];
    db[co] = accumulate ? db[co] + (float)t : (float)t;
  }
}

}  // namespace

// ConvTranspose3d with kernel = stride (sd, sh, sw): dw_t[ci][co][o] (+)= sum_v x[v][ci] * dout[s v + o][co], one single-tap class
// per output offset o = (od * sh + oh) * sw + ow (the dout lattice at that offset).  L.xv: the input lattice, L.yv: dout at full
// resolution
static int convT_wgrad_classes(const WgradLaunch &L, float *dw_t, int sd, int sh, int sw, int accumulate) {
  const int no = sd * sh * sw;
  WgradLaunch C = L;
  WgradClasses wc{};
  RealTaps reals;
  wc.n = no;
  for (int o = 0; o < no; ++o) {
    C.yv = lattice_view(L.yv, sd, sh, sw, o, &wc.yoff[o]);
    wc.mask[o] = 1u << 13;
    for (int t = 0; t < 27; ++t) reals.t[o].wt[t] = -1;
    reals.t[o].wt[13] = (signed char)o;
  }
  return wgrad_launch_classes(C, WgradOut{dw_t, no, (long long)L.Cout * no, 1, accumulate}, wc, reals);
}

// one-pass kernel with NCI input-channel blocks per workgroup; bp: room for the bias partials or nullptr
template <typename T16, int NCI>
static int convT_tr_launch(const WgradLaunch &L, const WgradPlan &p, float *bp) {
  static DynLdsOnce once;
  DG_REQUIRE(ensure_dyn_lds(once, reinterpret_cast<const void *>(convT_wgrad_tr_kernel<T16, NCI>), (int)WT3<NCI>::LDS_BYTES) ==
                 hipSuccess, DGTTA_ERR_LAUNCH, "convT_wgrad_tr: cannot raise the dynamic LDS limit");
  hipLaunchKernelGGL((convT_wgrad_tr_kernel<T16, NCI>), dim3((unsigned)p.units, (unsigned)(cdiv(p.cibs, NCI) * p.cobs)), dim3(256),
                     WT3<NCI>::LDS_BYTES, L.st, (const bf16_t *)L.x, L.xv, (const bf16_t *)L.dy, L.yv, (float *)L.ws, L.Cin, L.Cout, p.tW,
                     p.tH, p.nsd, p.DR, p.cobs, p.cibs, bp);
  DG_CHECK_LAUNCH("convT_wgrad_tr_kernel");
  return DGTTA_OK;
}

// ConvTranspose3d k2 s2 weight gradient: dw_t[ci][co][o] (+)= sum_v x[v][ci] * dout[2v+o][co]  (one pass, or 8 single-tap launches).
// L.xv: the input lattice, L.yv: dout at full resolution
static int convT_wgrad(const WgradLaunch &L, float *dw_t, int accumulate, Region bias_part, int *bias_units) {
  if (bias_units) *bias_units = 0;
  if (L.dtype != DGTTA_F32) {
    const int one = dgtta_switches().convt_wgrad_onepass;      // DGTTA_CONVT_WGRAD_ONEPASS=0 (tests): the 8-class launch
    WgradPlan p = wgrad_plan(L.B, L.Cin, L.Cout, L.xv.D, L.xv.H, L.xv.W, 1, WT2::TWO, WT2::TH);      // same tile shape (2 rows x 16 voxels) on the input lattice
    if (wgrad_onepass_ok(L, p) && one != '0') {
      // bias partials [unit][32 cobs] ride along when the caller offers room for them
      float *bp = (bias_part.p && bias_units && bias_part.bytes >= (size_t)p.units * p.cobs * 32 * sizeof(float)) ? (float *)bias_part.p : nullptr;
      if (bp) *bias_units = (int)p.units;
      const bool f16 = L.dtype == DGTTA_F16;
      int rc;
      if (p.cibs >= 2)      // two input-channel blocks share a dout tile
        rc = f16 ? convT_tr_launch<f16_t, 2>(L, p, bp) : convT_tr_launch<bf16_t, 2>(L, p, bp);
      else
        rc = f16 ? convT_tr_launch<f16_t, 1>(L, p, bp) : convT_tr_launch<bf16_t, 1>(L, p, bp);
      if (rc != DGTTA_OK) return rc;
      RealTaps rt;
      for (int t = 0; t < 27; ++t) rt.t[0].wt[t] = (signed char)(t < 8 ? t : -1);      // slab tap slot o -> dw_t[..][o]
      // (dw_t[ci][co][8] is not the dense 27-tap layout, so this ends in the row kernels)
      return wgrad_reduce_launch(L, WgradOut{dw_t, 8, (long long)L.Cout * 8, 1, accumulate}, p, 1, p.units, rt);
    }
  }
  return convT_wgrad_classes(L, dw_t, 2, 2, 2, accumulate);
}

// fp32 transposed-conv weight gradient as six launches of the 16-bit kernel on exact three-term bf16 splits (wgrad_f32_split,
// conv_wgrad.hip): extra bytes behind the slab region = 3 planes of x (input lattice) and 3 of dout (output lattice)
size_t convT_wgrad_split_extra_bytes(int B, int Cin, int Cout, int Di, int Hi, int Wi) {
  return 3 * wgrad_split_plane_bytes(B, Cin, Di, Hi, Wi) + 3 * wgrad_split_plane_bytes(B, Cout, 2 * Di, 2 * Hi, 2 * Wi);
}

// bias_part / bias_units (optional): room for [units][ceil(Cout / 32) * 32] floats; *bias_units > 0 on return means the launch left
// the per-unit sums of dout there (convT_bias_finalize adds them up), 0 means the caller runs its own pass over dout
int convT_wgrad_mfma(const ConvProblem &P, Src x, Src dout, float *dw_t, Region ws, int accumulate, Region bias_part, int *bias_units) {
  if (bias_units) *bias_units = 0;
  const int B = P.B, Di = P.Di, Hi = P.Hi, Wi = P.Wi;
  const View xv = dense_view(B, Di, Hi, Wi, x.ld), yfull = dense_view(B, P.Dt(), P.Ht(), P.Wt(), dout.ld);
  const WgradLaunch L{x.p, xv, dout.p, yfull, B, P.Cin, P.Cout, P.dtype, ws.p, ws.bytes, P.st};
  if (P.dtype == DGTTA_F32) {
    // the caller offered the split workspace (dgtta_convT3d_bwd_split_ws_bytes): six 16-bit launches (DGTTA_WGRAD_F32_SPLIT=0: never)
    const size_t slab = align_up(conv3_wgrad_mfma_ws_bytes(B, P.Cin, P.Cout, Di, Hi, Wi), 256);
    const SplitOperand sx{(const float *)x.p, x.ld, P.Cin, B, Di, Hi, Wi}, sy{(const float *)dout.p, dout.ld, P.Cout, B, P.Dt(), P.Ht(), P.Wt()};
    const int rc = wgrad_f32_split(sx, sy, ws.p, ws.bytes, slab, accumulate, P.st,
                                   [&](const bf16_t *xs, int ldxs, const bf16_t *gs, int ldys, int acc) {
      WgradLaunch leg = L;
      leg.x = xs, leg.xv = dense_view(B, Di, Hi, Wi, ldxs), leg.dy = gs, leg.yv = dense_view(B, P.Dt(), P.Ht(), P.Wt(), ldys);
      leg.dtype = DGTTA_BF16, leg.ws_bytes = slab;
      return convT_wgrad(leg, dw_t, acc, Region{}, nullptr);
    });
    if (rc != DGTTA_ERR_UNSUPPORTED) return rc;
    return convT_wgrad(L, dw_t, accumulate, Region{}, nullptr);
  }
  if (!dtype_ok(P.dtype)) return DGTTA_ERR_UNSUPPORTED;
  return convT_wgrad(L, dw_t, accumulate, bias_part, bias_units);
}

int convT_bias_finalize(const float *part, int units, int Cout, float *db, int accumulate, hipStream_t st) {
  hipLaunchKernelGGL(convT_bias_finalize_kernel, dim3((unsigned)cdiv(Cout, 32)), dim3(256), 0, st, part, units, cdiv(Cout, 32) * 32,
                     Cout, db, accumulate);
  return hipGetLastError() == hipSuccess ? DGTTA_OK : DGTTA_ERR_LAUNCH;
}

// (the anisotropic plans' transposed convs: convT_wgrad_classes with any kernel = stride)
int convTa_wgrad_mfma(const ConvProblem &P, Src x, Src dout, float *dw_t, Region ws, int accumulate) {
  if (ws.bytes < wgrad_classes_bytes(P.B, P.Cin, P.Cout, P.Di, P.Hi, P.Wi, P.noff())) return DGTTA_ERR_WORKSPACE;
  const View xv = dense_view(P.B, P.Di, P.Hi, P.Wi, x.ld), yfull = dense_view(P.B, P.Dt(), P.Ht(), P.Wt(), dout.ld);
  const WgradLaunch L{x.p, xv, dout.p, yfull, P.B, P.Cin, P.Cout, P.dtype, ws.p, ws.bytes, P.st};
  return convT_wgrad_classes(L, dw_t, P.sd, P.sh, P.sw, accumulate);
}
