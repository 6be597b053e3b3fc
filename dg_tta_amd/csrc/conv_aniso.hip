// Anisotropic convolutions of nnU-Net plans: [kd, 3, 3] kernels (kd = 1 or 3, padding kd / 2, 1, 1) with per-axis strides
// (sd, sh, sw) in {1, 2}^3, and transposed convolutions with kernel = stride in {1, 2}^3.
//
//   GEMM view:  M = output voxels (32 per MFMA block, consecutive along W), N = output channels, K = KD x 9 taps x Cin.
//   MFMA:       16-bit storage -> v_mfma_f32_32x32x16_{bf16,f16}; fp32 storage -> v_mfma_f32_32x32x2_f32 x4 (exact fp32 fma
//               chain); fp32 accumulation in all cases (mfma_step of conv_common.h).
//   Workgroup:  8 waves, output tile TD x TH x TW voxels (8 or 16 M-blocks of 32 voxels) x 32 output channels.
//   LDS:        A = input halo tile of one K-chunk (16 channels; 8 for fp32), [16-byte channel group][halo voxel]; its extent
//               is (T - 1) * S + K per axis, so a KD = 1, SD = 1 layer stages one plane per output plane instead of three.  Where
//               SW = 2 the halo rows are staged de-interleaved by W parity so that the 32 lanes of an M-block read
//               consecutive slots.  B = the chunk's weights [tap][group][cout] (KD x 9 taps only).
//   Data gradient: stride 1 = this kernel on dy with the transposed weight image and mirrored taps; a strided layer runs
//               one class per parity of its strided axes (2 to 8 classes, blockIdx.z), each a stride-1 conv over the taps
//               that reach that parity (a class without taps - kd = 1 with sd = 2, odd planes - writes zeros).
//   Weight gradient: the class-masked weight-gradient kernels of conv_wgrad_rows.hip (through conv_wgrad.hip) (only the present taps are multiplied)
//               with the fixed-order slab reduction into torch layout [Cout][Cin][kd][3][3] (conva_wgrad_mfma).
//   Transposed conv: the pointwise class GEMM of conv_mfma.hip with kd*kh*kw output classes (convTa_run).
#include "conv_common.h"
#include <stdlib.h>

namespace {

template <int MBW, int MBH, int MBD, int KD, int SD, int SH, int SW>
struct GeoA {
  static constexpr int HD = KD / 2;                   // zero padding along D (1 for kd = 3, 0 for kd = 1)
  static constexpr int NTAP = KD * 9;
  static constexpr int RPM = 32 / MBW;
  static constexpr int TW = MBW, TH = RPM * MBH, TD = MBD;
  static constexpr int MB = MBH * MBD;
  static constexpr int ID = (TD - 1) * SD + 1 + 2 * HD, IH = (TH - 1) * SH + 3, IW = (TW - 1) * SW + 3;
  static constexpr int IWH = (SW == 2) ? (IW + 1) / 2 : IW;
  static constexpr int ROW = (SW == 2) ? 2 * IWH : IW;
  static constexpr int NV = ID * IH * ROW;
  __host__ __device__ static constexpr int lds_col(int wx) { return (SW == 2) ? (wx & 1) * IWH + (wx >> 1) : wx; }
};

template <typename T, int MBW, int MBH, int MBD, int KD, int SD, int SH, int SW>
struct CfgA {
  typedef GeoA<MBW, MBH, MBD, KD, SD, SH, SW> G;
  static constexpr int EPV = Elem<T>::EPV;
  static constexpr int NG = 2;                 // 16-byte channel groups per K-chunk (one MFMA k-step)
  static constexpr int CK = NG * EPV;
  static constexpr int NC = 32;
  static constexpr int NW = 8;
  static constexpr size_t A_BYTES = (size_t)NG * G::NV * 16;
  static constexpr size_t B_BYTES = (size_t)G::NTAP * NG * NC * 16;
  static constexpr size_t LDS_BYTES = A_BYTES + B_BYTES;
};

// x: view xv; y: view yv (+ the class's offsets); virtual tap t = kd * 9 + kh * 3 + kw uses weight tap cs.taps[cls].wt[t]
// (-1: absent).  w: LDS-image order [N/32][K/(2*EPV)][ntaps_src][2][32][EPV] (conv_weight_image_index).
template <typename T, int MBW, int MBH, int MBD, int KD, int SD, int SH, int SW>
__global__ __launch_bounds__(512) void conva_mfma_kernel(const T *__restrict__ x, View xv, const T *__restrict__ w, ConvClasses cs,
                                                         const float *__restrict__ bias, T *__restrict__ y, View yv, int Cin,
                                                         int Cout, int CinP, int tilesW, int tilesH, int tilesD,
                                                         double *__restrict__ stats, int ntaps_src) {
  typedef CfgA<T, MBW, MBH, MBD, KD, SD, SH, SW> Cfg;
  typedef typename Cfg::G G;
  constexpr int EPV = Cfg::EPV, NG = Cfg::NG, CK = Cfg::CK, NC = Cfg::NC, NW = Cfg::NW, NV = G::NV, NTAP = G::NTAP;
  constexpr int MPW = G::MB / NW, NT = NW * 64;
  const int cls = blockIdx.z;
  x += cs.xoff[cls];
  y += cs.yoff[cls];
  const int accumulate = cs.acc[cls];
  const int Di = xv.D, Hi = xv.H, Wi = xv.W, Do = yv.D, Ho = yv.H, Wo = yv.W;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint4 *sA = reinterpret_cast<uint4 *>(smem);                    // [NG][NV]
  uint4 *sB = reinterpret_cast<uint4 *>(smem + Cfg::A_BYTES);     // [NTAP][NG][NC]

  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int r = lane & 31, h = lane >> 5;

  // a contiguous run of tiles per XCD (neighbouring tiles share their halo)
  int tlin = blockIdx.x;
  if ((gridDim.x & 7) == 0) tlin = (tlin & 7) * (int)(gridDim.x >> 3) + (tlin >> 3);
  int t = tlin;
  const int tw = t % tilesW;
  t /= tilesW;
  const int th = t % tilesH;
  t /= tilesH;
  const int td = t % tilesD;
  const int b = t / tilesD;
  const int n0 = blockIdx.y * NC;
  const int od0 = td * G::TD, oh0 = th * G::TH, ow0 = tw * G::TW;
  const int id0 = od0 * SD - G::HD, ih0 = oh0 * SH - 1, iw0 = ow0 * SW - 1;

  int a_off[MPW];
#pragma unroll
  for (int i = 0; i < MPW; ++i) {
    const int mb = wave * MPW + i;
    const int mbd = mb / MBH, mbh = mb % MBH;
    const int row = mbh * G::RPM + r / MBW, col = r % MBW;
    a_off[i] = ((mbd * SD) * G::IH + row * SH) * G::ROW + col;   // SW = 2: column index in the half row
  }
  f32x16_t acc[MPW];
#pragma unroll
  for (int i = 0; i < MPW; ++i)
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[i][q] = 0.f;

  const T *xbp = x + (int64_t)b * xv.sb;
  const int cin_lim = (Cin + EPV - 1) / EPV * EPV;

  __shared__ signed char s_wt[32];
  if (tid < 32) s_wt[tid] = tid < NTAP ? cs.taps[cls].wt[tid] : (signed char)-1;
  __syncthreads();

  constexpr int NA = (NV * NG + NT - 1) / NT, NBL = (NTAP * NC * NG + NT - 1) / NT;
  uint4 ra[NA], rb[NBL];
  int wslot[NBL];
#pragma unroll
  for (int i = 0; i < NBL; ++i) {
    const int idx = tid + i * NT;       // == LDS index (tap * NG + g) * NC + n
    const int n = idx % NC, g = (idx / NC) % NG, tap = idx / (NG * NC);
    const int wt = idx < NTAP * NC * NG ? s_wt[tap] : -1;
    const int off = ((((n0 + n) / 32) * (CinP / (2 * EPV)) + g / 2) * ntaps_src + wt) * 64 + (g & 1) * 32 + (n0 + n) % 32;
    wslot[i] = wt >= 0 ? off : -1;
  }
  auto load_chunk = [&](int kc) {
#pragma unroll
    for (int i = 0; i < NA; ++i) {
      const int idx = tid + i * NT;
      const int g = idx % NG, v = idx / NG;
      const int wx_l = v % G::ROW, hy = (v / G::ROW) % G::IH, dz = v / (G::ROW * G::IH);
      const int wx = (SW == 2) ? ((wx_l >= G::IWH) ? 2 * (wx_l - G::IWH) + 1 : 2 * wx_l) : wx_l;   // inverse of lds_col
      const int gd = id0 + dz, gh = ih0 + hy, gw = iw0 + wx;
      const int c = kc + g * EPV;
      const bool ok = idx < NV * NG && wx < G::IW && (unsigned)gd < (unsigned)Di && (unsigned)gh < (unsigned)Hi &&
                      (unsigned)gw < (unsigned)Wi && c < cin_lim;
      const T *p = ok ? xbp + gd * xv.sd + gh * xv.sh + gw * xv.sw + c : x;
      const uint4 val = *reinterpret_cast<const uint4 *>(p);
      ra[i] = ok ? val : make_uint4(0, 0, 0, 0);
    }
    const int kterm = (kc / (2 * EPV)) * ntaps_src * 64;
#pragma unroll
    for (int i = 0; i < NBL; ++i) {
      const bool ok = wslot[i] >= 0;
      const T *p = w + (int64_t)(ok ? wslot[i] + kterm : 0) * EPV;
      const uint4 val = *reinterpret_cast<const uint4 *>(p);
      rb[i] = ok ? val : make_uint4(0, 0, 0, 0);
    }
  };
  auto store_chunk = [&]() {
#pragma unroll
    for (int i = 0; i < NA; ++i) {
      const int idx = tid + i * NT;
      if (idx < NV * NG) sA[(idx % NG) * NV + idx / NG] = ra[i];
    }
#pragma unroll
    for (int i = 0; i < NBL; ++i) {
      const int idx = tid + i * NT;
      if (idx < NTAP * NC * NG) sB[idx] = rb[i];
    }
  };

  // register staging, software pipelined: the loads of chunk k + 1 are in flight while chunk k is multiplied
  load_chunk(0);
  for (int kc = 0; kc < CinP; kc += CK) {
    __syncthreads();
    store_chunk();
    __syncthreads();
    if (kc + CK < CinP) load_chunk(kc + CK);
#pragma unroll
    for (int tap = 0; tap < NTAP; ++tap) {
      if (s_wt[tap] < 0) continue;     // wave-uniform
      const int kd = tap / 9, kh = (tap / 3) % 3, kw = tap % 3;
      const int tap_off = (kd * G::IH + kh) * G::ROW + G::lds_col(kw);
      const uint4 bf = sB[(tap * NG + h) * NC + r];
#pragma unroll
      for (int i = 0; i < MPW; ++i) mfma_step<T>(sA[h * NV + a_off[i] + tap_off], bf, acc[i]);
    }
  }

  // ---- epilogue: bias, convert, store (acc row m = (q&3) + 8*(q>>2) + 4*h, column = r); optional InstanceNorm partial sums
  float st1 = 0.f, st2 = 0.f;
  const int co = n0 + r;
  const float bv = (bias && co < Cout) ? bias[co] : 0.f;
#pragma unroll
  for (int i = 0; i < MPW; ++i) {
    const int mb = wave * MPW + i;
    const int mbd = mb / MBH, mbh = mb % MBH;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int m = (q & 3) + 8 * (q >> 2) + 4 * h;
      const int od = od0 + mbd, oh = oh0 + mbh * G::RPM + m / MBW, ow = ow0 + m % MBW;
      if (co < Cout && od < Do && oh < Ho && ow < Wo) {
        T *o = y + b * yv.sb + od * yv.sd + oh * yv.sh + ow * yv.sw + co;
        float v = acc[i][q] + bv;
        if (accumulate) v += ld_f<T>(o);
        st_f<T>(o, v);
        st1 += v;
        st2 += v * v;
      }
    }
  }
  if (stats) {
    __syncthreads();                       // all waves are done with the A/B tiles: reuse LDS for the reduction
    float *red = reinterpret_cast<float *>(smem);      // [NW][NC][2]
    const float a = st1 + __shfl_xor(st1, 32, 64), c2 = st2 + __shfl_xor(st2, 32, 64);
    if (h == 0) {
      red[(wave * NC + r) * 2 + 0] = a;
      red[(wave * NC + r) * 2 + 1] = c2;
    }
    __syncthreads();
    const int tiles_per_b = tilesW * tilesH * tilesD;
    if (tid < NC && n0 + tid < Cout) {
      double s = 0.0, ss = 0.0;
#pragma unroll
      for (int wv = 0; wv < NW; ++wv) {
        s += (double)red[(wv * NC + tid) * 2 + 0];
        ss += (double)red[(wv * NC + tid) * 2 + 1];
      }
      double *p = stats + 32 + (((int64_t)b * tiles_per_b + (tlin % tiles_per_b)) * Cout + n0 + tid) * 2;
      p[0] = s;
      p[1] = ss;
    }
    if (blockIdx.x == 0 && blockIdx.y == 0 && blockIdx.z == 0 && tid == 0) reinterpret_cast<long long *>(stats)[0] = tiles_per_b;
  }
}

template <typename T, int MBW, int MBH, int MBD, int KD, int SD, int SH, int SW>
int launch_conva(const ConvLaunch &L, const ConvClasses &cs) {
  typedef CfgA<T, MBW, MBH, MBD, KD, SD, SH, SW> Cfg;
  typedef typename Cfg::G G;
  static_assert(Cfg::LDS_BYTES <= 160 * 1024, "conva tile does not fit the LDS");
  auto kern = conva_mfma_kernel<T, MBW, MBH, MBD, KD, SD, SH, SW>;
  static DynLdsOnce lds_once;
  DG_REQUIRE(ensure_dyn_lds(lds_once, reinterpret_cast<const void *>(kern), (int)Cfg::LDS_BYTES) == hipSuccess, DGTTA_ERR_LAUNCH,
             "conv3d_fwd: cannot raise the dynamic LDS limit to %zu", (size_t)Cfg::LDS_BYTES);
  const View &yv = L.yv;
  const int tW = cdiv(yv.W, G::TW), tH = cdiv(yv.H, G::TH), tD = cdiv(yv.D, G::TD);
  const int64_t tiles = (int64_t)tW * tH * tD * L.B;
  DG_REQUIRE(tiles < (1ll << 31), DGTTA_ERR_UNSUPPORTED, "conv3d_fwd: too many tiles");
  DG_REQUIRE(!L.stats || (int64_t)tW * tH * tD <= conv3_mfma_max_tiles(yv.D, yv.H, yv.W), DGTTA_ERR_UNSUPPORTED,
             "conv3d_fwd: tile count exceeds the statistics buffer");
  dim3 grid((unsigned)tiles, (unsigned)cdiv(L.CoutP, Cfg::NC), (unsigned)cs.n);
  hipLaunchKernelGGL(kern, grid, dim3(Cfg::NW * 64), Cfg::LDS_BYTES, L.st, (const T *)L.x, L.xv, (const T *)L.w, cs, L.bias, (T *)L.y,
                     yv, L.Cin, L.Cout, L.CinP, tW, tH, tD, L.stats, L.ntaps_src);
  DG_CHECK_LAUNCH("conva_mfma_kernel");
  return DGTTA_OK;
}

// tile shape from the output extent: (TD, TH, TW) = (4, 4, 32) where the halo fits the LDS (SD = 1), else (4, 4, 16) or
// (4, 8, 8); each is a shape of conv3_mfma_max_tiles, so the InstanceNorm partial sums fit dgtta_conv3d_stats_bytes
template <typename T, int KD, int SD, int SH, int SW>
int dispatch_conva(const ConvLaunch &L, const ConvClasses &cs) {
  if constexpr (SD == 1)
    if (L.yv.W >= 32) return launch_conva<T, 32, 4, 4, KD, SD, SH, SW>(L, cs);
  if (L.yv.W >= 16) return launch_conva<T, 16, 2, 4, KD, SD, SH, SW>(L, cs);
  return launch_conva<T, 8, 2, 4, KD, SD, SH, SW>(L, cs);
}

template <typename T, int KD>
int dispatch_conva_strides(const ConvLaunch &L, const ConvClasses &cs, int sd, int sh, int sw) {
  switch ((sd - 1) * 4 + (sh - 1) * 2 + (sw - 1)) {
    case 0: return dispatch_conva<T, KD, 1, 1, 1>(L, cs);
    case 1: return dispatch_conva<T, KD, 1, 1, 2>(L, cs);
    case 2: return dispatch_conva<T, KD, 1, 2, 1>(L, cs);
    case 3: return dispatch_conva<T, KD, 1, 2, 2>(L, cs);
    case 4: return dispatch_conva<T, KD, 2, 1, 1>(L, cs);
    case 5: return dispatch_conva<T, KD, 2, 1, 2>(L, cs);
    case 6: return dispatch_conva<T, KD, 2, 2, 1>(L, cs);
    case 7: return dispatch_conva<T, KD, 2, 2, 2>(L, cs);
  }
  return DGTTA_ERR_UNSUPPORTED;
}

template <typename T>
int run_conva(const ConvLaunch &L, const ConvClasses &cs, int kd, int sd, int sh, int sw) {
  if (kd == 1) return dispatch_conva_strides<T, 1>(L, cs, sd, sh, sw);
  return dispatch_conva_strides<T, 3>(L, cs, sd, sh, sw);
}

// dtype: one of the three storage types (the entry points check dtype_ok first)
int run_conva_dt(int dtype, const ConvLaunch &L, const ConvClasses &cs, int kd, int sd, int sh, int sw) {
  DISPATCH_T(dtype, return run_conva<T>(L, cs, kd, sd, sh, sw));
}

}  // namespace

// (the shared checks of conv_api.h with cap: this family bounds the channel counts at 2^16)
extern "C" size_t dgtta_conv3d_kpacked_bytes(int kd, int CinP, int CoutP, int dtype) {
  if ((kd != 1 && kd != 3) || CinP <= 0 || CoutP <= 0 || CinP > (1 << 16) || CoutP > (1 << 16) || !dtype_ok(dtype)) return 0;
  return (size_t)kd * 9 * ((size_t)CinP * n32(CoutP) + (size_t)CoutP * n32(CinP)) * esize(dtype);
}

extern "C" int dgtta_conv3d_kpack_weights(const float *w_t, void *wpack, int kd, int kh, int kw, int Cin, int Cout, int CinP,
                                          int CoutP, int dtype, void *stream) {
  DG_REQUIRE(w_t && wpack, DGTTA_ERR_BADARG, "conv3d_kpack_weights: null pointer");
  DG_REQUIRE(Cin > 0 && Cout > 0 && CinP >= Cin && CoutP >= Cout && CinP <= (1 << 16) && CoutP <= (1 << 16), DGTTA_ERR_BADARG,
             "conv3d_kpack_weights: bad channel counts");
  DG_REQUIRE((kd == 1 || kd == 3) && kh == 3 && kw == 3, DGTTA_ERR_UNSUPPORTED,
             "conv3d_kpack_weights: kernel %dx%dx%d (supported: [1|3] x 3 x 3)", kd, kh, kw);
  DG_REQUIRE(dtype_ok(dtype), DGTTA_ERR_UNSUPPORTED, "conv3d_kpack_weights: dtype %d", dtype);
  DG_REQUIRE(CinP % conv_granule(dtype) == 0 && CoutP % conv_granule(dtype) == 0, DGTTA_ERR_BADARG,
             "conv3d_kpack_weights: padded channel counts must be multiples of %d", conv_granule(dtype));
  const ConvProblem P{0, Cin, Cout, CinP, CoutP, 0, 0, 0, kd, 1, 1, 1, dtype, (hipStream_t)stream};
  return conv_pack_images(P, w_t, wpack);
}

extern "C" int dgtta_conv3d_fwd(const void *x, int ldx, const void *wpack, const float *bias, void *y, int ldy, void *stats, int B,
                                int Cin, int Cout, int CinP, int CoutP, int Di, int Hi, int Wi, int kd, int sd, int sh, int sw,
                                int dtype, void *stream) {
  static const char fn[] = "conv3d_fwd";
  const ConvProblem P{B, Cin, Cout, CinP, CoutP, Di, Hi, Wi, kd, sd, sh, sw, dtype, (hipStream_t)stream};
  CONV_REQUIRE_PTRS(fn, x && wpack && y);
  CONV_REQUIRE_DIMS(fn, P, true, true);
  CONV_REQUIRE_LD(fn, ldx >= Cin && ldy >= Cout);
  CONV_REQUIRE_KERNEL(fn, P);
  DG_REQUIRE(operand_ok(epv_of(dtype), x, ldx, Cin, CinP), DGTTA_ERR_UNSUPPORTED,
             "conv3d_fwd: x must be 16-byte aligned with rows of whole 16 bytes, CinP a multiple of %d", conv_granule(dtype));
  Taps taps;
  for (int t = 0; t < 27; ++t) taps.wt[t] = (signed char)(t < P.ntaps() ? t : -1);
  const ConvLaunch L{x, dense_view(B, Di, Hi, Wi, ldx), wpack, bias, y, dense_view(B, P.Do(), P.Ho(), P.Wo(), ldy), B, Cin, Cout, CinP,
                     CoutP, (double *)stats, P.ntaps(), P.st};
  return run_conva_dt(dtype, L, single_class(taps, 0), kd, sd, sh, sw);
}

extern "C" int dgtta_conv3d_dgrad(const void *dy, int lddy, const void *wpack, void *dx, int lddx, int B, int Cin, int Cout, int CinP,
                                  int CoutP, int Di, int Hi, int Wi, int kd, int sd, int sh, int sw, int accumulate, int dtype,
                                  void *stream) {
  static const char fn[] = "conv3d_dgrad";
  const ConvProblem P{B, Cin, Cout, CinP, CoutP, Di, Hi, Wi, kd, sd, sh, sw, dtype, (hipStream_t)stream};
  CONV_REQUIRE_PTRS(fn, dy && wpack && dx);
  CONV_REQUIRE_DIMS(fn, P, true, true);
  CONV_REQUIRE_LD(fn, lddx >= Cin && lddy >= Cout);
  CONV_REQUIRE_KERNEL(fn, P);
  CONV_REQUIRE_EVEN(fn, P);
  DG_REQUIRE(operand_ok(epv_of(dtype), dy, lddy, Cout, CoutP), DGTTA_ERR_UNSUPPORTED,
             "conv3d_dgrad: dy must be 16-byte aligned with rows of whole 16 bytes, CoutP a multiple of %d", conv_granule(dtype));
  const void *imgB = (const char *)wpack + (size_t)P.ntaps() * CinP * n32(CoutP) * esize(dtype);
  // one stride-1 class per parity of the strided axes
  View yv;
  const ConvClasses cs = dgrad_parity_classes(P, lddx, accumulate, &yv);
  const ConvProblem G = dgrad_as_fwd(P);
  const ConvLaunch L{dy, dense_view(B, P.Do(), P.Ho(), P.Wo(), lddy), imgB, nullptr, dx, yv, B, G.Cin, G.Cout, G.CinP, G.CoutP, nullptr,
                     P.ntaps(), P.st};
  return run_conva_dt(dtype, L, cs, kd, 1, 1, 1);
}

// workspace: [bias partials][weight-gradient slabs] (conv_wgrad_ws_layout)
extern "C" size_t dgtta_conv3d_kwgrad_ws_bytes(int B, int Cin, int Cout, int Di, int Hi, int Wi, int kd, int sd, int sh, int sw) {
  const ConvProblem P{B, Cin, Cout, Cin, Cout, Di, Hi, Wi, kd, sd, sh, sw, DGTTA_F32, nullptr};
  if (!conv_dims_ok(P, true) || !kernel_ok(P)) return 0;
  return conv_wgrad_ws_layout(P, true).total();
}

extern "C" int dgtta_conv3d_wgrad(const void *x, int ldx, const void *dy, int lddy, float *dw_t, float *db, void *ws, size_t ws_bytes,
                                  int B, int Cin, int Cout, int Di, int Hi, int Wi, int kd, int sd, int sh, int sw, int accumulate,
                                  int dtype, void *stream) {
  static const char fn[] = "conv3d_wgrad";
  const ConvProblem P{B, Cin, Cout, Cin, Cout, Di, Hi, Wi, kd, sd, sh, sw, dtype, (hipStream_t)stream};
  CONV_REQUIRE_PTRS(fn, x && dy && dw_t && ws);
  CONV_REQUIRE_DIMS(fn, P, true, ldx >= Cin && lddy >= Cout);
  CONV_REQUIRE_KERNEL(fn, P);
  CONV_REQUIRE_EVEN(fn, P);
  const ConvWsLayout lay = conv_wgrad_ws_layout(P, true);
  CONV_REQUIRE_WS(fn, ws_bytes, lay.total());
  const int rc = conva_wgrad_mfma(P, Src{x, ldx}, Src{dy, lddy}, dw_t, lay.main_of(ws, ws_bytes), accumulate);
  if (rc == DGTTA_ERR_UNSUPPORTED)
    dgtta_set_error("conv3d_wgrad: operands not taken by the MFMA kernel (16-byte aligned rows, Cout a multiple of %d)",
                    dtype == DGTTA_F32 ? 4 : 8);
  if (rc != DGTTA_OK) return rc;
  if (db) return conv_bias_grad(dy, lddy, db, ws, B, Cout, P.out_vox(), accumulate, dtype, P.st);
  return DGTTA_OK;
}

// ---- ConvTranspose3d with kernel = stride (sd, sh, sw) in {1, 2}^3, not all 1:
//      out[b][s*v + o][co] = bias[co] + sum_ci x[b][v][ci] w[ci][co][o]
extern "C" size_t dgtta_convT3d_s_fwd_ws_bytes(int Cin, int Cout, int sd, int sh, int sw, int dtype) {
  const ConvProblem P{1, Cin, Cout, Cin, Cout, 1, 1, 1, sd, sd, sh, sw, dtype, nullptr};
  if (!conv_dims_ok(P, true) || !convt_strides_ok(P) || !dtype_ok(dtype)) return 0;
  return convT_pack_region(Cin, Cout, dtype);
}

extern "C" int dgtta_convT3d_s_fwd(const void *x, int ldx, const float *w_t, const float *bias, void *out, int ldo, void *ws,
                                   size_t ws_bytes, int B, int Cin, int Cout, int Di, int Hi, int Wi, int sd, int sh, int sw, int dtype,
                                   void *stream) {
  static const char fn[] = "convT3d_s_fwd";
  const ConvProblem P{B, Cin, Cout, Cin, Cout, Di, Hi, Wi, sd, sd, sh, sw, dtype, (hipStream_t)stream};
  CONV_REQUIRE_PTRS(fn, x && w_t && out && ws);
  CONV_REQUIRE_DIMS(fn, P, true, ldx >= Cin && ldo >= Cout);
  CONV_REQUIRE_CONVT_STRIDES(fn, P);
  CONV_REQUIRE_WS(fn, ws_bytes, convT_pack_region(Cin, Cout, dtype));
  const int rc = convTa_run(P, 0, Src{x, ldx}, w_t, bias, Dst{out, ldo}, ws);
  if (rc == DGTTA_ERR_UNSUPPORTED) dgtta_set_error("convT3d_s_fwd: x must be 16-byte aligned with rows of whole 16 bytes");
  return rc;
}

// workspace: [bias partials][packed weights][weight-gradient slabs] (convT_bwd_ws_layout)
extern "C" size_t dgtta_convT3d_s_bwd_ws_bytes(int B, int Cin, int Cout, int Di, int Hi, int Wi, int sd, int sh, int sw) {
  const ConvProblem P{B, Cin, Cout, Cin, Cout, Di, Hi, Wi, sd, sd, sh, sw, DGTTA_F32, nullptr};
  if (!conv_dims_ok(P, true) || !convt_strides_ok(P)) return 0;
  return convT_bwd_ws_layout(P, true).total();
}

extern "C" int dgtta_convT3d_s_bwd(const void *x, int ldx, const void *dout, int lddo, const float *w_t, void *dx, int lddx, float *dw_t,
                                   float *db, void *ws, size_t ws_bytes, int B, int Cin, int Cout, int Di, int Hi, int Wi, int sd, int sh,
                                   int sw, int accumulate, int dtype, void *stream) {
  static const char fn[] = "convT3d_s_bwd";
  const ConvProblem P{B, Cin, Cout, Cin, Cout, Di, Hi, Wi, sd, sd, sh, sw, dtype, (hipStream_t)stream};
  const Src xs{x, ldx}, dos{dout, lddo};
  CONV_REQUIRE_PTRS(fn, x && dout && w_t && ws);
  CONV_REQUIRE_DIMS(fn, P, true, ldx >= Cin && lddo >= Cout);
  CONV_REQUIRE_CONVT_STRIDES(fn, P);
  const ConvWsLayout lay = convT_bwd_ws_layout(P, true);
  CONV_REQUIRE_WS(fn, ws_bytes, lay.total());
  if (dx) {
    DG_REQUIRE(lddx >= Cin, DGTTA_ERR_BADARG, "convT3d_s_bwd: lddx < Cin");
    const int rc = convTa_run(P, 1, dos, w_t, nullptr, Dst{dx, lddx}, lay.pack_of(ws));
    if (rc == DGTTA_ERR_UNSUPPORTED) dgtta_set_error("convT3d_s_bwd: dout must be 16-byte aligned with rows of whole 16 bytes");
    if (rc != DGTTA_OK) return rc;
  }
  if (dw_t) {
    const int rc = convTa_wgrad_mfma(P, xs, dos, dw_t, lay.main_of(ws, ws_bytes), accumulate);
    if (rc == DGTTA_ERR_UNSUPPORTED)
      dgtta_set_error("convT3d_s_bwd: operands not taken by the MFMA kernel (16-byte aligned rows, Cout a multiple of %d)",
                      dtype == DGTTA_F32 ? 4 : 8);
    if (rc != DGTTA_OK) return rc;
  }
  if (db) return conv_bias_grad(dout, lddo, db, ws, B, Cout, P.t_vox(), accumulate, dtype, P.st);
  return DGTTA_OK;
}
