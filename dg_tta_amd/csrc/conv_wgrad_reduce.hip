// Slab reduction of the weight-gradient kernels: sums the fp32 partial slabs [27][32 ci][32 co] that the workgroups of a launch
// left, in a fixed order, into the caller's weight-gradient layout.
#include "conv_wgrad_common.h"

namespace {

// dw[co*s_co + ci*s_ci + real_tap*s_tap] (+)= sum over slabs of virtual tap t (real_tap = real.wt[t], -1: skip).
// Workgroup = 32 consecutive output channels (one coalesced 128-byte row of every slab) x 8 slab groups; the 8 partial
// sums are combined through LDS in fixed order (deterministic).
template <int G>   // G slab groups per output row (8: many slabs, 1: few slabs -> 8 output rows per workgroup)
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float *__restrict__ slabs, float *__restrict__ dw, int Cin,
                                                           int Cout, int cobs, int npairs, int nslab, int accumulate,
                                                           RealTaps reals, long long s_co, long long s_ci,
                                                           long long s_tap) {
  const Taps &real = reals.t[blockIdx.y];
  slabs += (int64_t)blockIdx.y * npairs * nslab * (27 * 1024);
  constexpr int R = 8 / G;                  // output rows (tap, ci, co-block) per workgroup
  __shared__ float part[8][32];
  const int lane = threadIdx.x & 31, sub = threadIdx.x >> 5;
  const int grp = sub % G, rsel = sub / G;
  const int cobs32 = (Cout + 31) / 32;
  const int64_t nrows = (int64_t)27 * Cin * cobs32;
  int64_t t = (int64_t)blockIdx.x * R + rsel;
  const bool live = t < nrows;
  if (!live) t = 0;
  const int cb = (int)(t % cobs32);
  t /= cobs32;
  const int ci = (int)(t % Cin);
  const int tap = (int)(t / Cin);
  const int rt = real.wt[tap];
  const int co = cb * 32 + lane;
  const bool ok = live && rt >= 0 && co < Cout;
  float s = 0.f;
  if (ok) {
    const int pair = (ci >> 5) * cobs + cb;
    const float *p = slabs + (int64_t)pair * nslab * (27 * 1024) + (tap * 32 + (ci & 31)) * 32 + lane;
    // eight slabs are requested before the first is added (round 4): one dependent load per slab made the launch a chain
    // of nslab / G memory round trips (32 us for 256 slabs).  The additions keep their order: same sums, bit for bit.
    for (int k = grp; k < nslab; k += 8 * G) {
      float v[8];
#pragma unroll
      for (int j = 0; j < 8; ++j) v[j] = (k + j * G < nslab) ? p[(int64_t)(k + j * G) * (27 * 1024)] : 0.f;
#pragma unroll
      for (int j = 0; j < 8; ++j)
        if (k + j * G < nslab) s += v[j];
    }
  }
  if (G > 1) {
    part[sub][lane] = s;
    __syncthreads();
    if (grp == 0) {
      s = 0.f;
#pragma unroll
      for (int g = 0; g < G; ++g) s += part[rsel * G + g][lane];
    }
  }
  if (grp == 0 && ok) {
    float *o = dw + co * s_co + ci * s_ci + rt * s_tap;
    *o = accumulate ? *o + s : s;
  }
}

// Few slabs (< 64) into the dense layout dw_t[co][ci][27], round 6.  The kernel above gives each output row (tap, ci, co-block)
// to 32 lanes: coalesced slab reads, but the 27 floats of a (ci, co) are written by workgroups far apart in the grid, as
// 4-byte stores 100+ KB apart, so every 128-byte line of dw goes to memory in pieces (the 22 MB of the 640 -> 320 layer took
// 77 us, 4x the 11 MB of a 320 -> 320 layer).  Here a workgroup owns 8 input channels x 32 output channels: thread (ci, co)
// sums its 27 taps over the slabs (9 taps x 4 slabs in flight; slabs in ascending order: the same bits as above), the sums
// meet in LDS, and each output channel's 8 x 27 = 216 consecutive floats leave as 54 float4 of one wave instruction.
__global__ __launch_bounds__(256) void wgrad_reduce_taps_kernel(const float *__restrict__ slabs, float *__restrict__ dw, int Cin,
                                                                int Cout, int cobs, int nslab, int accumulate, long long s_co) {
  __shared__ float stg[32][217];
  const int lane = threadIdx.x & 31, sub = threadIdx.x >> 5;
  const int cobs32 = (Cout + 31) / 32;
  const int cb = blockIdx.x % cobs32, ci0 = (blockIdx.x / cobs32) * 8;      // (Cin % 8 == 0: the launcher checks)
  const int ci = ci0 + sub;
  const float *p = slabs + (int64_t)((ci >> 5) * cobs + cb) * nslab * (27 * 1024) + (ci & 31) * 32 + lane;
#pragma unroll 1
  for (int t0 = 0; t0 < 27; t0 += 9) {
    float s[9];
#pragma unroll
    for (int t = 0; t < 9; ++t) s[t] = 0.f;
    for (int k = 0; k < nslab; k += 4) {
      float v[9][4];
#pragma unroll
      for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int j = 0; j < 4; ++j) v[t][j] = p[(int64_t)(k + j < nslab ? k + j : k) * (27 * 1024) + (t0 + t) * 1024];
#pragma unroll
      for (int t = 0; t < 9; ++t)
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (k + j < nslab) s[t] += v[t][j];
    }
#pragma unroll
    for (int t = 0; t < 9; ++t) stg[lane][sub * 27 + t0 + t] = s[t];
  }
  __syncthreads();
  const int wv = threadIdx.x >> 6, l = threadIdx.x & 63;
  if (l < 54) {
#pragma unroll
    for (int r = 0; r < 8; ++r) {
      const int cl = wv + 4 * r, co = cb * 32 + cl;
      if (co >= Cout) break;
      float4 o = make_float4(stg[cl][4 * l], stg[cl][4 * l + 1], stg[cl][4 * l + 2], stg[cl][4 * l + 3]);
      float4 *dst = (float4 *)(dw + co * s_co + (int64_t)ci0 * 27) + l;
      if (accumulate) {
        const float4 old = *dst;
        o.x += old.x, o.y += old.y, o.z += old.z, o.w += old.w;
      }
      *dst = o;
    }
  }
}

}  // namespace

// the dense-layout reduction (wgrad_reduce_taps_kernel) takes: all 27 taps in place, dw_t[co][ci][27], whole groups of 8 input
// channels, 16-byte aligned rows (DGTTA_WGRAD_REDUCE_TAPS=0, tests: always the row kernel)
static bool reduce_taps_ok(const Taps *real, const float *dw, int Cin, long long s_ci, long long s_tap) {
  if (!real || dgtta_switches().wgrad_reduce_taps == '0' || s_tap != 1 || s_ci != 27 || Cin % 8 || ((uintptr_t)dw & 15)) return false;
  for (int t = 0; t < 27; ++t)
    if (real->wt[t] != t) return false;
  return true;
}

int wgrad_reduce_launch(const WgradLaunch &L, const WgradOut &out, const WgradPlan &p, int ncls, int64_t nslab, const RealTaps &reals) {
  const float *slabs = (const float *)L.ws;
  const int Cin = L.Cin, Cout = L.Cout;
  const int64_t rrows = (int64_t)27 * Cin * ((Cout + 31) / 32);
  const int npairs = p.cibs * p.cobs;
  if (nslab >= 64)
    hipLaunchKernelGGL(wgrad_reduce_kernel<8>, dim3((unsigned)rrows, (unsigned)ncls), dim3(256), 0, L.st, slabs, out.dw, Cin, Cout, p.cobs,
                       npairs, (int)nslab, out.accumulate, reals, out.s_co, out.s_ci, out.s_tap);
  else if (reduce_taps_ok(ncls == 1 ? &reals.t[0] : nullptr, out.dw, Cin, out.s_ci, out.s_tap))
    hipLaunchKernelGGL(wgrad_reduce_taps_kernel, dim3((unsigned)((Cin / 8) * ((Cout + 31) / 32))), dim3(256), 0, L.st, slabs, out.dw, Cin,
                       Cout, p.cobs, (int)nslab, out.accumulate, out.s_co);
  else
    hipLaunchKernelGGL(wgrad_reduce_kernel<1>, dim3((unsigned)cdiv64(rrows, 8), (unsigned)ncls), dim3(256), 0, L.st, slabs, out.dw, Cin,
                       Cout, p.cobs, npairs, (int)nslab, out.accumulate, reals, out.s_co, out.s_ci, out.s_tap);
  DG_CHECK_LAUNCH("wgrad_reduce_kernel");
  return DGTTA_OK;
}
