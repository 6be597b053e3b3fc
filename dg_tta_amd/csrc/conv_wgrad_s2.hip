// Weight gradient of the stride-2 3x3x3 convolutions in one pass on the matrix cores (16-bit storage, even input extents).
#include "conv_wgrad_common.h"

namespace {

// ---------------------------------------------------------------------------------------------------------------------
// bf16 weight gradient of a STRIDE-2 conv in one pass:  dW[tap][ci][co] = sum_vo x[2 vo + tap - 1][ci] * dy[vo][co].
// Same scheme as conv3_wgrad_tr_kernel (conv_wgrad_rows.hip: LDS-DMA staging, ds_read_b64_tr_b16 operands, 7 taps per wave, slab output) with
// the x tile kept at FULL resolution: output tile 2 rows x 16 voxels needs x rows 2h0-1 .. 2h0+3 and voxels 2w0-1 ..
// 2w0+31; output slice d needs x slices 2d-1, 2d, 2d+1 (ring of 5: 3 live + 2 arriving).  The transposed read takes one
// row address per lane, so "every second voxel" is just a 128-byte row stride of the operand block.  dy is read once and x
// once (+ halo), instead of 8 parity-class passes that each re-read dy and gathered x with half-used cache lines.
template <typename T16 = bf16_t>
__global__ __launch_bounds__(256, 2) void conv3_wgrad_tr_s2_kernel(const bf16_t *__restrict__ x, View xv,
                                                                   const bf16_t *__restrict__ dy, View yv,
                                                                   float *__restrict__ slabs, int Cin, int Cout, int tilesW,
                                                                   int tilesH, int nsd, int DR, int cobs) {
  const int D = yv.D, H = yv.H, W = yv.W;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char *sX = smem;
  unsigned char *sY = smem + WT2::NXS * WT2::X_SLICE_B;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

  int t = xcd_unit(1);
  const int tw = t % tilesW;
  t /= tilesW;
  const int th = t % tilesH;
  t /= tilesH;
  const int ds = t % nsd;
  const int b = t / nsd;
  const int cib = blockIdx.y / cobs, cob = blockIdx.y % cobs;
  const int h0 = th * WT2::TH, w0 = tw * WT2::TWO;
  const int d_begin = ds * DR, d_end = (d_begin + DR < D) ? d_begin + DR : D;
  const bf16_t *xb = x + b * xv.sb + cib * 32;
  const bf16_t *yb = dy + b * yv.sb + cob * 32;
  const int cin_lim = (Cin + 7) / 8 * 8;
  const int l_vox = lane >> 2, l_chunk = lane & 3;

  auto xslot = [&](int xd) { return (xd + WT2::NXS) % WT2::NXS; };
  // piece i of this wave for output slice `od`: x slices 2od-1+{s} (s given by the piece index) and the dy slice
  auto issue_x_slice = [&](int xd, int i) __attribute__((always_inline)) {      // piece index idx = wave + 4 i < NPX1
    const int idx = wave + 4 * i;
    if (idx >= WT2::NPX1) return;
    const int r = idx / 3, pi = idx % 3;
    if (pi == 2 && lane >= 4) return;
    const int gh = 2 * h0 - 1 + r, wx = 16 * pi + l_vox, gw = 2 * w0 - 1 + wx;
    const bool ok = (unsigned)xd < (unsigned)xv.D && (unsigned)gh < (unsigned)xv.H && (unsigned)gw < (unsigned)xv.W &&
                    cib * 32 + l_chunk * 8 < cin_lim;
    const void *src = ok ? (const void *)(xb + xd * xv.sd + gh * xv.sh + gw * xv.sw + l_chunk * 8) : (const void *)&g_zero16;
    dma16_to_lds(src, lds_addr_of(sX + xslot(xd) * WT2::X_SLICE_B + r * WT2::X_ROW_B + pi * 1024));
  };
  auto issue_y_slice = [&](int yd) __attribute__((always_inline)) {             // rows 0/1 by waves 0/1
    if (wave >= WT2::TH) return;
    const int gh = h0 + wave, gw = w0 + l_vox;
    const bool ok = (unsigned)yd < (unsigned)D && gh < H && gw < W && cob * 32 + l_chunk * 8 < Cout;
    const void *src = ok ? (const void *)(yb + yd * yv.sd + gh * yv.sh + gw * yv.sw + l_chunk * 8) : (const void *)&g_zero16;
    dma16_to_lds(src, lds_addr_of(sY + (yd & 1) * WT2::Y_SLICE_B + wave * WT2::Y_ROW_B));
  };
  constexpr int NPXW = (WT2::NPX1 + 3) / 4;      // x pieces per wave and x slice

  // transposed-read lane addresses: dy block rows are consecutive voxels (64 B), x block rows every second voxel (128 B)
  const int kq = (lane >> 5) * 8 + ((lane & 15) >> 2), cpart = ((lane >> 4) & 1) * 32 + (lane & 3) * 8;
  const int lane_off_y = kq * 64 + cpart, lane_off_x = kq * 128 + cpart;

  int tap_kd[7], tap_off[7];
#pragma unroll
  for (int i = 0; i < 7; ++i) {
    const int tc = wave + 4 * i < 27 ? wave + 4 * i : 26;
    tap_kd[i] = tc / 9;
    tap_off[i] = ((tc / 3) % 3) * WT2::X_ROW_B + (tc % 3) * 64;
  }
  f32x16_t acc[7];
#pragma unroll
  for (int i = 0; i < 7; ++i)
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[i][q] = 0.f;

  // prologue: x slices 2 d_begin - 1 .. 2 d_begin + 1, dy slice d_begin
#pragma unroll
  for (int sl = -1; sl <= 1; ++sl)
#pragma unroll
    for (int i = 0; i < NPXW; ++i) issue_x_slice(2 * d_begin + sl, i);
  issue_y_slice(d_begin);
  dma_wait_all();
  lds_barrier();

  for (int d = d_begin; d < d_end; ++d) {
    if (d + 1 < d_end) {       // next output slice: x slices 2d+2, 2d+3 and dy slice d+1 land during the MFMAs below
#pragma unroll
      for (int i = 0; i < NPXW; ++i) issue_x_slice(2 * d + 2, i);
#pragma unroll
      for (int i = 0; i < NPXW; ++i) issue_x_slice(2 * d + 3, i);
      issue_y_slice(d + 1);
    }
    const unsigned char *ys = sY + (d & 1) * WT2::Y_SLICE_B + lane_off_y;
    int slice_off[3];
#pragma unroll
    for (int kd = 0; kd < 3; ++kd) slice_off[kd] = xslot(2 * d + kd - 1) * WT2::X_SLICE_B;
    int so_t[7];
#pragma unroll
    for (int i = 0; i < 7; ++i) so_t[i] = (tap_kd[i] == 0 ? slice_off[0] : (tap_kd[i] == 1 ? slice_off[1] : slice_off[2])) + tap_off[i];
#pragma unroll
    for (int oh = 0; oh < WT2::TH; ++oh) {
      // K-step = the 16 output voxels of the row
      const s16x4_t blo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_t *)(ys + oh * WT2::Y_ROW_B));
      const s16x4_t bhi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_t *)(ys + oh * WT2::Y_ROW_B + 4 * 64));
      const s16x8_t bv = {blo[0], blo[1], blo[2], blo[3], bhi[0], bhi[1], bhi[2], bhi[3]};
      const bf16x8_t bfr = __builtin_bit_cast(bf16x8_t, bv);
      bf16x8_t afr[7];
#pragma unroll
      for (int i = 0; i < 7; ++i) {
        const unsigned char *pa = sX + lane_off_x + so_t[i] + 2 * oh * WT2::X_ROW_B;
        const s16x4_t alo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_t *)pa);
        const s16x4_t ahi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_t *)(pa + 4 * 128));
        const s16x8_t av = {alo[0], alo[1], alo[2], alo[3], ahi[0], ahi[1], ahi[2], ahi[3]};
        afr[i] = __builtin_bit_cast(bf16x8_t, av);
      }
#pragma unroll
      for (int i = 0; i < 7; ++i) acc[i] = mfma32_tr<T16>(afr[i], bfr, acc[i]);
    }
    dma_wait_all();
    lds_barrier();
  }

  float *slab = slabs + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * (27 * 1024);
  const int co = lane & 31, hh = lane >> 5;
#pragma unroll
  for (int i = 0; i < 7; ++i) {
    const int tap = wave + 4 * i;
    if (tap < 27) {
#pragma unroll
      for (int q = 0; q < 16; ++q) slab[(tap * 32 + (q & 3) + 8 * (q >> 2) + 4 * hh) * 32 + co] = acc[i][q];
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// The same for TWO output-channel blocks per workgroup (round 4): 8 waves, waves 0-3 / 4-7 take the 27 taps of block 0 / 1 and
// share the x tile.  With one block per workgroup a 32 -> 64 layer read x - four times the bytes of dy, the whole traffic of this
// HBM-bound kernel - once per block (2.8 GB at the 128^3 -> 64^3 transition where 1.3 GB are the operands; 853 us).  One
// 512-thread workgroup per CU halves the loads in flight, so the ring is two output slices ahead instead of one (7 x slots,
// 3 dy slots) and a step waits with a counted vmcnt for the slices of the NEXT step only; every wave issues the same five
// pieces per step (a wave without a piece of its own repeats a neighbour's: same bytes to the same address).
struct WT2X {
  static constexpr int NCO = 2, LA = 2;
  static constexpr int NXS = 3 + 2 * LA, NYS = LA + 1;
  static constexpr int Y_STEP_B = NCO * WT2::Y_SLICE_B;
  static constexpr int LDS_BYTES = NXS * WT2::X_SLICE_B + NYS * Y_STEP_B;
};

template <typename T16 = bf16_t>
__global__ __launch_bounds__(512, 2) void conv3_wgrad_tr_s2x_kernel(const bf16_t *__restrict__ x, View xv,
                                                                    const bf16_t *__restrict__ dy, View yv,
                                                                    float *__restrict__ slabs, int Cin, int Cout, int tilesW,
                                                                    int tilesH, int nsd, int DR, int cobs) {
  const int D = yv.D, H = yv.H, W = yv.W;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char *sX = smem;
  unsigned char *sY = smem + WT2X::NXS * WT2::X_SLICE_B;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int tg = wave & 3, cb = wave >> 2;                 // tap group, output-channel block of the pair

  int t = xcd_unit(1);
  const int tw = t % tilesW;
  t /= tilesW;
  const int th = t % tilesH;
  t /= tilesH;
  const int ds = t % nsd;
  const int b = t / nsd;
  const int cogs = cobs / 2;
  const int cib = blockIdx.y / cogs, cog = blockIdx.y % cogs;
  const int h0 = th * WT2::TH, w0 = tw * WT2::TWO;
  const int d_begin = ds * DR, d_end = (d_begin + DR < D) ? d_begin + DR : D;
  const bf16_t *xb = x + b * xv.sb + cib * 32;
  const bf16_t *yb = dy + b * yv.sb + cog * 64;
  const int cin_lim = (Cin + 7) / 8 * 8;
  const int l_vox = lane >> 2, l_chunk = lane & 3;

  auto xslot = [&](int xd) { return (xd + WT2X::NXS) % WT2X::NXS; };
  // 15 pieces per x slice over 8 waves: pieces wave and wave + 8 (the 16th repeats piece 14)
  auto issue_x_slice = [&](int xd) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < 2; ++i) {
      int idx = wave + 8 * i;
      idx = idx < WT2::NPX1 ? idx : WT2::NPX1 - 1;
      const int r = idx / 3, pi = idx % 3;
      const int gh = 2 * h0 - 1 + r, wx = 16 * pi + l_vox, gw = 2 * w0 - 1 + wx;
      // the third piece of a row is one voxel (4 lanes): the other lanes write zeros into the unused tail of the LDS row
      const bool ok = (unsigned)xd < (unsigned)xv.D && (unsigned)gh < (unsigned)xv.H && (unsigned)gw < (unsigned)xv.W &&
                      cib * 32 + l_chunk * 8 < cin_lim && (pi < 2 || lane < 4);
      const void *src = ok ? (const void *)(xb + xd * xv.sd + gh * xv.sh + gw * xv.sw + l_chunk * 8) : (const void *)&g_zero16;
      if (pi < 2 || lane < 12)      // voxels 32 .. 34 of the 36-voxel LDS row
        dma16_to_lds(src, lds_addr_of(sX + xslot(xd) * WT2::X_SLICE_B + r * WT2::X_ROW_B + pi * 1024));
    }
  };
  // 4 pieces per dy slice (2 rows x 2 blocks): piece wave & 3
  auto issue_y_slice = [&](int yd) __attribute__((always_inline)) {
    const int row = wave & 1, blk = (wave >> 1) & 1;
    const int gh = h0 + row, gw = w0 + l_vox;
    const bool ok = (unsigned)yd < (unsigned)D && gh < H && gw < W && cog * 64 + blk * 32 + l_chunk * 8 < Cout;
    const void *src = ok ? (const void *)(yb + yd * yv.sd + gh * yv.sh + gw * yv.sw + blk * 32 + l_chunk * 8)
                         : (const void *)&g_zero16;
    dma16_to_lds(src, lds_addr_of(sY + (yd % WT2X::NYS) * WT2X::Y_STEP_B + blk * WT2::Y_SLICE_B + row * WT2::Y_ROW_B));
  };
  auto issue_step = [&](int od) __attribute__((always_inline)) {      // x slices 2 od, 2 od + 1 and dy slice od: 5 pieces per wave
    issue_x_slice(2 * od);
    issue_x_slice(2 * od + 1);
    issue_y_slice(od);
  };

  const int kq = (lane >> 5) * 8 + ((lane & 15) >> 2), cpart = ((lane >> 4) & 1) * 32 + (lane & 3) * 8;
  const int lane_off_y = kq * 64 + cpart, lane_off_x = kq * 128 + cpart;

  int tap_kd[7], tap_off[7];
#pragma unroll
  for (int i = 0; i < 7; ++i) {
    const int tc = tg + 4 * i < 27 ? tg + 4 * i : 26;
    tap_kd[i] = tc / 9;
    tap_off[i] = ((tc / 3) % 3) * WT2::X_ROW_B + (tc % 3) * 64;
  }
  f32x16_t acc[7];
#pragma unroll
  for (int i = 0; i < 7; ++i)
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[i][q] = 0.f;

  // prologue: x slice 2 d_begin - 1, then the steps d_begin and d_begin + 1
  issue_x_slice(2 * d_begin - 1);
  issue_step(d_begin);
  if (d_begin + 1 < d_end) issue_step(d_begin + 1);
  dma_wait_all();
  lds_barrier();

  for (int d = d_begin; d < d_end; ++d) {
    const bool ahead = d + WT2X::LA < d_end;
    if (ahead) issue_step(d + WT2X::LA);      // lands during this step and the next
    const unsigned char *ys = sY + (d % WT2X::NYS) * WT2X::Y_STEP_B + cb * WT2::Y_SLICE_B + lane_off_y;
    int slice_off[3];
#pragma unroll
    for (int kd = 0; kd < 3; ++kd) slice_off[kd] = xslot(2 * d + kd - 1) * WT2::X_SLICE_B;
    int so_t[7];
#pragma unroll
    for (int i = 0; i < 7; ++i) so_t[i] = (tap_kd[i] == 0 ? slice_off[0] : (tap_kd[i] == 1 ? slice_off[1] : slice_off[2])) + tap_off[i];
#pragma unroll
    for (int oh = 0; oh < WT2::TH; ++oh) {
      const s16x4_t blo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_t *)(ys + oh * WT2::Y_ROW_B));
      const s16x4_t bhi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_t *)(ys + oh * WT2::Y_ROW_B + 4 * 64));
      const s16x8_t bv = {blo[0], blo[1], blo[2], blo[3], bhi[0], bhi[1], bhi[2], bhi[3]};
      const bf16x8_t bfr = __builtin_bit_cast(bf16x8_t, bv);
      bf16x8_t afr[7];
#pragma unroll
      for (int i = 0; i < 7; ++i) {
        const unsigned char *pa = sX + lane_off_x + so_t[i] + 2 * oh * WT2::X_ROW_B;
        const s16x4_t alo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_t *)pa);
        const s16x4_t ahi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_t *)(pa + 4 * 128));
        const s16x8_t av = {alo[0], alo[1], alo[2], alo[3], ahi[0], ahi[1], ahi[2], ahi[3]};
        afr[i] = __builtin_bit_cast(bf16x8_t, av);
      }
#pragma unroll
      for (int i = 0; i < 7; ++i) acc[i] = mfma32_tr<T16>(afr[i], bfr, acc[i]);
    }
    // the slices of step d + 1 were issued one step ago: everything but the five pieces issued above must have landed
    if (ahead) asm volatile("s_waitcnt vmcnt(5)" ::: "memory");
    else dma_wait_all();
    lds_barrier();
  }

  const int pair = cib * cobs + cog * 2 + cb;
  float *slab = slabs + ((int64_t)pair * gridDim.x + blockIdx.x) * (27 * 1024);
  const int co = lane & 31, hh = lane >> 5;
#pragma unroll
  for (int i = 0; i < 7; ++i) {
    const int tap = tg + 4 * i;
    if (tap < 27) {
#pragma unroll
      for (int q = 0; q < 16; ++q) slab[(tap * 32 + (q & 3) + 8 * (q >> 2) + 4 * hh) * 32 + co] = acc[i][q];
    }
  }
}

template <typename T16>
int s2_launch(const WgradLaunch &L, const WgradPlan &p, bool two_blocks) {
  static DynLdsOnce once, once_x;
  if (two_blocks) {
    DG_REQUIRE(ensure_dyn_lds(once_x, reinterpret_cast<const void *>(conv3_wgrad_tr_s2x_kernel<T16>), (int)WT2X::LDS_BYTES) ==
                   hipSuccess, DGTTA_ERR_LAUNCH, "wgrad_tr_s2x: cannot raise the dynamic LDS limit");
    hipLaunchKernelGGL(conv3_wgrad_tr_s2x_kernel<T16>, dim3((unsigned)p.units, (unsigned)(p.cibs * (p.cobs / 2))), dim3(512),
                       WT2X::LDS_BYTES, L.st, (const bf16_t *)L.x, L.xv, (const bf16_t *)L.dy, L.yv, (float *)L.ws, L.Cin, L.Cout, p.tW,
                       p.tH, p.nsd, p.DR, p.cobs);
  } else {
    DG_REQUIRE(ensure_dyn_lds(once, reinterpret_cast<const void *>(conv3_wgrad_tr_s2_kernel<T16>), (int)WT2::LDS_BYTES) ==
                   hipSuccess, DGTTA_ERR_LAUNCH, "wgrad_tr_s2: cannot raise the dynamic LDS limit");
    hipLaunchKernelGGL(conv3_wgrad_tr_s2_kernel<T16>, dim3((unsigned)p.units, (unsigned)(p.cibs * p.cobs)), dim3(256),
                       WT2::LDS_BYTES, L.st, (const bf16_t *)L.x, L.xv, (const bf16_t *)L.dy, L.yv, (float *)L.ws, L.Cin, L.Cout, p.tW,
                       p.tH, p.nsd, p.DR, p.cobs);
  }
  DG_CHECK_LAUNCH("conv3_wgrad_tr_s2_kernel");
  return DGTTA_OK;
}

}  // namespace

int conv3_wgrad_s2_launch(const WgradLaunch &L, const WgradPlan &p, bool two_blocks) {
  return L.dtype == DGTTA_F16 ? s2_launch<f16_t>(L, p, two_blocks) : s2_launch<bf16_t>(L, p, two_blocks);
}
