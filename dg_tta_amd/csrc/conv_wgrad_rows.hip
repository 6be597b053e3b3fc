// Weight gradient of the stride-1 3x3x3 convolutions on the matrix cores: the row kernels (the ring sweep that runs first on the
// large plain launches is conv_wgrad_ring.hip, the small planes are conv_wgrad_flat.hip).
#include "conv_wgrad_common.h"

namespace {

// =====================================================================================================================
// Weight gradient on the matrix cores (stride 1):  dW[tap][ci][co] = sum_v x[v + tap - 1][ci] * dy[v][co]
//   GEMM view: M = ci, N = co, K = voxels (runs of 32 along W).  A workgroup owns one 32(ci) x 32(co) channel tile and a
//   column of the volume: TH=4 output rows x 32 voxels, D range [d0,d1); its 4 waves own the four 16x16 sub-blocks and
//   keep all 27 tap accumulators (27 x f32x4) in registers while the column is swept slice by slice.
//   MFMA: bf16 v_mfma_f32_16x16x32_bf16 (K=32 = one voxel row per instruction), fp32 v_mfma_f32_16x16x4_f32 x8.
//   LDS: x and dy are staged TRANSPOSED (channel-major, 16-byte runs of consecutive voxels) with an in-register
//   EPV x EPV transpose, as a ring of 4 x-slices (halo of 1 in D and H) and 2 dy-slices; global loads for slice d+2 are
//   issued before the MFMAs of slice d and written to LDS after them.  The W shift of a tap (kw-1) is a funnel shift
//   of the aligned 16-byte run plus the next run's first dword(s).  Layout [row][run][channel][16 B] makes the 16
//   lanes of a k-group read consecutive 16-byte slots (no bank conflicts).
//   Each workgroup writes one fp32 partial slab; wgrad_reduce_kernel sums slabs in fixed order (deterministic).
// =====================================================================================================================
// x: view xv (input lattice of the virtual stride-1 problem), dy: view yv (output lattice; tiles run over it).
// mask bit t set = virtual tap t is accumulated.
template <typename T>
__global__ __launch_bounds__(256, (sizeof(T) == 2 ? 2 : 1)) void conv3_wgrad_mfma_kernel(const T *__restrict__ x, View xv, const T *__restrict__ dy,
                                                               View yv, float *__restrict__ slabs, int Cin, int Cout,
                                                               int tilesW, int tilesH, int nsd, int DR, int cobs,
                                                               WgradClasses wc) {
  const int cls = blockIdx.z;
  x += wc.xoff[cls];
  dy += wc.yoff[cls];
  const unsigned tapmask = wc.mask[cls];
  const int D = yv.D;
  typedef WG<T> C;
  constexpr int EPV = C::EPV;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  uint4 *sX = reinterpret_cast<uint4 *>(smem);                 // [4][XR][NCH_X][32]
  uint4 *sY = sX + 4 * C::XSLOT;                               // [2][TH][NCH_Y][32]
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int m = lane & 15, kg = lane >> 4;
  const int cih = wave >> 1, coh = wave & 1;

  int t = blockIdx.x;
  const int tw = t % tilesW;
  t /= tilesW;
  const int th = t % tilesH;
  t /= tilesH;
  const int ds = t % nsd;
  const int b = t / nsd;
  const int cib = blockIdx.y / cobs, cob = blockIdx.y % cobs;
  const int h0 = th * C::TH, w0 = tw * 32;
  const int d_begin = ds * DR, d_end = (d_begin + DR < D) ? d_begin + DR : D;
  const T *xb = x + b * xv.sb;
  const T *yb0 = dy + b * yv.sb;
  const int cin_lim = (Cin + EPV - 1) / EPV * EPV;

  uint4 stg[C::ROUNDS][EPV];

  // all loads of a slice are issued back to back: unconditional loads from a clamped address + select (a conditional
  // load makes hipcc branch and wait per element, which serialises the round trips)
  auto load_units = [&](int dx_slice, bool do_x, int dy_slice, bool do_y) {
#pragma unroll
    for (int rd = 0; rd < C::ROUNDS; ++rd) {
      const int u = tid + rd * 256;
      const bool is_x = u < C::NUX;
      const int v = is_x ? u : u - C::NUX;
      const int nch = is_x ? C::NCH_X : C::NCH_Y;
      const int cg = v % C::GC, ch = (v / C::GC) % nch, row = v / (C::GC * nch);
      const View &vw = is_x ? xv : yv;
      const T *bp = is_x ? xb : yb0;
      const int gd = is_x ? dx_slice : dy_slice, gh = is_x ? h0 - 1 + row : h0 + row;
      const int c = (is_x ? cib : cob) * 32 + cg * EPV;
      const bool rowok = u < C::NU && (is_x ? do_x : do_y) && (unsigned)gd < (unsigned)vw.D &&
                         (unsigned)gh < (unsigned)vw.H && c < (is_x ? cin_lim : Cout);
      const T *base = bp + (rowok ? gd * vw.sd + gh * vw.sh + c : 0);
      const int gw0 = w0 + EPV * ch - (is_x ? 1 : 0);
#pragma unroll
      for (int j = 0; j < EPV; ++j) {
        const int gw = gw0 + j;
        const bool ok = rowok && (unsigned)gw < (unsigned)vw.W;
        const uint4 val = *reinterpret_cast<const uint4 *>(base + (ok ? gw * vw.sw : 0));
        stg[rd][j] = ok ? val : make_uint4(0, 0, 0, 0);
      }
    }
  };
  auto store_units = [&](int xslot, bool do_x, int yslot, bool do_y) {
#pragma unroll
    for (int rd = 0; rd < C::ROUNDS; ++rd) {
      const int u = tid + rd * 256;
      uint4 o[EPV];
      if (u < C::NUX) {
        if (!do_x) continue;
        transpose_unit<T>(stg[rd], o);
        const int cg = u % C::GC, ch = (u / C::GC) % C::NCH_X, row = u / (C::GC * C::NCH_X);
        uint4 *dst = sX + xslot * C::XSLOT;
#pragma unroll
        for (int j = 0; j < EPV; ++j) dst[C::slot(row, ch, C::NCH_X, cg * EPV + j)] = o[j];
      } else if (u < C::NU) {
        if (!do_y) continue;
        transpose_unit<T>(stg[rd], o);
        const int v = u - C::NUX;
        const int cg = v % C::GC, ch = (v / C::GC) % C::NCH_Y, row = v / (C::GC * C::NCH_Y);
        uint4 *dst = sY + yslot * C::YSLOT;
#pragma unroll
        for (int j = 0; j < EPV; ++j) dst[C::slot(row, ch, C::NCH_Y, cg * EPV + j)] = o[j];
      }
    }
  };

  f32x4_t acc[27];
#pragma unroll
  for (int i = 0; i < 27; ++i) acc[i] = f32x4_t{0.f, 0.f, 0.f, 0.f};

  // prologue: x slices d_begin-1, d_begin, d_begin+1 and dy slice d_begin
  load_units(d_begin - 1, true, d_begin, true);
  store_units((d_begin - 1) & 3, true, d_begin & 1, true);
  load_units(d_begin, true, 0, false);
  store_units(d_begin & 3, true, 0, false);
  load_units(d_begin + 1, true, 0, false);
  store_units((d_begin + 1) & 3, true, 0, false);
  __syncthreads();

  for (int d = d_begin; d < d_end; ++d) {
    const bool more = d + 1 < d_end;
    load_units(d + 2, more, d + 1, more);     // in flight during the MFMAs below
    const uint4 *yb = sY + (d & 1) * C::YSLOT;
#pragma unroll
    for (int oh = 0; oh < C::TH; ++oh) {
#pragma unroll
      for (int stp = 0; stp < C::NSTEP; ++stp) {
        const int run = stp * 4 + kg;
        const uint4 bf = yb[C::slot(oh, run, C::NCH_Y, coh * 16 + m)];
#pragma unroll
        for (int kd = 0; kd < 3; ++kd) {
          const uint4 *xs = sX + ((d + kd - 1) & 3) * C::XSLOT;
#pragma unroll
          for (int kh = 0; kh < 3; ++kh) {
            if (((tapmask >> (kd * 9 + kh * 3)) & 7u) == 0) continue;      // wave-uniform: no tap of this (kd,kh) wanted
            const uint4 c0 = xs[C::slot(oh + kh, run, C::NCH_X, cih * 16 + m)];
            const uint2 ex = *reinterpret_cast<const uint2 *>(xs + C::slot(oh + kh, run + 1, C::NCH_X, cih * 16 + m));
#pragma unroll
            for (int kw = 0; kw < 3; ++kw)
              if ((tapmask >> (kd * 9 + kh * 3 + kw)) & 1u)
                mfma16<T>(shift_run<T>(c0, ex.x, ex.y, kw), bf, acc[kd * 9 + kh * 3 + kw]);
          }
        }
      }
    }
    store_units((d + 2) & 3, more, (d + 1) & 1, more);      // waits for the loads; transpose + LDS writes
    __syncthreads();
  }

  // partial slab [27][32 ci][32 co]; C/D map of the 16x16 MFMA: col = lane&15, row = (lane>>4)*4 + reg
  float *slab = slabs + (((int64_t)cls * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * (27 * 1024);
#pragma unroll
  for (int tap = 0; tap < 27; ++tap)
#pragma unroll
    for (int q = 0; q < 4; ++q) slab[(tap * 32 + cih * 16 + kg * 4 + q) * 32 + coh * 16 + m] = acc[tap][q];
}

// ---------------------------------------------------------------------------------------------------------------------
// bf16 weight gradient with hardware-transposed operand reads (stride 1, all 27 taps).  Same decomposition and slab
// format as conv3_wgrad_mfma_kernel, but:
//   * x / dy slices stay VOXEL-major in LDS ([row][voxel][32 channels = 64 B]) and are filled by LDS-DMA
//     (global_load_lds_dwordx4: 16 voxels x 64 B per instruction, no staging registers, no register transposes, no
//     ds_write); the K-contiguous MFMA operands (8 consecutive voxels of one channel per lane) come out of
//     ds_read_b64_tr_b16, so a tap's W shift is an address offset instead of a funnel shift per operand;
//   * MFMA 32x32x16: a wave owns the whole 32(ci) x 32(co) tile for 7 (or 6) of the 27 taps (tap = wave + 4 i), the dy
//     fragment of a (row, 16-voxel step) is shared by its taps; per MFMA: 2 transposed reads, ~1 VALU, no shifts.
// (The predecessor spent its issue slots on funnel shifts and 8x8 register transposes: measured 2.5x the MFMA time.)

// CLS: class launch (blockIdx.z selects operand offsets and a tap subset, as in conv3_wgrad_mfma_kernel): the set taps
// are dealt round-robin to the 4 waves, slots beyond a wave's share are skipped with wave-uniform branches.
template <bool CLS = false, typename T16 = bf16_t>
__global__ __launch_bounds__(256, 2) void conv3_wgrad_tr_kernel(const bf16_t *__restrict__ x, View xv,
                                                                const bf16_t *__restrict__ dy, View yv,
                                                                float *__restrict__ slabs, int Cin, int Cout, int tilesW,
                                                                int tilesH, int nsd, int DR, int cobs, WgradClasses wc, int upw,
                                                                int units, int xcd_map) {
  const int cls = CLS ? blockIdx.z : 0;
  if (CLS) {
    x += wc.xoff[cls];
    dy += wc.yoff[cls];
  }
  const int D = yv.D, H = yv.H, W = yv.W;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char *sX = smem;                                   // ring of 4 x slices
  unsigned char *sY = smem + 4 * WT::X_SLICE_B;               // ring of 2 dy slices
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);

  int tap_id[7], tap_kd[7], tap_off[7];
  int ntap_w = 7;
  // a workgroup sweeps `upw` consecutive units (columns of the volume) into the same accumulators: one slab per
  // workgroup, i.e. upw times fewer partial slabs to write and to reduce
  f32x16_t acc[7];
#pragma unroll
  for (int i = 0; i < 7; ++i)
#pragma unroll
    for (int q = 0; q < 16; ++q) acc[i][q] = 0.f;
  const int cib = blockIdx.y / cobs, cob = blockIdx.y % cobs;
  auto sweep = [&](int t) __attribute__((always_inline)) {
  const int tw = t % tilesW;
  t /= tilesW;
  const int th = t % tilesH;
  t /= tilesH;
  const int ds = t % nsd;
  const int b = t / nsd;
  const int h0 = th * WT::TH, w0 = tw * 32;
  const int d_begin = ds * DR, d_end = (d_begin + DR < D) ? d_begin + DR : D;
  const bf16_t *xb = x + b * xv.sb + cib * 32;
  const bf16_t *yb = dy + b * yv.sb + cob * 32;
  const int cin_lim = (Cin + 7) / 8 * 8;

  // DMA of one slice: piece idx (wave-uniform) -> x row r (3 pieces: voxels 0-15, 16-31, 32-33) or dy row (2 pieces);
  // lane l of a piece = voxel 16*pi + l/4, 16-byte channel chunk l%4
  const int l_vox = lane >> 2, l_chunk = lane & 3;
  constexpr int NPW = (WT::NP + 3) / 4;        // pieces per wave and slice
  auto issue_piece = [&](int i, int xd, int xslot, bool do_x, int yd, int yslot, bool do_y) __attribute__((always_inline)) {
    const int idx = wave + 4 * i;
    if (idx < WT::NPX) {
      if (!do_x) return;
      const int r = idx / 3, pi = idx % 3;
      if (pi == 2 && lane >= 8) return;
      const int gh = h0 - 1 + r, wx = 16 * pi + l_vox, gw = w0 - 1 + wx;
      const bool ok = (unsigned)xd < (unsigned)xv.D && (unsigned)gh < (unsigned)xv.H && (unsigned)gw < (unsigned)xv.W &&
                      cib * 32 + l_chunk * 8 < cin_lim;
      const void *src = ok ? (const void *)(xb + xd * xv.sd + gh * xv.sh + gw * xv.sw + l_chunk * 8) : (const void *)&g_zero16;
      dma16_to_lds(src, lds_addr_of(sX + xslot * WT::X_SLICE_B + r * WT::X_ROW_B + pi * 1024));
    } else if (idx < WT::NP) {
      if (!do_y) return;
      const int j = idx - WT::NPX, r = j / 2, pi = j % 2;
      const int gh = h0 + r, gw = w0 + 16 * pi + l_vox;
      const bool ok = (unsigned)yd < (unsigned)D && gh < H && gw < W && cob * 32 + l_chunk * 8 < Cout;
      const void *src = ok ? (const void *)(yb + yd * yv.sd + gh * yv.sh + gw * yv.sw + l_chunk * 8) : (const void *)&g_zero16;
      dma16_to_lds(src, lds_addr_of(sY + yslot * WT::Y_SLICE_B + r * WT::Y_ROW_B + pi * 1024));
    }
  };
  auto issue_slice = [&](int xd, int xslot, bool do_x, int yd, int yslot, bool do_y) __attribute__((always_inline)) {
#pragma unroll
    for (int i = 0; i < NPW; ++i) issue_piece(i, xd, xslot, do_x, yd, yslot, do_y);
  };

  // transposed-read lane address inside a 16-voxel x 32-channel block (64-byte voxel rows): group lane 4q+p supplies
  // voxel row q, channels 4p..4p+3 of the group's 16 channels; groups 0/1 = channels 0-15 / 16-31, lanes >= 32 = k 8..15
  const int lane_off = ((lane >> 5) * 8 + ((lane & 15) >> 2)) * 64 + ((lane >> 4) & 1) * 32 + (lane & 3) * 8;

  // this wave's taps: tap = wave + 4 i (i < 7) -- with classes, the (wave + 4 i)-th set bit of the class mask;
  // wave-uniform offsets of the x operand
  if (CLS) {
    const unsigned mask = wc.mask[cls];
    ntap_w = 0;
#pragma unroll
    for (int i = 0; i < 7; ++i) tap_id[i] = 26;
    int seen = 0;
    for (int tp = 0; tp < 27; ++tp)
      if ((mask >> tp) & 1u) {
        if ((seen & 3) == wave) {
#pragma unroll
          for (int i = 0; i < 7; ++i)
            if (i == (seen >> 2)) tap_id[i] = tp;
          ntap_w = (seen >> 2) + 1;
        }
        ++seen;
      }
  } else {
#pragma unroll
    for (int i = 0; i < 7; ++i) tap_id[i] = wave + 4 * i < 27 ? wave + 4 * i : 26;
  }
#pragma unroll
  for (int i = 0; i < 7; ++i) {
    const int tc = tap_id[i];
    tap_kd[i] = tc / 9;
    tap_off[i] = ((tc / 3) % 3) * WT::X_ROW_B + (tc % 3) * 64;
  }

  // prologue: x slices d_begin-1, d_begin, d_begin+1 and dy slice d_begin
  issue_slice(d_begin - 1, (d_begin - 1) & 3, true, d_begin, d_begin & 1, true);
  issue_slice(d_begin, d_begin & 3, true, 0, 0, false);
  issue_slice(d_begin + 1, (d_begin + 1) & 3, true, 0, 0, false);
  dma_wait_all();
  lds_barrier();

  for (int d = d_begin; d < d_end; ++d) {
    const bool more = d + 1 < d_end;
    const unsigned char *ys = sY + (d & 1) * WT::Y_SLICE_B + lane_off;
    int slice_off[3];
#pragma unroll
    for (int kd = 0; kd < 3; ++kd) slice_off[kd] = ((d + kd - 1) & 3) * WT::X_SLICE_B;
    // the tap's ring slot is selected once per slice (round 4: inside the unrolled row loop every operand read carried its own
    // compare / select chain - two transposed reads per MFMA made the sweep issue bound)
    int so_t[7];
#pragma unroll
    for (int i = 0; i < 7; ++i) so_t[i] = (tap_kd[i] == 0 ? slice_off[0] : (tap_kd[i] == 1 ? slice_off[1] : slice_off[2])) + tap_off[i];
#pragma unroll
    for (int oh = 0; oh < WT::TH; ++oh) {
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        const bf16x8_t bfr = tr_operand(ys + oh * WT::Y_ROW_B + ks * 1024);
        // one DMA piece of the next slices per (row, k-step): a burst at the top of the slice would block this wave
        // until the memory pipeline has taken all of them
        if (oh * 2 + ks < NPW) issue_piece(oh * 2 + ks, d + 2, (d + 2) & 3, more, d + 1, (d + 1) & 1, more);
        // all 7 operand reads first, then 7 MFMAs (wave 3's seventh slot repeats tap 26 into a discarded accumulator,
        // so the code is branch-free and the reads pipeline ahead of the matrix instructions)
        bf16x8_t afr[7];
#pragma unroll
        for (int i = 0; i < 7; ++i) {
          if (CLS && i >= ntap_w) continue;      // wave-uniform
          afr[i] = tr_operand(sX + lane_off + so_t[i] + oh * WT::X_ROW_B + ks * 1024);
        }
#pragma unroll
        for (int i = 0; i < 7; ++i) {
          if (CLS && i >= ntap_w) continue;
          acc[i] = mfma32_tr<T16>(afr[i], bfr, acc[i]);
        }
      }
    }
    dma_wait_all();
    lds_barrier();
  }
  };
  if (CLS) {                 // class launches: one unit per workgroup, the body specialised as before
    sweep((int)blockIdx.x);
  } else {
    for (int uu = 0; uu < upw; ++uu) {
      const int t = xcd_unit(xcd_map) * upw + uu;
      if (t >= units) break;
      sweep(t);
    }
  }

  // partial slab [27][32 ci][32 co]; C/D map of the 32x32 MFMA: col = lane&31 (co), row = (q&3) + 8(q>>2) + 4(lane>>5) (ci)
  float *slab = slabs + (((int64_t)cls * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x) * (27 * 1024);
  const int co = lane & 31, hh = lane >> 5;
#pragma unroll
  for (int i = 0; i < 7; ++i) {
    const int tap = tap_id[i];
    if (CLS ? i < ntap_w : wave + 4 * i < 27) {
#pragma unroll
      for (int q = 0; q < 16; ++q) slab[(tap * 32 + (q & 3) + 8 * (q >> 2) + 4 * hh) * 32 + co] = acc[i][q];
    }
  }
}

// ---------------------------------------------------------------------------------------------------------------------
// 8-wave variant of conv3_wgrad_tr_kernel for Cout >= 64: a workgroup owns a 32(ci) x 64(co) channel tile, so the x tile
// (the larger one, with its halo) is staged once for two output-channel blocks: 58 instead of 94 DMA bytes per MFMA
// (the 4-wave kernel sits on the ~11 B/clk/CU fill rate).  Wave w owns taps w, w+8, w+16, w+24 (27 of the 32 slots are
// real) for both blocks: an x fragment feeds 2 MFMAs, 1.5 transposed reads per MFMA instead of 2.3.
struct WT8 {
  static constexpr int Y_ROW_B = 32 * 128, Y_SLICE_B = WT::TH * Y_ROW_B;       // dy rows of 64 channels
  static constexpr int LDS_BYTES = 4 * WT::X_SLICE_B + 2 * Y_SLICE_B;
  static constexpr int NPY = WT::TH * 4;                                        // 8 voxels x 128 B per piece
  static constexpr int NP = WT::NPX + NPY;
};

template <typename T16 = bf16_t>
__global__ __launch_bounds__(512, 1) void conv3_wgrad_tr8_kernel(const bf16_t *__restrict__ x, View xv,
                                                                 const bf16_t *__restrict__ dy, View yv,
                                                                 float *__restrict__ slabs, int Cin, int Cout, int tilesW,
                                                                 int tilesH, int nsd, int DR, int cobs, int upw, int units, int xcd_map) {
  const int D = yv.D, H = yv.H, W = yv.W;
  extern __shared__ __attribute__((aligned(16))) unsigned char smem[];
  unsigned char *sX = smem;
  unsigned char *sY = smem + 4 * WT::X_SLICE_B;
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  // a workgroup sweeps `upw` consecutive units (columns of the volume) into the same accumulators: one slab per
  // workgroup, i.e. upw times fewer partial slabs to write and to reduce
  f32x16_t acc[4][2];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int c = 0; c < 2; ++c)
#pragma unroll
      for (int q = 0; q < 16; ++q) acc[i][c][q] = 0.f;
  const int cobs2 = (cobs + 1) / 2;
  const int cib = blockIdx.y / cobs2, cob2 = blockIdx.y % cobs2;          // channel-block pair (2 cob2, 2 cob2 + 1)
  for (int uu = 0; uu < upw; ++uu) {
  int t = xcd_unit(xcd_map) * upw + uu;
  if (t >= units) break;
  const int tw = t % tilesW;
  t /= tilesW;
  const int th = t % tilesH;
  t /= tilesH;
  const int ds = t % nsd;
  const int b = t / nsd;
  const int h0 = th * WT::TH, w0 = tw * 32;
  const int d_begin = ds * DR, d_end = (d_begin + DR < D) ? d_begin + DR : D;
  const bf16_t *xb = x + b * xv.sb + cib * 32;
  const bf16_t *yb = dy + b * yv.sb + cob2 * 64;
  const int cin_lim = (Cin + 7) / 8 * 8;

  constexpr int NPW = (WT8::NP + 7) / 8;
  auto issue_piece = [&](int i, int xd, int xslot, int yd, int yslot, bool more, bool with_y = true) __attribute__((always_inline)) {
    const int idx = wave + 8 * i;
    if (!more) return;
    if (idx < WT::NPX) {
      const int r = idx / 3, pi = idx % 3;
      if (pi == 2 && lane >= 8) return;
      const int l_vox = lane >> 2, l_chunk = lane & 3;
      const int gh = h0 - 1 + r, gw = w0 - 1 + 16 * pi + l_vox;
      const bool ok = (unsigned)xd < (unsigned)xv.D && (unsigned)gh < (unsigned)xv.H && (unsigned)gw < (unsigned)xv.W &&
                      cib * 32 + l_chunk * 8 < cin_lim;
      const void *src = ok ? (const void *)(xb + xd * xv.sd + gh * xv.sh + gw * xv.sw + l_chunk * 8) : (const void *)&g_zero16;
      dma16_to_lds(src, lds_addr_of(sX + xslot * WT::X_SLICE_B + r * WT::X_ROW_B + pi * 1024));
    } else if (idx < WT8::NP && with_y) {
      const int j = idx - WT::NPX, r = j / 4, pi = j % 4;
      const int l_vox = lane >> 3, l_chunk = lane & 7;       // 8 voxels x 8 chunks of 16 B
      const int gh = h0 + r, gw = w0 + 8 * pi + l_vox;
      const bool ok = (unsigned)yd < (unsigned)D && gh < H && gw < W && cob2 * 64 + l_chunk * 8 < Cout;
      const void *src = ok ? (const void *)(yb + yd * yv.sd + gh * yv.sh + gw * yv.sw + l_chunk * 8) : (const void *)&g_zero16;
      dma16_to_lds(src, lds_addr_of(sY + yslot * WT8::Y_SLICE_B + r * WT8::Y_ROW_B + pi * 1024));
    }
  };

  const int kq = (lane >> 5) * 8 + ((lane & 15) >> 2), cpart = ((lane >> 4) & 1) * 32 + (lane & 3) * 8;
  const int lane_off_x = kq * 64 + cpart, lane_off_y = kq * 128 + cpart;

  int tap_kd[4], tap_off[4];
#pragma unroll
  for (int i = 0; i < 4; ++i) {
    const int tc = wave + 8 * i < 27 ? wave + 8 * i : 26;
    tap_kd[i] = tc / 9;
    tap_off[i] = ((tc / 3) % 3) * WT::X_ROW_B + (tc % 3) * 64;
  }
  // prologue: x slices d_begin-1, d_begin, d_begin+1 and dy slice d_begin
#pragma unroll
  for (int i = 0; i < NPW; ++i) issue_piece(i, d_begin - 1, (d_begin - 1) & 3, d_begin, d_begin & 1, true);
#pragma unroll
  for (int sl = 0; sl <= 1; ++sl)
#pragma unroll
    for (int i = 0; i < (WT::NPX + 7) / 8; ++i) issue_piece(i, d_begin + sl, (d_begin + sl) & 3, 0, 0, true, false);
  dma_wait_all();
  lds_barrier();
  for (int d = d_begin; d < d_end; ++d) {
    const bool more = d + 1 < d_end;
    const unsigned char *ys = sY + (d & 1) * WT8::Y_SLICE_B + lane_off_y;
    int slice_off[3];
#pragma unroll
    for (int kd = 0; kd < 3; ++kd) slice_off[kd] = ((d + kd - 1) & 3) * WT::X_SLICE_B;
    int so_t[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) so_t[i] = (tap_kd[i] == 0 ? slice_off[0] : (tap_kd[i] == 1 ? slice_off[1] : slice_off[2])) + tap_off[i];
#pragma unroll
    for (int oh = 0; oh < WT::TH; ++oh) {
#pragma unroll
      for (int ks = 0; ks < 2; ++ks) {
        if (oh * 2 + ks < NPW) issue_piece(oh * 2 + ks, d + 2, (d + 2) & 3, d + 1, (d + 1) & 1, more);
        bf16x8_t bfr[2];
#pragma unroll
        for (int c = 0; c < 2; ++c) {
          const unsigned char *pb = ys + oh * WT8::Y_ROW_B + ks * 16 * 128 + c * 64;
          const s16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_t *)pb);
          const s16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_t *)(pb + 4 * 128));
          const s16x8_t v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
          bfr[c] = __builtin_bit_cast(bf16x8_t, v);
        }
        bf16x8_t afr[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          afr[i] = tr_operand(sX + lane_off_x + so_t[i] + oh * WT::X_ROW_B + ks * 1024);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int c = 0; c < 2; ++c) acc[i][c] = mfma32_tr<T16>(afr[i], bfr[c], acc[i][c]);
      }
    }
    dma_wait_all();
    lds_barrier();
  }
  }   // units
  const int co = lane & 31, hh = lane >> 5;
#pragma unroll
  for (int c = 0; c < 2; ++c) {
    const int cob = 2 * cob2 + c;
    if (cob >= cobs) continue;
    float *slab = slabs + (((int64_t)cib * cobs + cob) * gridDim.x + blockIdx.x) * (27 * 1024);
#pragma unroll
    for (int i = 0; i < 4; ++i) {
      const int tap = wave + 8 * i;
      if (tap < 27) {
#pragma unroll
        for (int q = 0; q < 16; ++q) slab[(tap * 32 + (q & 3) + 8 * (q >> 2) + 4 * hh) * 32 + co] = acc[i][c][q];
      }
    }
  }
}

template <typename T>
int mfma_launch(const WgradLaunch &L, const WgradPlan &p, const WgradClasses &wc) {
  auto kern = conv3_wgrad_mfma_kernel<T>;
  static DynLdsOnce mf_once;
  DG_REQUIRE(ensure_dyn_lds(mf_once, reinterpret_cast<const void *>(kern), (int)WG<T>::LDS_BYTES) == hipSuccess,
             DGTTA_ERR_LAUNCH, "wgrad_mfma: cannot raise the dynamic LDS limit");
  hipLaunchKernelGGL(kern, dim3((unsigned)p.units, (unsigned)(p.cibs * p.cobs), (unsigned)wc.n), dim3(256), WG<T>::LDS_BYTES,
                     L.st, (const T *)L.x, L.xv, (const T *)L.dy, L.yv, (float *)L.ws, L.Cin, L.Cout, p.tW, p.tH, p.nsd, p.DR, p.cobs, wc);
  DG_CHECK_LAUNCH("conv3_wgrad_mfma_kernel");
  return DGTTA_OK;
}

template <typename T16>
int tr_launch(const WgradLaunch &L, const WgradPlan &p, const WgradClasses &wc, bool plain, int upw, int64_t nslab) {
  auto ktr = plain ? conv3_wgrad_tr_kernel<false, T16> : conv3_wgrad_tr_kernel<true, T16>;
  static DynLdsOnce tr_once[2];
  DG_REQUIRE(ensure_dyn_lds(tr_once[plain], reinterpret_cast<const void *>(ktr), (int)WT::LDS_BYTES) == hipSuccess,
             DGTTA_ERR_LAUNCH, "wgrad_tr: cannot raise the dynamic LDS limit");
  hipLaunchKernelGGL(ktr, dim3((unsigned)nslab, (unsigned)(p.cibs * p.cobs), (unsigned)wc.n), dim3(256), WT::LDS_BYTES,
                     L.st, (const bf16_t *)L.x, L.xv, (const bf16_t *)L.dy, L.yv, (float *)L.ws, L.Cin, L.Cout, p.tW, p.tH, p.nsd,
                     p.DR, p.cobs, wc, upw, (int)p.units, dgtta_switches().wgrad_xcd != '0');
  DG_CHECK_LAUNCH("conv3_wgrad_tr_kernel");
  return DGTTA_OK;
}

template <typename T16>
int tr8_launch(const WgradLaunch &L, const WgradPlan &p, int upw, int64_t nslab) {
  static DynLdsOnce a8;
  DG_REQUIRE(ensure_dyn_lds(a8, reinterpret_cast<const void *>(conv3_wgrad_tr8_kernel<T16>), (int)WT8::LDS_BYTES) ==
                 hipSuccess, DGTTA_ERR_LAUNCH, "wgrad_tr8: cannot raise the dynamic LDS limit");
  const int64_t gy = (int64_t)p.cibs * ((p.cobs + 1) / 2);
  hipLaunchKernelGGL(conv3_wgrad_tr8_kernel<T16>, dim3((unsigned)nslab, (unsigned)gy), dim3(512),
                     WT8::LDS_BYTES, L.st, (const bf16_t *)L.x, L.xv, (const bf16_t *)L.dy, L.yv, (float *)L.ws, L.Cin, L.Cout, p.tW, p.tH,
                     p.nsd, p.DR, p.cobs, upw, (int)p.units, dgtta_switches().wgrad_xcd != '0');
  DG_CHECK_LAUNCH("conv3_wgrad_tr8_kernel");
  return DGTTA_OK;
}

}  // namespace

int conv3_wgrad_mfma_launch(const WgradLaunch &L, const WgradPlan &p, const WgradClasses &wc) {
  if (L.dtype == DGTTA_F32) return mfma_launch<float>(L, p, wc);
  return L.dtype == DGTTA_F16 ? mfma_launch<f16_t>(L, p, wc) : mfma_launch<bf16_t>(L, p, wc);
}

int conv3_wgrad_tr_launch(const WgradLaunch &L, const WgradPlan &p, const WgradClasses &wc, bool plain, int upw, int64_t nslab) {
  return L.dtype == DGTTA_F16 ? tr_launch<f16_t>(L, p, wc, plain, upw, nslab) : tr_launch<bf16_t>(L, p, wc, plain, upw, nslab);
}

int conv3_wgrad_tr8_launch(const WgradLaunch &L, const WgradPlan &p, int upw, int64_t nslab) {
  return L.dtype == DGTTA_F16 ? tr8_launch<f16_t>(L, p, upw, nslab) : tr8_launch<bf16_t>(L, p, upw, nslab);
}
