// Matrix-core kernels of the 1x1x1 heads with MORE than 32 input channels: the auxiliary (deep supervision) heads of the decoder
// stages below full resolution - Cin in {64, 128, 256} (320 in anisotropic plans), all 105 classes - are skinny GEMMs
//   forward   out[rows][nsel]  = x[rows][Cin] . W_sel^T + b        (K = Cin)
//   dgrad     dx[rows][Cin]  (+)= dout[rows][nsel] . W_sel          (K = nsel, zero padded to 16)
//   wgrad     dW_sel[nsel][Cin] = dout^T . x                        (K = rows)
// on v_mfma_f32_32x32x16_{bf16,f16}, 16-bit storage only.  A workgroup (4 waves) keeps its weight operand in LDS for its whole
// life and moves 64-row tiles through LDS with coalesced 16-byte accesses; a wave owns a 32-row half of the tile and every
// other 32-column block of the result.  LDS rows carry 8 pad elements, meant to spread the 16-byte operand reads of 32 lanes
// (pitch 2 K + 16 bytes) over the banks (bank conflicts were not counted).  The class dimension is padded to 32 INSIDE the
// kernels (zero weight rows, masked stores).  Per row a head moves 420 B of logits against 2 Cin B of activations, so the
// forward spends a second MFMA per step on the low term of a TWO-TERM 16-bit split of the fp32 weights (w ~ hi + lo; not
// exact: the residual is about 2^-17 |w| for bf16, and for fp16 lo underflows for small weights and hi overflows above
// 65504): the logits are much closer to those of the VALU head kernels (fp32 weights) than weights rounded to 16 bits give.
// The tile loop is single-buffered (load, barrier, MFMA, barrier) and the forward holds 87-126 KB of LDS from Cin = 128 on,
// i.e. one workgroup per CU.  Measured against the general kernels: profiles/deep_supervision_heads.txt (made by
// profiles/tools/dsheadbench.py), quoted in DESIGN.md.
// Deterministic: fixed summation order per output, the weight gradient's splits are added in order by reduce_splits.
#include "conv_common.h"

namespace {

constexpr int HM_ROWS = 64;      // rows of a tile
constexpr int HM_PAD = 8;        // pad elements of an LDS row (16 bytes)
constexpr int HM_WP = HM_ROWS + HM_PAD;      // pitch of the transposed tiles of the weight gradient

__device__ __forceinline__ f32x16_t zero_acc() {
  f32x16_t a;
#pragma unroll
  for (int q = 0; q < 16; ++q) a[q] = 0.f;
  return a;
}

// ---------------------------------------------------------------------------------------------------------------- forward
// grid (tiles, class chunks of CC); LDS: W hi [CC][Cin + 8], W lo [CC][Cin + 8], x tile [64][Cin + 8] (16 bit), bias [CC]
template <typename T16>
__global__ __launch_bounds__(256) void head_fwd_mfma_kernel(const unsigned short *__restrict__ x, int ldx, const float *__restrict__ w,
                                                            const float *__restrict__ bias, const int *__restrict__ sel, int nsel,
                                                            float *__restrict__ out, int ldo, int Cin, int64_t rows, int CC) {
  extern __shared__ uint4 hm_smem[];
  const int P = Cin + HM_PAD;
  unsigned short *swh = reinterpret_cast<unsigned short *>(hm_smem);
  unsigned short *swl = swh + CC * P;
  unsigned short *sx = swl + CC * P;
  float *sb = reinterpret_cast<float *>(sx + HM_ROWS * P);
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
  const int c0 = blockIdx.y * CC;
  const int nc = nsel - c0 < CC ? nsel - c0 : CC;
  for (int i = tid; i < CC * Cin; i += 256) {
    const int k = i / Cin, ci = i - k * Cin;
    const float v = k < nc ? w[(int64_t)(sel ? sel[c0 + k] : c0 + k) * Cin + ci] : 0.f;
    const unsigned short hi = f32_to_16<T16>(v);
    swh[k * P + ci] = hi;
    swl[k * P + ci] = f32_to_16<T16>(v - from16<T16>(hi));
  }
  for (int i = tid; i < CC; i += 256) sb[i] = i < nc ? bias[sel ? sel[c0 + i] : c0 + i] : 0.f;
  const int n16 = Cin >> 3;      // 16-byte groups of a row
  const int64_t ntile = (rows + HM_ROWS - 1) / HM_ROWS;
  for (int64_t t = blockIdx.x; t < ntile; t += gridDim.x) {
    const int64_t r0 = t * HM_ROWS;
    const int nr = rows - r0 < HM_ROWS ? (int)(rows - r0) : HM_ROWS;
    __syncthreads();      // the previous tile is consumed (first tile: the weights are published)
#pragma unroll 2
    for (int i = tid; i < HM_ROWS * n16; i += 256) {
      const int v = i / n16, c = i - v * n16;
      uint4 val = make_uint4(0u, 0u, 0u, 0u);
      if (v < nr) val = *reinterpret_cast<const uint4 *>(x + (r0 + v) * ldx + c * 8);
      *reinterpret_cast<uint4 *>(sx + v * P + c * 8) = val;
    }
    __syncthreads();
    const int rb = wave & 1;
    const unsigned short *ap = sx + (rb * 32 + r) * P + 8 * h;
    for (int cb = wave >> 1; cb * 32 < nc; cb += 2) {
      const unsigned short *bh = swh + (cb * 32 + r) * P + 8 * h, *bl = swl + (cb * 32 + r) * P + 8 * h;
      f32x16_t acc = zero_acc();
      for (int ks = 0; ks < Cin; ks += 16) {
        const uint4 a = *reinterpret_cast<const uint4 *>(ap + ks);
        mfma_step<T16>(a, *reinterpret_cast<const uint4 *>(bl + ks), acc);
        mfma_step<T16>(a, *reinterpret_cast<const uint4 *>(bh + ks), acc);
      }
      const int cls = cb * 32 + r;
      if (cls < nc) {
        const float bv = sb[cls];
#pragma unroll
        for (int q = 0; q < 16; ++q) {
          const int row = rb * 32 + (q & 3) + 8 * (q >> 2) + 4 * h;
          if (row < nr) out[(r0 + row) * ldo + c0 + cls] = acc[q] + bv;
        }
      }
    }
  }
}

// ---------------------------------------------------------------------------------------------------------- data gradient
// grid (tiles, chunks of CB 32-channel blocks); LDS: W^T [CB * 32][KP + 8], dout tile [64][KP + 8] (16 bit), KP = nsel padded to 16
template <typename T16, bool ACC>
__global__ __launch_bounds__(256) void head_dgrad_mfma_kernel(const float *__restrict__ dout, int lddo, const float *__restrict__ w,
                                                              const int *__restrict__ sel, int nsel, unsigned short *__restrict__ dx,
                                                              int lddx, int Cin, int64_t rows, int CB) {
  extern __shared__ uint4 hm_smem[];
  const int KP = (nsel + 15) & ~15, P = KP + HM_PAD;
  unsigned short *swt = reinterpret_cast<unsigned short *>(hm_smem);
  unsigned short *sd = swt + CB * 32 * P;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
  const int ci0 = blockIdx.y * CB * 32;
  const int nci = Cin - ci0 < CB * 32 ? Cin - ci0 : CB * 32;
  for (int i = tid; i < nci * KP; i += 256) {
    const int k = i / nci, c = i - k * nci;
    const float v = k < nsel ? w[(int64_t)(sel ? sel[k] : k) * Cin + ci0 + c] : 0.f;
    swt[c * P + k] = f32_to_16<T16>(v);
  }
  const int64_t ntile = (rows + HM_ROWS - 1) / HM_ROWS;
  for (int64_t t = blockIdx.x; t < ntile; t += gridDim.x) {
    const int64_t r0 = t * HM_ROWS;
    const int nr = rows - r0 < HM_ROWS ? (int)(rows - r0) : HM_ROWS;
    __syncthreads();
    // fp32 gradient rows -> 16 bit, zero beyond the last row and class: eight loads in flight per thread
    for (int e0 = tid; e0 < HM_ROWS * KP; e0 += 256 * 8) {
      float tmp[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int e = e0 + 256 * u, v = e / KP, k = e - v * KP;
        tmp[u] = (v < nr && k < nsel) ? dout[(r0 + v) * lddo + k] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int e = e0 + 256 * u, v = e / KP, k = e - v * KP;
        if (v < HM_ROWS) sd[v * P + k] = f32_to_16<T16>(tmp[u]);
      }
    }
    __syncthreads();
    const int rb = wave & 1;
    const unsigned short *ap = sd + (rb * 32 + r) * P + 8 * h;
    for (int cb = wave >> 1; cb * 32 < nci; cb += 2) {
      const unsigned short *bp = swt + (cb * 32 + r) * P + 8 * h;
      f32x16_t acc = zero_acc();
      for (int ks = 0; ks < KP; ks += 16)
        mfma_step<T16>(*reinterpret_cast<const uint4 *>(ap + ks), *reinterpret_cast<const uint4 *>(bp + ks), acc);
      const int ci = ci0 + cb * 32 + r;
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int row = rb * 32 + (q & 3) + 8 * (q >> 2) + 4 * h;
        if (row < nr) {
          unsigned short *o = dx + (r0 + row) * lddx + ci;
          float v = acc[q];
          if (ACC) v += from16<T16>(*o);
          *o = f32_to_16<T16>(v);
        }
      }
    }
  }
}

// -------------------------------------------------------------------------------------------------------- weight gradient
// part[split][k][ci] = sum over the split's rows of dout[row][k] x[row][ci].  grid (splits, chunks of CB <= 4 channel blocks); both
// operands are summed over ROWS, so the tiles sit transposed in LDS - dout^T [128][64 + 8], x^T [CB * 32][64 + 8] - written as
// dwords of two consecutive rows.  Wave kb owns classes 32 kb .. 32 kb + 31 and all CB channel blocks.
template <typename T16>
__global__ __launch_bounds__(256) void head_wgrad_rows_kernel(const unsigned short *__restrict__ x, int ldx, const float *__restrict__ dout,
                                                              int lddo, float *__restrict__ part, int nsel, int Cin, int64_t rows, int CB) {
  __shared__ __attribute__((aligned(16))) unsigned short sdt[128 * HM_WP];
  __shared__ __attribute__((aligned(16))) unsigned short sxt[128 * HM_WP];
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
  const int ci0 = blockIdx.y * CB * 32;
  const int ncb = (Cin - ci0) / 32 < CB ? (Cin - ci0) / 32 : CB;
  for (int i = tid; i < 128 * HM_WP / 2; i += 256) {      // class rows >= nsel and channel rows >= 32 ncb stay zero
    reinterpret_cast<unsigned *>(sdt)[i] = 0u;
    reinterpret_cast<unsigned *>(sxt)[i] = 0u;
  }
  f32x16_t acc[4];
#pragma unroll
  for (int j = 0; j < 4; ++j) acc[j] = zero_acc();
  const int64_t ntile = (rows + HM_ROWS - 1) / HM_ROWS;
  const int64_t per = (ntile + gridDim.x - 1) / gridDim.x;
  const int64_t t0 = (int64_t)blockIdx.x * per, t1 = t0 + per < ntile ? t0 + per : ntile;
  const int n16 = ncb * 4;
  for (int64_t t = t0; t < t1; ++t) {
    const int64_t r0 = t * HM_ROWS;
    const int nv = rows - r0 < HM_ROWS ? (int)(rows - r0) : HM_ROWS;
    __syncthreads();
    for (int e0 = tid; e0 < 32 * nsel; e0 += 256 * 4) {      // (row pair, class): lanes along the classes
      float ta[4], tb[4];
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int e = e0 + 256 * u, vp = e / nsel, k = e - vp * nsel;
        ta[u] = (vp < 32 && 2 * vp < nv) ? dout[(r0 + 2 * vp) * lddo + k] : 0.f;
        tb[u] = (vp < 32 && 2 * vp + 1 < nv) ? dout[(r0 + 2 * vp + 1) * lddo + k] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < 4; ++u) {
        const int e = e0 + 256 * u, vp = e / nsel, k = e - vp * nsel;
        if (vp < 32) reinterpret_cast<unsigned *>(sdt)[(k * HM_WP) / 2 + vp] = pack2_16<T16>(ta[u], tb[u]);
      }
    }
    for (int i = tid; i < 32 * n16; i += 256) {               // (row pair, 8 channels): lanes along the channels
      const int vp = i / n16, c8 = i - vp * n16;
      uint4 u0 = make_uint4(0u, 0u, 0u, 0u), u1 = u0;
      if (2 * vp < nv) u0 = *reinterpret_cast<const uint4 *>(x + (r0 + 2 * vp) * ldx + ci0 + c8 * 8);
      if (2 * vp + 1 < nv) u1 = *reinterpret_cast<const uint4 *>(x + (r0 + 2 * vp + 1) * ldx + ci0 + c8 * 8);
      const unsigned a[4] = {u0.x, u0.y, u0.z, u0.w}, b[4] = {u1.x, u1.y, u1.z, u1.w};
      unsigned *o = reinterpret_cast<unsigned *>(sxt) + (c8 * 8 * HM_WP) / 2 + vp;
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        o[(2 * j) * (HM_WP / 2)] = (a[j] & 0xffffu) | (b[j] << 16);
        o[(2 * j + 1) * (HM_WP / 2)] = (a[j] >> 16) | (b[j] & 0xffff0000u);
      }
    }
    __syncthreads();
    if (wave * 32 < nsel) {
      const unsigned short *ap = sdt + (wave * 32 + r) * HM_WP + 8 * h;
#pragma unroll
      for (int ks = 0; ks < HM_ROWS; ks += 16) {
        const uint4 a = *reinterpret_cast<const uint4 *>(ap + ks);
#pragma unroll
        for (int j = 0; j < 4; ++j)
          if (j < ncb) mfma_step<T16>(a, *reinterpret_cast<const uint4 *>(sxt + (j * 32 + r) * HM_WP + 8 * h + ks), acc[j]);
      }
    }
  }
#pragma unroll
  for (int j = 0; j < 4; ++j)
    if (j < ncb) {
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int k = wave * 32 + (q & 3) + 8 * (q >> 2) + 4 * h;
        if (k < nsel) part[((int64_t)blockIdx.x * nsel + k) * Cin + ci0 + j * 32 + r] = acc[j][q];
      }
    }
}

constexpr size_t HM_LDS_MAX = 144 * 1024;      // of the 160 KiB of a CU

bool hm_shape_ok(int Cin, int nsel, int dtype) {
  return (dtype == DGTTA_BF16 || dtype == DGTTA_F16) && Cin >= 32 && Cin <= 320 && Cin % 32 == 0 && nsel >= 1 && nsel <= 128;
}
unsigned hm_tile_grid(int64_t rows, int64_t cap) {
  const int64_t nt = (rows + HM_ROWS - 1) / HM_ROWS;
  return (unsigned)(nt < cap ? nt : cap);
}

}  // namespace

int head_fwd_mfma(const void *x, int ldx, const float *w, const float *bias, const int *sel, int nsel, float *out, int ldo, int Cin,
                  int64_t rows, int dtype, hipStream_t st) {
  if (!hm_shape_ok(Cin, nsel, dtype) || ldx % 8 || ((uintptr_t)x & 15)) return DGTTA_ERR_UNSUPPORTED;
  // all classes in one workgroup where hi + lo of the weights fit beside the tile, else chunks of 64 classes (x is read per chunk)
  const int P = Cin + HM_PAD, NP = (nsel + 31) & ~31;
  auto lds_of = [&](int cc) { return (size_t)(2 * cc + HM_ROWS) * P * 2 + (size_t)cc * 4; };
  const int CC = lds_of(NP) <= 96 * 1024 ? NP : (NP < 64 ? NP : 64);
  const size_t lds = lds_of(CC);
  if (lds > HM_LDS_MAX) return DGTTA_ERR_UNSUPPORTED;
  const dim3 grid(hm_tile_grid(rows, 1024), (unsigned)((nsel + CC - 1) / CC));
  static DynLdsOnce once_b, once_h;
  if (dtype == DGTTA_BF16) {
    DG_REQUIRE(ensure_dyn_lds(once_b, reinterpret_cast<const void *>(head_fwd_mfma_kernel<bf16_t>), (int)HM_LDS_MAX) == hipSuccess,
               DGTTA_ERR_LAUNCH, "head_fwd_mfma: cannot raise the dynamic LDS limit");
    hipLaunchKernelGGL(head_fwd_mfma_kernel<bf16_t>, grid, dim3(256), lds, st, (const unsigned short *)x, ldx, w, bias, sel, nsel, out,
                       ldo, Cin, rows, CC);
  } else {
    DG_REQUIRE(ensure_dyn_lds(once_h, reinterpret_cast<const void *>(head_fwd_mfma_kernel<f16_t>), (int)HM_LDS_MAX) == hipSuccess,
               DGTTA_ERR_LAUNCH, "head_fwd_mfma: cannot raise the dynamic LDS limit");
    hipLaunchKernelGGL(head_fwd_mfma_kernel<f16_t>, grid, dim3(256), lds, st, (const unsigned short *)x, ldx, w, bias, sel, nsel, out,
                       ldo, Cin, rows, CC);
  }
  DG_CHECK_LAUNCH("head_fwd_mfma_kernel");
  return DGTTA_OK;
}

int head_dgrad_mfma(const float *dout, int lddo, const float *w, const int *sel, int nsel, void *dx, int lddx, int Cin, int64_t rows,
                    int accumulate_dx, int dtype, hipStream_t st) {
  if (!hm_shape_ok(Cin, nsel, dtype)) return DGTTA_ERR_UNSUPPORTED;
  const int P = ((nsel + 15) & ~15) + HM_PAD, nblk = Cin / 32;
  const int nchunk = (nblk + 7) / 8, CB = (nblk + nchunk - 1) / nchunk;      // at most 256 channels of W^T per workgroup
  const size_t lds = (size_t)(CB * 32 + HM_ROWS) * P * 2;
  const dim3 grid(hm_tile_grid(rows, 1024), (unsigned)((nblk + CB - 1) / CB));
#define HM_DGRAD(T16, ACC)                                                                                                           \
  do {                                                                                                                               \
    static DynLdsOnce once;                                                                                                          \
    DG_REQUIRE(ensure_dyn_lds(once, reinterpret_cast<const void *>(head_dgrad_mfma_kernel<T16, ACC>), (int)HM_LDS_MAX) == hipSuccess, \
               DGTTA_ERR_LAUNCH, "head_dgrad_mfma: cannot raise the dynamic LDS limit");                                             \
    hipLaunchKernelGGL((head_dgrad_mfma_kernel<T16, ACC>), grid, dim3(256), lds, st, dout, lddo, w, sel, nsel, (unsigned short *)dx,  \
                       lddx, Cin, rows, CB);                                                                                         \
  } while (0)
  if (dtype == DGTTA_BF16) {
    if (accumulate_dx) HM_DGRAD(bf16_t, true);
    else HM_DGRAD(bf16_t, false);
  } else {
    if (accumulate_dx) HM_DGRAD(f16_t, true);
    else HM_DGRAD(f16_t, false);
  }
#undef HM_DGRAD
  DG_CHECK_LAUNCH("head_dgrad_mfma_kernel");
  return DGTTA_OK;
}

// part: nsplit * nsel * Cin floats; the caller adds the splits in order (reduce_splits)
int head_wgrad_rows_mfma(const void *x, int ldx, const float *dout, int lddo, float *part, int nsplit, int nsel, int Cin, int64_t rows,
                         int dtype, hipStream_t st) {
  if (!hm_shape_ok(Cin, nsel, dtype) || ldx % 8 || ((uintptr_t)x & 15)) return DGTTA_ERR_UNSUPPORTED;
  const int nblk = Cin / 32, CB = nblk < 4 ? nblk : 4;
  const dim3 grid((unsigned)nsplit, (unsigned)((nblk + CB - 1) / CB));
  if (dtype == DGTTA_BF16)
    hipLaunchKernelGGL(head_wgrad_rows_kernel<bf16_t>, grid, dim3(256), 0, st, (const unsigned short *)x, ldx, dout, lddo, part, nsel, Cin,
                       rows, CB);
  else
    hipLaunchKernelGGL(head_wgrad_rows_kernel<f16_t>, grid, dim3(256), 0, st, (const unsigned short *)x, ldx, dout, lddo, part, nsel, Cin,
                       rows, CB);
  DG_CHECK_LAUNCH("head_wgrad_rows_kernel");
  return DGTTA_OK;
}
