// Layout converters (NCDHW fp32 <-> channels-last storage), argmax over class rows and hard-Dice counting.
#include "conv_api.h"

namespace {

// ============================================================================ layout converters, argmax/dice
template <typename T>
__global__ void ncdhw_to_ndhwc_kernel(const float *__restrict__ src, T *__restrict__ dst, int C, int64_t V, int ldc,
                                      int64_t total) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % ldc);
    const int64_t row = i / ldc;
    const int64_t b = row / V, v = row % V;
    st_f<T>(dst + i, c < C ? src[(b * C + c) * V + v] : 0.f);
  }
}
template <typename T>
__global__ void ndhwc_to_ncdhw_kernel(const T *__restrict__ src, float *__restrict__ dst, int C, int64_t V, int ldc,
                                      int64_t total) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t v = i % V;
    const int c = (int)((i / V) % C);
    const int64_t b = i / (V * C);
    dst[i] = ld_f<T>(src + (b * V + v) * ldc + c);
  }
}

__global__ void argmax_dice_kernel(const float *__restrict__ logits, int ldc, int C, const int64_t *__restrict__ labels,
                                   int64_t *__restrict__ amax, unsigned long long *__restrict__ counts, int64_t total) {
  extern __shared__ unsigned int scnt[];  // [3*C]
  for (int i = threadIdx.x; i < 3 * C; i += blockDim.x) scnt[i] = 0;
  __syncthreads();
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    int best = 0;
    if (logits) {
      const float *p = logits + i * ldc;
      float bv = p[0];
      for (int c = 1; c < C; ++c)
        if (p[c] > bv) {  // first maximum wins, as torch.argmax
          bv = p[c];
          best = c;
        }
      if (amax) amax[i] = best;
    } else {
      best = (int)amax[i];  // predictions given
      if ((unsigned)best >= (unsigned)C) best = -1;
    }
    if (labels) {
      const int gt = (int)labels[i];
      if (best >= 0) atomicAdd(&scnt[best], 1u);
      if ((unsigned)gt < (unsigned)C) {
        atomicAdd(&scnt[C + gt], 1u);
        if (gt == best) atomicAdd(&scnt[2 * C + gt], 1u);
      }
    }
  }
  __syncthreads();
  if (labels)
    for (int i = threadIdx.x; i < 3 * C; i += blockDim.x)
      if (scnt[i]) atomicAdd(&counts[i], (unsigned long long)scnt[i]);
}

// argmax over the classes of voxel-major rows that are stored back to back (ldc == C: the sliding-window accumulator,
// 105 classes x 512^3 = 56 GB).  argmax_dice_kernel reads one row per thread - 64 lanes 420 bytes apart, 0.3 TB/s; here a
// workgroup streams 64 rows (one contiguous run, all loads in flight at once) into LDS and scans them from there: four
// threads per row take a quarter of the classes each (odd C: rows C words apart are conflict free), combined in class
// order with the same strict comparison, so the first maximum wins as before.
constexpr int AR_MAXC = 112;
constexpr int AR_RUN = (64 * AR_MAXC + 255) / 256;
template <typename ACC>
__global__ __launch_bounds__(256) void argmax_rows_kernel(const ACC *__restrict__ logits, int C, int64_t *__restrict__ amax,
                                                          int64_t total) {
  extern __shared__ float ar_tile[];          // [64][C]
  __shared__ float pv[4][64];
  __shared__ int pi[4][64];
  const int vox = threadIdx.x & 63, q = threadIdx.x >> 6;
  const int cq = (C + 3) >> 2;
  const int64_t ntile = (total + 63) >> 6;
  for (int64_t t = blockIdx.x; t < ntile; t += gridDim.x) {
    const int64_t v0 = t << 6;
    const int nv = total - v0 < 64 ? (int)(total - v0) : 64;
    const int n = nv * C;
    const ACC *lp = logits + v0 * C;
    if constexpr (sizeof(ACC) == 4) {
      float r[AR_RUN];
#pragma unroll
      for (int j = 0; j < AR_RUN; ++j) {
        const int i = (int)threadIdx.x + 256 * j;
        r[j] = i < n ? ld_f<ACC>(lp + i) : 0.f;
      }
      __syncthreads();                        // previous tile scanned
#pragma unroll
      for (int j = 0; j < AR_RUN; ++j) {
        const int i = (int)threadIdx.x + 256 * j;
        if (i < n) ar_tile[i] = r[j];
      }
    } else {
      // 16-bit rows: two classes per 32-bit load (a tile starts at voxel 64 t: 4-byte aligned for any C); the odd last
      // half of the last tile is read on its own - the word would reach past the end of the buffer
      constexpr int RUN2 = (AR_RUN + 1) / 2;
      const unsigned short *hp = reinterpret_cast<const unsigned short *>(lp);
      unsigned r[RUN2];
#pragma unroll
      for (int j = 0; j < RUN2; ++j) {
        const int i = 2 * ((int)threadIdx.x + 256 * j);
        r[j] = i + 1 < n ? *reinterpret_cast<const unsigned *>(hp + i) : (i < n ? (unsigned)hp[i] : 0u);
      }
      __syncthreads();
#pragma unroll
      for (int j = 0; j < RUN2; ++j) {
        const int i = 2 * ((int)threadIdx.x + 256 * j);
        if (i < n) ar_tile[i] = f16_to_f32((unsigned short)(r[j] & 0xffffu));
        if (i + 1 < n) ar_tile[i + 1] = f16_to_f32((unsigned short)(r[j] >> 16));
      }
    }
    __syncthreads();
    if (vox < nv) {
      const float *row = ar_tile + vox * C;
      const int c0 = q * cq, c1 = min(C, c0 + cq);
      // quarter 0 starts from class 0 as the sequential scan does; the others from "nothing yet" (-inf, replaced by
      // anything greater), so that a NaN inside a quarter is passed over exactly as in the sequential scan
      float bv = q == 0 ? row[0] : -__builtin_inff();
      int best = c0 < C ? c0 : C - 1;
      for (int c = q == 0 ? 1 : c0; c < c1; ++c)
        if (row[c] > bv) {
          bv = row[c];
          best = c;
        }
      pv[q][vox] = bv;
      pi[q][vox] = best;
    }
    __syncthreads();
    if (threadIdx.x < (unsigned)nv) {
      float bv = pv[0][threadIdx.x];
      int best = pi[0][threadIdx.x];
#pragma unroll
      for (int k = 1; k < 4; ++k)
        if (pv[k][threadIdx.x] > bv) {
          bv = pv[k][threadIdx.x];
          best = pi[k][threadIdx.x];
        }
      amax[v0 + threadIdx.x] = best;
    }
  }
}

// More classes than the LDS tile of argmax_rows_kernel holds (e.g. the 118 classes of TotalSegmentator v2 weights): one WAVE
// per row, lane l scans classes l, l + 64, ...; the partial maxima are combined so that the FIRST class that reaches the
// maximum wins and NaNs are passed over, exactly as the sequential scan does (row[0] = NaN keeps class 0).
template <typename ACC>
__global__ __launch_bounds__(256) void argmax_rows_wide_kernel(const ACC *__restrict__ logits, int C, int64_t *__restrict__ amax,
                                                               int64_t total) {
  const int lane = threadIdx.x & 63;
  const int64_t w0 = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6), nw = (int64_t)gridDim.x * 4;
  for (int64_t v = w0; v < total; v += nw) {
    const ACC *row = logits + v * C;
    float bv = -__builtin_inff();
    int best = lane < C ? lane : C - 1;
    if (lane == 0) bv = ld_f<ACC>(row);
    for (int c = lane == 0 ? 64 : lane; c < C; c += 64) {
      const float x = ld_f<ACC>(row + c);
      if (x > bv) bv = x, best = c;
    }
    const bool first_nan = __shfl(bv != bv ? 1 : 0, 0, 64) != 0;
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) {
      const float ov = __shfl_xor(bv, m, 64);
      const int ob = __shfl_xor(best, m, 64);
      if (ov > bv || (ov == bv && ob < best)) bv = ov, best = ob;
    }
    if (lane == 0) amax[v] = first_nan ? 0 : best;
  }
}

}  // namespace

extern "C" int dgtta_ncdhw_to_ndhwc(const float *src, void *dst, int B, int C, int64_t V, int ldc, int dtype,
                                    void *stream) {
  DG_REQUIRE(src && dst && B > 0 && C > 0 && V > 0 && ldc >= C, DGTTA_ERR_BADARG, "ncdhw_to_ndhwc: bad args");
  const int64_t total = (int64_t)B * V * ldc;
  DISPATCH_T(dtype, hipLaunchKernelGGL((ncdhw_to_ndhwc_kernel<T>), dim3(gs_blocks(total)), dim3(256), 0,
                                       (hipStream_t)stream, src, (T *)dst, C, V, ldc, total));
  DG_CHECK_LAUNCH("ncdhw_to_ndhwc_kernel");
  return DGTTA_OK;
}

extern "C" int dgtta_ndhwc_to_ncdhw(const void *src, float *dst, int B, int C, int64_t V, int ldc, int dtype,
                                    void *stream) {
  DG_REQUIRE(src && dst && B > 0 && C > 0 && V > 0 && ldc >= C, DGTTA_ERR_BADARG, "ndhwc_to_ncdhw: bad args");
  const int64_t total = (int64_t)B * V * C;
  DISPATCH_T(dtype, hipLaunchKernelGGL((ndhwc_to_ncdhw_kernel<T>), dim3(gs_blocks(total)), dim3(256), 0,
                                       (hipStream_t)stream, (const T *)src, dst, C, V, ldc, total));
  DG_CHECK_LAUNCH("ndhwc_to_ncdhw_kernel");
  return DGTTA_OK;
}

extern "C" int dgtta_argmax_rows(const void *logits, int acc_dtype, int C, int64_t rows, int64_t *argmax_out, void *stream) {
  DG_REQUIRE(logits && argmax_out && rows > 0, DGTTA_ERR_BADARG, "argmax_rows: bad args");
  DG_REQUIRE(C > 0 && C <= 65536, DGTTA_ERR_UNSUPPORTED, "argmax_rows: C %d", C);
  DG_REQUIRE(acc_dtype == DGTTA_F32 || acc_dtype == DGTTA_F16, DGTTA_ERR_UNSUPPORTED, "argmax_rows: rows are fp32 or fp16");
  DG_REQUIRE(((uintptr_t)logits & 3) == 0, DGTTA_ERR_BADARG, "argmax_rows: rows must start on a 4-byte boundary");
  if (C > AR_MAXC) {      // wider than the LDS tile: one wave per row
    const dim3 gridw((unsigned)(cdiv64(rows, 4) < 16384 ? cdiv64(rows, 4) : 16384));
    if (acc_dtype == DGTTA_F32)
      hipLaunchKernelGGL(argmax_rows_wide_kernel<float>, gridw, dim3(256), 0, (hipStream_t)stream, (const float *)logits, C, argmax_out, rows);
    else
      hipLaunchKernelGGL(argmax_rows_wide_kernel<f16_t>, gridw, dim3(256), 0, (hipStream_t)stream, (const f16_t *)logits, C, argmax_out, rows);
    DG_CHECK_LAUNCH("argmax_rows_wide_kernel");
    return DGTTA_OK;
  }
  const int64_t ntile = cdiv64(rows, 64);
  const dim3 grid((unsigned)(ntile < 4096 ? ntile : 4096));
  const size_t lds = (size_t)64 * C * sizeof(float);
  if (acc_dtype == DGTTA_F32)
    hipLaunchKernelGGL(argmax_rows_kernel<float>, grid, dim3(256), lds, (hipStream_t)stream, (const float *)logits, C, argmax_out,
                       rows);
  else
    hipLaunchKernelGGL(argmax_rows_kernel<f16_t>, grid, dim3(256), lds, (hipStream_t)stream, (const f16_t *)logits, C, argmax_out,
                       rows);
  DG_CHECK_LAUNCH("argmax_rows_kernel");
  return DGTTA_OK;
}

extern "C" int dgtta_argmax_dice(const float *logits, int ldc, int C, const int64_t *labels, int64_t *argmax_out,
                                 int64_t *counts, int B, int64_t V, void *stream) {
  DG_REQUIRE((logits || argmax_out) && C > 0 && C <= 1024 && (!logits || ldc >= C) && B > 0 && V > 0, DGTTA_ERR_BADARG,
             "argmax_dice: bad args");
  DG_REQUIRE(!labels || counts, DGTTA_ERR_BADARG, "argmax_dice: labels without counts");
  const int64_t total = (int64_t)B * V;
  // back-to-back rows, no Dice counts asked for (the sliding-window label map): the streaming kernel
  if (logits && !labels && argmax_out && ldc == C && C <= AR_MAXC && total >= 4096)
    return dgtta_argmax_rows(logits, DGTTA_F32, C, total, argmax_out, stream);
  hipLaunchKernelGGL(argmax_dice_kernel, dim3(gs_blocks(total, 2048)), dim3(256), 3 * C * sizeof(unsigned int),
                     (hipStream_t)stream, logits, ldc, C, labels, argmax_out, (unsigned long long *)counts, total);
  DG_CHECK_LAUNCH("argmax_dice_kernel");
  return DGTTA_OK;
}
