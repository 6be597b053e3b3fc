// 1x1x1 segmentation head on selected rows of the weight (map_label folded in): forward, data gradient, weight gradient.
// VALU kernels by shape (general, 32-channel register rows, LDS-staged coalesced, wide 33..128 classes); the MFMA weight
// gradient of the production shape is head_wgrad_mfma (head_wgrad.hip); heads with more than 32 input channels in 16-bit
// storage (the auxiliary heads of deep supervision) run the matrix-core kernels of seghead_mfma.hip.
#include "conv_api.h"

namespace {

// ============================================================================ 1x1x1 head on selected rows
template <typename T, bool NDHWC>
__global__ void head_fwd_kernel(const T *__restrict__ x, int ldx, const float *__restrict__ w,
                                const float *__restrict__ bias, const int *__restrict__ sel, int nsel,
                                float *__restrict__ out, int ldo, int Cin, int64_t V, int64_t total) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    int k;
    int64_t row;
    if (NDHWC) {
      k = (int)(i % nsel);
      row = i / nsel;
    } else {  // i = (b*nsel + k)*V + v
      const int64_t v = i % V;
      k = (int)((i / V) % nsel);
      row = (i / (V * nsel)) * V + v;
    }
    const int r = sel ? sel[k] : k;
    const T *xp = x + row * ldx;
    const float *wp = w + (int64_t)r * Cin;
    float acc = 0.f;
    for (int ci = 0; ci < Cin; ++ci) acc = __builtin_fmaf(ld_f<T>(xp + ci), wp[ci], acc);
    acc += bias[r];
    if (NDHWC) out[row * ldo + k] = acc;
    else out[i] = acc;
  }
}

template <typename T, bool ACC>
__global__ void head_dgrad_kernel(const float *__restrict__ dout, int lddo, const float *__restrict__ w,
                                  const int *__restrict__ sel, int nsel, T *__restrict__ dx, int lddx, int Cin,
                                  int64_t total) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int ci = (int)(i % Cin);
    const int64_t row = i / Cin;
    float acc = 0.f;
    for (int k = 0; k < nsel; ++k) acc = __builtin_fmaf(dout[row * lddo + k], w[(int64_t)(sel ? sel[k] : k) * Cin + ci], acc);
    if (ACC) acc += ld_f<T>(dx + row * lddx + ci);      // the rows already hold another consumer's gradient
    st_f<T>(dx + row * lddx + ci, acc);
  }
}

// Fast head kernels for the production shape (CIN input channels, nsel <= 32 selected rows): one thread per voxel, the
// activation row lives in registers (16-byte loads), the selected weight rows in LDS (broadcast reads).
template <typename T, int CIN, bool NDHWC>
__global__ __launch_bounds__(256) void head_fwd_fast_kernel(const T *__restrict__ x, int ldx, const float *__restrict__ w,
                                                            const float *__restrict__ bias, const int *__restrict__ sel,
                                                            int nsel, float *__restrict__ out, int ldo, int64_t V,
                                                            int64_t rows) {
  constexpr int EPV = 16 / sizeof(T);
  __shared__ float sw[128 * CIN + 128];
  for (int i = threadIdx.x; i < nsel * CIN; i += 256) sw[i] = w[(int64_t)(sel ? sel[i / CIN] : i / CIN) * CIN + i % CIN];
  for (int i = threadIdx.x; i < nsel; i += 256) sw[128 * CIN + i] = bias[sel ? sel[i] : i];
  __syncthreads();
  for (int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x; row < rows; row += (int64_t)gridDim.x * 256) {
    float xr[CIN];
#pragma unroll
    for (int g = 0; g < CIN / EPV; ++g)
      unpack16<T>(*reinterpret_cast<const uint4 *>(x + row * ldx + g * EPV), xr + g * EPV);
    for (int k = 0; k < nsel; ++k) {
      float acc = 0.f;
#pragma unroll
      for (int ci = 0; ci < CIN; ++ci) acc = __builtin_fmaf(xr[ci], sw[k * CIN + ci], acc);
      acc += sw[128 * CIN + k];
      if (NDHWC) out[row * ldo + k] = acc;
      else out[((row / V) * nsel + k) * V + row % V] = acc;
    }
  }
}

template <typename T, int CIN>
__global__ __launch_bounds__(256) void head_dgrad_fast_kernel(const float *__restrict__ dout, int lddo,
                                                              const float *__restrict__ w, const int *__restrict__ sel,
                                                              int nsel, T *__restrict__ dx, int lddx, int64_t rows) {
  __shared__ float sw[32 * CIN];
  for (int i = threadIdx.x; i < nsel * CIN; i += 256) sw[i] = w[(int64_t)(sel ? sel[i / CIN] : i / CIN) * CIN + i % CIN];
  __syncthreads();
  for (int64_t row = (int64_t)blockIdx.x * 256 + threadIdx.x; row < rows; row += (int64_t)gridDim.x * 256) {
    float acc[CIN];
#pragma unroll
    for (int ci = 0; ci < CIN; ++ci) acc[ci] = 0.f;
    for (int k = 0; k < nsel; ++k) {
      const float g = dout[row * lddo + k];
#pragma unroll
      for (int ci = 0; ci < CIN; ++ci) acc[ci] = __builtin_fmaf(g, sw[k * CIN + ci], acc[ci]);
    }
#pragma unroll
    for (int ci = 0; ci < CIN; ++ci) st_f<T>(dx + row * lddx + ci, acc[ci]);
  }
}

// Coalesced variants for the production shape (32 input channels in contiguous 64-byte bf16 rows / 128-byte fp32 rows,
// nsel <= 16 selected classes in contiguous fp32 rows): a workgroup moves 256 rows through LDS in both directions, so
// that every global access is a contiguous 16-byte-per-lane stream (thread-per-row loads touch 64 cache lines per
// instruction, and the per-class 4-byte stores 64 lines for 256 bytes).
template <typename T>
__global__ __launch_bounds__(256) void head_fwd_lds_kernel(const T *__restrict__ x, const float *__restrict__ w,
                                                           const float *__restrict__ bias, const int *__restrict__ sel,
                                                           int nsel, float *__restrict__ out, int64_t rows) {
  constexpr int CIN = 32, EPV = 16 / sizeof(T), XU = CIN / EPV;      // uint4 per input row
  constexpr int XP = XU + 1;                                          // padded row pitch in uint4
  __shared__ float sw[16 * CIN + 16];
  __shared__ uint4 sx[256 * XP];
  __shared__ float so[256 * 17];
  for (int i = threadIdx.x; i < nsel * CIN; i += 256) sw[i] = w[(int64_t)(sel ? sel[i / CIN] : i / CIN) * CIN + i % CIN];
  for (int i = threadIdx.x; i < nsel; i += 256) sw[16 * CIN + i] = bias[sel ? sel[i] : i];
  for (int64_t r0 = (int64_t)blockIdx.x * 256; r0 < rows; r0 += (int64_t)gridDim.x * 256) {
    const int nr = rows - r0 < 256 ? (int)(rows - r0) : 256;
    __syncthreads();
    const uint4 *gx = reinterpret_cast<const uint4 *>(x + r0 * CIN);
    for (int i = threadIdx.x; i < nr * XU; i += 256) sx[(i / XU) * XP + i % XU] = gx[i];
    __syncthreads();
    if ((int)threadIdx.x < nr) {
      float xr[CIN];
#pragma unroll
      for (int g = 0; g < XU; ++g) unpack16<T>(sx[threadIdx.x * XP + g], xr + g * EPV);
      for (int k = 0; k < nsel; ++k) {
        float acc = 0.f;
#pragma unroll
        for (int ci = 0; ci < CIN; ++ci) acc = __builtin_fmaf(xr[ci], sw[k * CIN + ci], acc);
        so[threadIdx.x * 17 + k] = acc + sw[16 * CIN + k];
      }
    }
    __syncthreads();
    float *go = out + r0 * nsel;
    for (int i = threadIdx.x; i < nr * nsel; i += 256) go[i] = so[(i / nsel) * 17 + i % nsel];
  }
}

template <typename T>
__global__ __launch_bounds__(256) void head_dgrad_lds_kernel(const float *__restrict__ dout, const float *__restrict__ w,
                                                             const int *__restrict__ sel, int nsel, T *__restrict__ dx,
                                                             int64_t rows, unsigned short *__restrict__ d16) {
  // d16 != NULL: also leave the 16-bit copy of dout [rows][nsel] that the MFMA weight gradient of the head reads (saves
  // its own conversion pass over the fp32 gradient)
  constexpr int CIN = 32, EPV = 16 / sizeof(T), XU = CIN / EPV, XP = XU + 1;
  __shared__ float sw[16 * CIN];
  __shared__ float sg[256 * 17];
  __shared__ uint4 sx[256 * XP];
  for (int i = threadIdx.x; i < nsel * CIN; i += 256) sw[i] = w[(int64_t)(sel ? sel[i / CIN] : i / CIN) * CIN + i % CIN];
  for (int64_t r0 = (int64_t)blockIdx.x * 256; r0 < rows; r0 += (int64_t)gridDim.x * 256) {
    const int nr = rows - r0 < 256 ? (int)(rows - r0) : 256;
    __syncthreads();
    const float *gg = dout + r0 * nsel;
    for (int i = threadIdx.x; i < nr * nsel; i += 256) {
      const float v = gg[i];
      sg[(i / nsel) * 17 + i % nsel] = v;
      if constexpr (sizeof(T) == 2) {
        if (d16 && nsel != 16) d16[r0 * nsel + i] = f32_to_16<T>(v);
      }
    }
    __syncthreads();
    if constexpr (sizeof(T) == 2) {
      if (d16 && nsel == 16 && (int)threadIdx.x < nr) {      // one 32-byte row per thread: two 16-byte stores
        uint4 *o = reinterpret_cast<uint4 *>(d16 + (r0 + threadIdx.x) * 16);
        const float *g = sg + threadIdx.x * 17;
        o[0] = make_uint4(pack2_16<T>(g[0], g[1]), pack2_16<T>(g[2], g[3]), pack2_16<T>(g[4], g[5]), pack2_16<T>(g[6], g[7]));
        o[1] = make_uint4(pack2_16<T>(g[8], g[9]), pack2_16<T>(g[10], g[11]), pack2_16<T>(g[12], g[13]),
                          pack2_16<T>(g[14], g[15]));
      }
    }
    if ((int)threadIdx.x < nr) {
      float acc[CIN];
#pragma unroll
      for (int ci = 0; ci < CIN; ++ci) acc[ci] = 0.f;
      for (int k = 0; k < nsel; ++k) {
        const float g = sg[threadIdx.x * 17 + k];
#pragma unroll
        for (int ci = 0; ci < CIN; ++ci) acc[ci] = __builtin_fmaf(g, sw[k * CIN + ci], acc[ci]);
      }
#pragma unroll
      for (int g = 0; g < XU; ++g) sx[threadIdx.x * XP + g] = pack16<T>(acc + g * EPV);
    }
    __syncthreads();
    uint4 *gx = reinterpret_cast<uint4 *>(dx + r0 * CIN);
    for (int i = threadIdx.x; i < nr * XU; i += 256) gx[i] = sx[(i / XU) * XP + i % XU];
  }
}

// partial[split][k][ci] ; grid (pairs/256, nsplit)
template <typename T>
__global__ void head_wgrad_kernel(const T *__restrict__ x, int ldx, const float *__restrict__ dout, int lddo,
                                  float *__restrict__ part, int Cin, int nsel, int64_t rows) {
  const int pair = blockIdx.x * blockDim.x + threadIdx.x;
  if (pair >= Cin * nsel) return;
  const int ci = pair % Cin, k = pair / Cin;
  const int64_t per = cdiv64(rows, gridDim.y);
  const int64_t r0 = (int64_t)blockIdx.y * per, r1 = (r0 + per < rows) ? r0 + per : rows;
  float acc = 0.f;
  for (int64_t r = r0; r < r1; ++r) acc = __builtin_fmaf(dout[r * lddo + k], ld_f<T>(x + r * ldx + ci), acc);
  part[((int64_t)blockIdx.y * nsel + k) * Cin + ci] = acc;
}

// Wide head (32 input channels, 33..128 evaluated classes - the full 105-class head of a pre-training step or of a TTA run whose
// model-output modifier is user code, so that map_label cannot be folded into the head): round 5.  The one-thread-per-output
// kernels above walk a 420-byte row per lane (head_dgrad_kernel 9.1 ms, head_wgrad_kernel 11.9 ms per 2 x 128^3 step); here a
// workgroup stages 64 rows of dout (one contiguous run) and of x through LDS.
constexpr int HWD_ROWS = 64, HWD_MAXK = 128;
// n contiguous floats -> LDS rows of `cols` values at pitch LDP: EIGHT loads in flight per thread before the first LDS store (a
// load - store loop pays the memory latency once per element: the first version of these kernels spent 40 us per tile in it)
__device__ __forceinline__ void hwd_stage_rows(float *tile, const float *src, int n, int cols, int LDP) {
  for (int e0 = threadIdx.x; e0 < n; e0 += 256 * 8) {
    float tmp[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int e = e0 + 256 * u;
      tmp[u] = e < n ? src[e] : 0.f;
    }
#pragma unroll
    for (int u = 0; u < 8; ++u) {
      const int e = e0 + 256 * u;
      if (e < n) {
        const int v = e / cols;
        tile[v * LDP + (e - v * cols)] = tmp[u];
      }
    }
  }
}
//   dx[r][ci] = sum_k dout[r][k] w[sel k][ci]: thread = (row, 8-channel group); dout row element broadcast to the row's 4 threads,
//   weight rows broadcast to all rows
template <typename T>
__global__ __launch_bounds__(256) void head_dgrad_wide_kernel(const float *__restrict__ dout, int lddo, const float *__restrict__ w,
                                                            const int *__restrict__ sel, int nsel, T *__restrict__ dx, int lddx,
                                                            int64_t rows) {
  extern __shared__ float hw_smem[];
  float *sw = hw_smem;                    // [nsel][32]
  float *sg = hw_smem + HWD_MAXK * 32;    // [64][nsel | 1]
  const int LDP = nsel | 1;
  for (int i = threadIdx.x; i < nsel * 32; i += 256) sw[i] = w[(int64_t)(sel ? sel[i >> 5] : i >> 5) * 32 + (i & 31)];
  const int r = threadIdx.x >> 2, g = threadIdx.x & 3;
  const int64_t ntile = (rows + HWD_ROWS - 1) / HWD_ROWS;
  for (int64_t t = blockIdx.x; t < ntile; t += gridDim.x) {
    const int64_t r0 = t * HWD_ROWS;
    const int nv = rows - r0 < HWD_ROWS ? (int)(rows - r0) : HWD_ROWS;
    __syncthreads();
    if (lddo == nsel) {
      hwd_stage_rows(sg, dout + r0 * lddo, nv * nsel, nsel, LDP);
    } else {
      for (int e = threadIdx.x; e < nv * nsel; e += 256) {
        const int v = e / nsel, k = e - v * nsel;
        sg[v * LDP + k] = dout[(r0 + v) * lddo + k];
      }
    }
    __syncthreads();
    if (r < nv) {
      float acc[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
      const float *gr = sg + r * LDP;
      for (int k = 0; k < nsel; ++k) {
        const float gk = gr[k];
        const float4 w0 = *reinterpret_cast<const float4 *>(sw + k * 32 + 8 * g), w1 = *reinterpret_cast<const float4 *>(sw + k * 32 + 8 * g + 4);
        acc[0] = __builtin_fmaf(gk, w0.x, acc[0]);
        acc[1] = __builtin_fmaf(gk, w0.y, acc[1]);
        acc[2] = __builtin_fmaf(gk, w0.z, acc[2]);
        acc[3] = __builtin_fmaf(gk, w0.w, acc[3]);
        acc[4] = __builtin_fmaf(gk, w1.x, acc[4]);
        acc[5] = __builtin_fmaf(gk, w1.y, acc[5]);
        acc[6] = __builtin_fmaf(gk, w1.z, acc[6]);
        acc[7] = __builtin_fmaf(gk, w1.w, acc[7]);
      }
      T *o = dx + (r0 + r) * lddx + 8 * g;
#pragma unroll
      for (int q = 0; q < 8; ++q) st_f<T>(o + q, acc[q]);
    }
  }
}

//   part[split][k][ci] = sum over the split's rows of dout[r][k] x[r][ci]: thread = (ci, class residue t >> 5 of 8), accumulators for
//   classes (t >> 5) + 8 j; grid.x = splits, each a contiguous range of 64-row tiles (deterministic: fixed order inside a split,
//   reduce_splits_kernel adds the splits in order)
template <typename T>
__global__ __launch_bounds__(256) void head_wgrad_wide_kernel(const T *__restrict__ x, int ldx, const float *__restrict__ dout,
                                                            int lddo, float *__restrict__ part, int nsel, int64_t rows) {
  extern __shared__ float hw_smem[];
  float *sx = hw_smem;                    // [64][33]
  float *sg = hw_smem + HWD_ROWS * 33;    // [64][nsel | 1]
  const int LDP = nsel | 1;
  const int ci = threadIdx.x & 31, cg = threadIdx.x >> 5;
  constexpr int NJ = HWD_MAXK / 8;
  float acc[NJ];
#pragma unroll
  for (int j = 0; j < NJ; ++j) acc[j] = 0.f;
  const int64_t ntile = (rows + HWD_ROWS - 1) / HWD_ROWS;
  const int64_t per = (ntile + gridDim.x - 1) / gridDim.x;
  const int64_t t0 = (int64_t)blockIdx.x * per, t1 = t0 + per < ntile ? t0 + per : ntile;
  for (int64_t t = t0; t < t1; ++t) {
    const int64_t r0 = t * HWD_ROWS;
    const int nv = rows - r0 < HWD_ROWS ? (int)(rows - r0) : HWD_ROWS;
    __syncthreads();
    {     // x rows: 8 loads in flight per thread (64 x 32 values = 8 per thread)
      float tx[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int e = threadIdx.x + 256 * u, v = e >> 5, c = e & 31;
        tx[u] = v < nv ? ld_f<T>(x + (r0 + v) * ldx + c) : 0.f;
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int e = threadIdx.x + 256 * u;
        sx[(e >> 5) * 33 + (e & 31)] = tx[u];
      }
    }
    if (lddo == nsel) {
      hwd_stage_rows(sg, dout + r0 * lddo, nv * nsel, nsel, LDP);
      for (int e = nv * nsel + threadIdx.x; e < HWD_ROWS * nsel; e += 256) {      // ragged last tile: zero rows
        const int v = e / nsel;
        sg[v * LDP + (e - v * nsel)] = 0.f;
      }
    } else {
      for (int e = threadIdx.x; e < HWD_ROWS * nsel; e += 256) {
        const int v = e / nsel, k = e - v * nsel;
        sg[v * LDP + k] = v < nv ? dout[(r0 + v) * lddo + k] : 0.f;
      }
    }
    __syncthreads();
    // branch free: all NJ products per row, also for classes >= nsel (they read the next row's values - the tile is padded by
    // HWD_MAXK floats - into accumulators that are never stored).  A per-class guard turned every product into its own
    // read - wait - fma - branch block: 9.5 ms instead of 1
#pragma unroll 4
    for (int v = 0; v < HWD_ROWS; ++v) {
      const float xv = sx[v * 33 + ci];
      const float *gr = sg + v * LDP + cg;
      float gv[NJ];
#pragma unroll
      for (int j = 0; j < NJ; ++j) gv[j] = gr[8 * j];
#pragma unroll
      for (int j = 0; j < NJ; ++j) acc[j] = __builtin_fmaf(gv[j], xv, acc[j]);
    }
  }
#pragma unroll
  for (int j = 0; j < NJ; ++j)
    if (cg + 8 * j < nsel) part[((int64_t)blockIdx.x * nsel + cg + 8 * j) * 32 + ci] = acc[j];
}

}  // namespace

extern "C" int dgtta_seghead_fwd(const void *x, int ldx, const float *w, const float *bias, const int *sel, int nsel,
                                 float *out, int out_ndhwc, int ldo, int B, int Cin, int64_t V, int dtype,
                                 void *stream) {
  DG_REQUIRE(x && w && bias && out, DGTTA_ERR_BADARG, "seghead_fwd: null pointer");
  DG_REQUIRE(B > 0 && Cin > 0 && nsel > 0 && V > 0 && ldx >= Cin && (!out_ndhwc || ldo >= nsel), DGTTA_ERR_BADARG,
             "seghead_fwd: bad dims");
  if (Cin == 32 && nsel <= 128 && ldx % 8 == 0 && ((uintptr_t)x & 15) == 0) {
    const int64_t rows = (int64_t)B * V;
    const int blocks = (int)(cdiv64(rows, 256) < 8192 ? cdiv64(rows, 256) : 8192);
    if (out_ndhwc && ldx == 32 && ldo == nsel && nsel <= 16 && ((uintptr_t)out & 15) == 0) {
      DISPATCH_T(dtype, hipLaunchKernelGGL((head_fwd_lds_kernel<T>), dim3(blocks), dim3(256), 0, (hipStream_t)stream,
                                           (const T *)x, w, bias, sel, nsel, out, rows));
      DG_CHECK_LAUNCH("head_fwd_lds_kernel");
      return DGTTA_OK;
    }
    if (out_ndhwc)
      DISPATCH_T(dtype, hipLaunchKernelGGL((head_fwd_fast_kernel<T, 32, true>), dim3(blocks), dim3(256), 0,
                                           (hipStream_t)stream, (const T *)x, ldx, w, bias, sel, nsel, out, ldo, V, rows));
    else
      DISPATCH_T(dtype, hipLaunchKernelGGL((head_fwd_fast_kernel<T, 32, false>), dim3(blocks), dim3(256), 0,
                                           (hipStream_t)stream, (const T *)x, ldx, w, bias, sel, nsel, out, ldo, V, rows));
    DG_CHECK_LAUNCH("head_fwd_fast_kernel");
    return DGTTA_OK;
  }
  if (Cin != 32 && out_ndhwc) {      // more than 32 channels in 16-bit storage (the auxiliary heads): matrix cores
    const int rc = head_fwd_mfma(x, ldx, w, bias, sel, nsel, out, ldo, Cin, (int64_t)B * V, dtype, (hipStream_t)stream);
    if (rc != DGTTA_ERR_UNSUPPORTED) return rc;
  }
  const int64_t total = (int64_t)B * V * nsel;
  if (out_ndhwc)
    DISPATCH_T(dtype, hipLaunchKernelGGL((head_fwd_kernel<T, true>), dim3(gs_blocks(total, 1 << 20)), dim3(256), 0,
                                         (hipStream_t)stream, (const T *)x, ldx, w, bias, sel, nsel, out, ldo, Cin, V,
                                         total));
  else
    DISPATCH_T(dtype, hipLaunchKernelGGL((head_fwd_kernel<T, false>), dim3(gs_blocks(total, 1 << 20)), dim3(256), 0,
                                         (hipStream_t)stream, (const T *)x, ldx, w, bias, sel, nsel, out, ldo, Cin, V,
                                         total));
  DG_CHECK_LAUNCH("head_fwd_kernel");
  return DGTTA_OK;
}

static int head_splits(int64_t rows) {
  int64_t s = cdiv64(rows, 2048);
  return (int)(s < 256 ? (s > 0 ? s : 1) : 256);
}

// workspace layout: [bias partials][main: split partials (VALU) | bf16 copy + slabs (MFMA)]
static size_t head_bias_region(int B, int nsel, int64_t V) {
  return align_up((size_t)B * reduce_blocks(V, B) * nsel * 2 * sizeof(double), 256);
}

extern "C" size_t dgtta_seghead_bwd_ws_bytes(int B, int Cin, int nsel, int64_t V) {
  if (B <= 0 || Cin <= 0 || nsel <= 0 || V <= 0) return 0;      // a size query of an empty problem (the launchers reject it with DGTTA_ERR_BADARG)
  size_t a = align_up((size_t)head_splits((int64_t)B * V) * nsel * Cin * sizeof(float), 256);
  size_t c = align_up(head_wgrad_mfma_ws_bytes(Cin, nsel, (int64_t)B * V), 256);
  return head_bias_region(B, nsel, V) + (a > c ? a : c);
}

// data gradient on the vector ALUs: the general kernel where dx is added to or the shape has no kernel of its own, else the
// 32-channel kernels (they overwrite).  *d16: set where the kernel leaves a 16-bit copy of dout at ws_main for head_wgrad_mfma
static int head_dgrad_valu(const float *dout, int lddo, const float *w, const int *sel, int nsel, void *dx, int lddx, bool want_d16,
                           void *ws_main, size_t main_bytes, int Cin, int64_t rows, int accumulate_dx, int dtype, hipStream_t st,
                           unsigned short **d16) {
  if (accumulate_dx || Cin != 32 || nsel > HWD_MAXK) {
    const int64_t total = rows * Cin;
    if (accumulate_dx)
      DISPATCH_T(dtype, hipLaunchKernelGGL((head_dgrad_kernel<T, true>), dim3(gs_blocks(total, 1 << 20)), dim3(256), 0, st, dout,
                                           lddo, w, sel, nsel, (T *)dx, lddx, Cin, total));
    else
      DISPATCH_T(dtype, hipLaunchKernelGGL((head_dgrad_kernel<T, false>), dim3(gs_blocks(total, 1 << 20)), dim3(256), 0, st, dout,
                                           lddo, w, sel, nsel, (T *)dx, lddx, Cin, total));
    DG_CHECK_LAUNCH("head_dgrad_kernel");
    return DGTTA_OK;
  }
  if (nsel <= 32) {
    const int blocks = (int)(cdiv64(rows, 256) < 8192 ? cdiv64(rows, 256) : 8192);
    if (lddx == 32 && lddo == nsel && nsel <= 16 && ((uintptr_t)dx & 15) == 0) {
      if (want_d16 && dtype != DGTTA_F32 && head_wgrad_mfma_ws_bytes(Cin, nsel, rows) > 0 &&
          main_bytes >= head_wgrad_mfma_ws_bytes(Cin, nsel, rows)) {
        *d16 = (unsigned short *)ws_main;       // the first region of head_wgrad_mfma's workspace
      }
      DISPATCH_T(dtype, hipLaunchKernelGGL((head_dgrad_lds_kernel<T>), dim3(blocks), dim3(256), 0, st, dout, w, sel, nsel,
                                           (T *)dx, rows, *d16));
      DG_CHECK_LAUNCH("head_dgrad_lds_kernel");
    } else {
      DISPATCH_T(dtype, hipLaunchKernelGGL((head_dgrad_fast_kernel<T, 32>), dim3(blocks), dim3(256), 0, st, dout, lddo, w,
                                           sel, nsel, (T *)dx, lddx, rows));
      DG_CHECK_LAUNCH("head_dgrad_fast_kernel");
    }
    return DGTTA_OK;
  }
  // the wide head: 64-row tiles through LDS
  const size_t lds = ((size_t)HWD_MAXK * 32 + (size_t)HWD_ROWS * (nsel | 1)) * sizeof(float);
  const int64_t nt = cdiv64(rows, HWD_ROWS);
  DISPATCH_T(dtype, {
    static DynLdsOnce once;
    DG_REQUIRE(ensure_dyn_lds(once, reinterpret_cast<const void *>(head_dgrad_wide_kernel<T>),
                              (HWD_MAXK * 32 + HWD_ROWS * (HWD_MAXK | 1)) * (int)sizeof(float)) == hipSuccess,
               DGTTA_ERR_LAUNCH, "seghead_bwd: cannot raise the dynamic LDS limit");
    hipLaunchKernelGGL((head_dgrad_wide_kernel<T>), dim3((unsigned)(nt < 4096 ? nt : 4096)), dim3(256), lds, st, dout, lddo, w, sel,
                       nsel, (T *)dx, lddx, rows);
  });
  DG_CHECK_LAUNCH("head_dgrad_wide_kernel");
  return DGTTA_OK;
}

// per-split partials of the weight gradient, part[ns][nsel][Cin], on the vector ALUs
static int head_wgrad_parts_valu(const void *x, int ldx, const float *dout, int lddo, float *part, int ns, int nsel, int Cin,
                                 int64_t rows, int dtype, hipStream_t st) {
  if (Cin == 32 && nsel > 32 && nsel <= HWD_MAXK) {
    const size_t lds = ((size_t)HWD_ROWS * 33 + (size_t)HWD_ROWS * (nsel | 1) + HWD_MAXK) * sizeof(float);
    DISPATCH_T(dtype, {
      static DynLdsOnce once;
      DG_REQUIRE(ensure_dyn_lds(once, reinterpret_cast<const void *>(head_wgrad_wide_kernel<T>),
                                (HWD_ROWS * 33 + HWD_ROWS * (HWD_MAXK | 1) + HWD_MAXK) * (int)sizeof(float)) == hipSuccess,
                 DGTTA_ERR_LAUNCH, "seghead_bwd: cannot raise the dynamic LDS limit");
      hipLaunchKernelGGL((head_wgrad_wide_kernel<T>), dim3(ns), dim3(256), lds, st, (const T *)x, ldx, dout, lddo, part, nsel, rows);
    });
    DG_CHECK_LAUNCH("head_wgrad_wide_kernel");
    return DGTTA_OK;
  }
  DISPATCH_T(dtype, hipLaunchKernelGGL((head_wgrad_kernel<T>), dim3(cdiv(Cin * nsel, 256), ns), dim3(256), 0, st, (const T *)x, ldx,
                                       dout, lddo, part, Cin, nsel, rows));
  DG_CHECK_LAUNCH("head_wgrad_kernel");
  return DGTTA_OK;
}

static int seghead_bwd(const void *x, int ldx, const float *dout, int lddo, const float *w, const int *sel, int nsel, void *dx,
                       int lddx, float *dw_sel, float *db_sel, void *ws, size_t ws_bytes, int B, int Cin, int64_t V, int accumulate,
                       int accumulate_dx, int dtype, void *stream) {
  DG_REQUIRE(x && dout && w && ws, DGTTA_ERR_BADARG, "seghead_bwd: null pointer");
  DG_REQUIRE(B > 0 && Cin > 0 && nsel > 0 && V > 0 && ldx >= Cin && lddo >= nsel, DGTTA_ERR_BADARG, "seghead_bwd: bad dims");
  DG_REQUIRE(ws_bytes >= dgtta_seghead_bwd_ws_bytes(B, Cin, nsel, V), DGTTA_ERR_WORKSPACE, "seghead_bwd: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  const int64_t rows = (int64_t)B * V;
  void *ws_bias = ws;
  void *ws_main = (char *)ws + head_bias_region(B, nsel, V);
  const size_t main_bytes = ws_bytes - head_bias_region(B, nsel, V);
  unsigned short *d16 = nullptr;      // 16-bit copy of dout written by the data-gradient kernel for the weight gradient
  if (dx) {
    DG_REQUIRE(lddx >= Cin, DGTTA_ERR_BADARG, "seghead_bwd: lddx < Cin");
    // adding to dx (an auxiliary head: the rows hold the transposed conv's gradient) or more than 32 channels: the matrix-core
    // kernel where it applies; everything else on the vector ALUs.  (accumulate_dx with Cin == 32 in 16-bit storage also lands on
    // the matrix-core kernel: no head of a real plan asks for it - the 32-channel head is the full-resolution one, whose rows
    // nobody wrote before - but the entry point accepts it.  That kernel leaves no 16-bit copy of dout, so d16 stays null and
    // head_wgrad_mfma converts dout itself.)
    int rc = DGTTA_ERR_UNSUPPORTED;
    if (accumulate_dx || Cin != 32) rc = head_dgrad_mfma(dout, lddo, w, sel, nsel, dx, lddx, Cin, rows, accumulate_dx, dtype, st);
    if (rc == DGTTA_ERR_UNSUPPORTED)
      rc = head_dgrad_valu(dout, lddo, w, sel, nsel, dx, lddx, dw_sel != nullptr, ws_main, main_bytes, Cin, rows, accumulate_dx, dtype,
                           st, &d16);
    if (rc != DGTTA_OK) return rc;
  }
  if (dw_sel) {
    int rc = head_wgrad_mfma(x, ldx, dout, lddo, dw_sel, ws_main, main_bytes, Cin, nsel, rows, accumulate, dtype, st,
                             d16 != nullptr);
    if (rc == DGTTA_ERR_UNSUPPORTED) {      // per-split partials (the 32-channel kernels keep their shapes), added in order
      const int ns = head_splits(rows);
      float *part = (float *)ws_main;
      rc = DGTTA_ERR_UNSUPPORTED;
      if (Cin != 32) rc = head_wgrad_rows_mfma(x, ldx, dout, lddo, part, ns, nsel, Cin, rows, dtype, st);
      if (rc == DGTTA_ERR_UNSUPPORTED) rc = head_wgrad_parts_valu(x, ldx, dout, lddo, part, ns, nsel, Cin, rows, dtype, st);
      if (rc == DGTTA_OK) rc = reduce_splits(part, dw_sel, (int64_t)nsel * Cin, ns, accumulate, st);
    }
    if (rc != DGTTA_OK) return rc;
  }
  if (db_sel) return conv_bias_grad(dout, lddo, db_sel, ws_bias, B, nsel, V, accumulate, DGTTA_F32, st);
  return DGTTA_OK;
}

extern "C" int dgtta_seghead_bwd(const void *x, int ldx, const float *dout, int lddo, const float *w, const int *sel,
                                 int nsel, void *dx, int lddx, float *dw_sel, float *db_sel, void *ws, size_t ws_bytes,
                                 int B, int Cin, int64_t V, int accumulate, int dtype, void *stream) {
  return seghead_bwd(x, ldx, dout, lddo, w, sel, nsel, dx, lddx, dw_sel, db_sel, ws, ws_bytes, B, Cin, V, accumulate, 0, dtype, stream);
}

extern "C" int dgtta_seghead_bwd_acc(const void *x, int ldx, const float *dout, int lddo, const float *w, const int *sel,
                                     int nsel, void *dx, int lddx, float *dw_sel, float *db_sel, void *ws, size_t ws_bytes,
                                     int B, int Cin, int64_t V, int accumulate, int accumulate_dx, int dtype, void *stream) {
  return seghead_bwd(x, ldx, dout, lddo, w, sel, nsel, dx, lddx, dw_sel, db_sel, ws, ws_bytes, B, Cin, V, accumulate, accumulate_dx,
                     dtype, stream);
}
