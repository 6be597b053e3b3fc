// InstanceNorm3d + LeakyReLU forward / backward (product kernels, HBM bound, VALU) and the per-channel reductions
// they share with the conv layers: InstanceNorm statistics, InstanceNorm backward sums, bias gradients.
// Semantics follow torch.nn.{InstanceNorm3d, LeakyReLU} as used by nnUNet's PlainConvUNet.
#include "conv_api.h"
#include "gfx950.h"
#include "instnorm_math.h"

namespace {

// ============================================================================ per-channel reductions over rows
// rows = voxels of one batch sample; MODE 0: (sum y, sum y^2)          [InstanceNorm statistics]
//                                     MODE 1: (sum da, sum da*xhat)     [InstanceNorm backward]; da = gz*lrelu'(a)
//                                     MODE 2: (sum y, 0)                [bias gradient]
// grid (nblk, B); partial[b][blk][c][2] double; the finalize kernels sum blocks in fixed order.
template <typename T, int MODE>
__global__ __launch_bounds__(256) void chan_reduce_kernel(const T *__restrict__ y, int ldy, const T *__restrict__ gz,
                                                          int ldgz, const float *__restrict__ mean_rstd,
                                                          const float *__restrict__ gamma,
                                                          const float *__restrict__ beta, float slope,
                                                          double *__restrict__ partial, int C, int64_t V) {
  __shared__ float red[2][256];
  const int b = blockIdx.y;
  int CL = 1;
  while (CL < C && CL < 64) CL <<= 1;  // channel lanes (power of two <= 64)
  const int RG = 256 / CL;             // row groups
  const int cl = threadIdx.x % CL, rg = threadIdx.x / CL;
  const int64_t rows_per_blk = cdiv64(V, gridDim.x);
  const int64_t r0 = (int64_t)blockIdx.x * rows_per_blk, r1 = (r0 + rows_per_blk < V) ? r0 + rows_per_blk : V;
  for (int c0 = 0; c0 < C; c0 += CL) {
    const int c = c0 + cl;
    float s0 = 0.f, s1 = 0.f;
    if (c < C) {
      float mu = 0.f, rs = 0.f, ga = 0.f, be = 0.f;
      if (MODE == 1) {
        mu = mean_rstd[((int64_t)b * C + c) * 2];
        rs = mean_rstd[((int64_t)b * C + c) * 2 + 1];
        ga = gamma[c];
        be = beta[c];
      }
      for (int64_t r = r0 + rg; r < r1; r += RG) {
        const float v = ld_f<T>(y + ((int64_t)b * V + r) * ldy + c);
        if (MODE == 0) {
          s0 += v;
          s1 += v * v;
        } else if (MODE == 2) {
          s0 += v;
        } else {
          const float xh = in_xhat(v, mu, rs);
          const float da = in_da(in_act(xh, ga, be), ld_f<T>(gz + ((int64_t)b * V + r) * ldgz + c), slope);
          s0 += da;
          s1 += da * xh;
        }
      }
    }
    __syncthreads();
    red[0][threadIdx.x] = s0;
    red[1][threadIdx.x] = s1;
    __syncthreads();
    if (rg == 0 && c < C) {
      double t0 = 0.0, t1 = 0.0;
      for (int k = 0; k < RG; ++k) {
        t0 += (double)red[0][k * CL + cl];
        t1 += (double)red[1][k * CL + cl];
      }
      double *p = partial + ((((int64_t)b * gridDim.x + blockIdx.x) * C) + c) * 2;
      p[0] = t0;
      p[1] = t1;
    }
  }
}

// 16-byte vectorised variant of chan_reduce_kernel (needs C, ld multiples of EPV = 16/sizeof(T) and aligned rows):
// a thread owns EPV consecutive channels, 256/G rows are in flight per iteration (G = C/EPV), two rows per thread and
// iteration for memory-level parallelism.  Same partial layout [b][blk][c][2] (double).
template <typename T>
struct VecOf {
  static constexpr int EPV = 16 / sizeof(T);
};

template <typename T, int MODE>
__global__ __launch_bounds__(256) void chan_reduce_vec_kernel(const T *__restrict__ y, int ldy, const T *__restrict__ gz,
                                                              int ldgz, const float *__restrict__ mean_rstd,
                                                              const float *__restrict__ gamma,
                                                              const float *__restrict__ beta, float slope,
                                                              double *__restrict__ partial, int C, int64_t V) {
  constexpr int EPV = VecOf<T>::EPV;
  extern __shared__ float sred[];          // [rpi][C][2]
  const int b = blockIdx.y;
  const int G = C / EPV, rpi = 256 / G;
  const int cg = threadIdx.x % G, rg = threadIdx.x / G;
  const bool active = rg < rpi;
  // rows are dealt to the workgroups in turn, 2 rpi at a time (round 4): with one contiguous chunk of V / gridDim.x rows
  // per workgroup the workgroups in flight read addresses a fixed 256 KiB (128^3 x 32 channels) apart - a few HBM channels
  // at a time, 3.1-3.8 TB/s where the apply passes, which walk the tensor in this interleaved order, stream at 5
  const int64_t r1 = V;
  float s0[EPV], s1[EPV], mu[EPV], rs[EPV], ga[EPV], be[EPV];
#pragma unroll
  for (int e = 0; e < EPV; ++e) {
    s0[e] = s1[e] = 0.f;
    mu[e] = rs[e] = ga[e] = be[e] = 0.f;
    if (MODE == 1 && active) {
      const int c = cg * EPV + e;
      mu[e] = mean_rstd[((int64_t)b * C + c) * 2];
      rs[e] = mean_rstd[((int64_t)b * C + c) * 2 + 1];
      ga[e] = gamma[c];
      be[e] = beta[c];
    }
  }
  if (active) {
    const T *yb = y + (int64_t)b * V * ldy + cg * EPV;
    const T *gb = (MODE == 1) ? gz + (int64_t)b * V * ldgz + cg * EPV : nullptr;
    for (int64_t r = (int64_t)blockIdx.x * (2 * rpi) + rg; r < r1; r += (int64_t)gridDim.x * (2 * rpi)) {
      const bool two = r + rpi < r1;
      // streaming loads, as in the apply passes (the tensors are far larger than the caches and are read once per pass)
      uint4 v0 = ld16_nt(yb + r * ldy), v1 = make_uint4(0, 0, 0, 0);
      uint4 g0 = make_uint4(0, 0, 0, 0), g1 = g0;
      if (two) v1 = ld16_nt(yb + (r + rpi) * ldy);
      if (MODE == 1) {
        g0 = ld16_nt(gb + r * ldgz);
        if (two) g1 = ld16_nt(gb + (r + rpi) * ldgz);
      }
#pragma unroll
      for (int k = 0; k < 2; ++k) {
        if (k == 1 && !two) break;
        float f[EPV], g[EPV];
        unpack16<T>(k ? v1 : v0, f);
        if (MODE == 1) unpack16<T>(k ? g1 : g0, g);
#pragma unroll
        for (int e = 0; e < EPV; ++e) {
          if (MODE == 0) {
            s0[e] += f[e];
            s1[e] += f[e] * f[e];
          } else if (MODE == 2) {
            s0[e] += f[e];
          } else {
            const float xh = in_xhat(f[e], mu[e], rs[e]);
            const float da = in_da(in_act(xh, ga[e], be[e]), g[e], slope);
            s0[e] += da;
            s1[e] += da * xh;
          }
        }
      }
    }
#pragma unroll
    for (int e = 0; e < EPV; ++e) {
      sred[((rg * C) + cg * EPV + e) * 2 + 0] = s0[e];
      sred[((rg * C) + cg * EPV + e) * 2 + 1] = s1[e];
    }
  }
  __syncthreads();
  for (int c = threadIdx.x; c < C; c += 256) {
    double t0 = 0.0, t1 = 0.0;
    for (int k = 0; k < rpi; ++k) {
      t0 += (double)sred[(k * C + c) * 2];
      t1 += (double)sred[(k * C + c) * 2 + 1];
    }
    double *p = partial + ((((int64_t)b * gridDim.x + blockIdx.x) * C) + c) * 2;
    p[0] = t0;
    p[1] = t1;
  }
}

template <typename T>
static bool vec_ok(const void *p, int ld, int C) {
  constexpr int EPV = 16 / sizeof(T);
  return p && ((uintptr_t)p & 15) == 0 && ld % EPV == 0 && C % EPV == 0 && C / EPV <= 256;
}

// launches the vectorised reduction when the operands allow it, else the scalar kernel
template <typename T, int MODE>
static void launch_chan_reduce(const void *y, int ldy, const void *gz, int ldgz, const float *mean_rstd,
                               const float *gamma, const float *beta, float slope, double *partial, int nblk, int B, int C,
                               int64_t V, hipStream_t st) {
  if (vec_ok<T>(y, ldy, C) && (MODE != 1 || vec_ok<T>(gz, ldgz, C))) {
    constexpr int EPV = 16 / sizeof(T);
    const int rpi = 256 / (C / EPV);
    hipLaunchKernelGGL((chan_reduce_vec_kernel<T, MODE>), dim3(nblk, B), dim3(256), (size_t)rpi * C * 2 * sizeof(float), st,
                       (const T *)y, ldy, (const T *)gz, ldgz, mean_rstd, gamma, beta, slope, partial, C, V);
  } else {
    hipLaunchKernelGGL((chan_reduce_kernel<T, MODE>), dim3(nblk, B), dim3(256), 0, st, (const T *)y, ldy, (const T *)gz,
                       ldgz, mean_rstd, gamma, beta, slope, partial, C, V);
  }
}

// 16-byte vectorised InstanceNorm+LeakyReLU apply kernels (forward MODE 0, backward MODE 1): grid (blocks, B); the
// per-channel constants of sample b are staged in LDS once per workgroup; each thread streams 16-byte channel groups.
// Same arithmetic as in_lrelu_apply_kernel / in_lrelu_bwd_apply_kernel.
// one element from its channel's staged constants k: forward (alpha, beta'), backward (mu, rs, ga, be, c1, c2)
template <int MODE>
__device__ __forceinline__ float in_apply_elem(float y, float gz, const float *k, float slope) {
  if (MODE == 0) return in_fwd(y, k[0], k[1], slope);
  const float xh = in_xhat(y, k[0], k[1]);
  return in_dy(in_da(in_act(xh, k[2], k[3]), gz, slope), xh, k[2], k[1], k[4], k[5]);
}

template <typename T, int MODE>
__global__ __launch_bounds__(256) void in_apply_vec_kernel(const T *__restrict__ y, int ldy, const T *__restrict__ gz,
                                                           int ldgz, const float *__restrict__ mean_rstd,
                                                           const float *__restrict__ gamma,
                                                           const float *__restrict__ beta, const float *__restrict__ c12,
                                                           T *__restrict__ out, int ldo, int C, int64_t V, float slope,
                                                           int nt) {
  constexpr int EPV = 16 / sizeof(T);
  extern __shared__ float sc[];     // fwd: [C][2] (alpha, beta'); bwd: [C][6] (mu, rs, ga, be, c1, c2)
  const int b = blockIdx.y;
  constexpr int NK = MODE == 0 ? 2 : 6;
  for (int c = threadIdx.x; c < C; c += 256) {
    const float mu = mean_rstd[((int64_t)b * C + c) * 2], rs = mean_rstd[((int64_t)b * C + c) * 2 + 1];
    if (MODE == 0) {
      const float al = in_alpha(rs, gamma[c]);
      sc[c * NK] = al;
      sc[c * NK + 1] = in_beta(beta[c], mu, al);
    } else {
      sc[c * NK] = mu;
      sc[c * NK + 1] = rs;
      sc[c * NK + 2] = gamma[c];
      sc[c * NK + 3] = beta[c];
      sc[c * NK + 4] = c12[((int64_t)b * C + c) * 2];
      sc[c * NK + 5] = c12[((int64_t)b * C + c) * 2 + 1];
    }
  }
  __syncthreads();
  const int G = C / EPV;
  const int64_t items = V * G;
  const T *yb = y + (int64_t)b * V * ldy;
  const T *gb = MODE == 1 ? gz + (int64_t)b * V * ldgz : nullptr;
  T *ob = out + (int64_t)b * V * ldo;
  if (256 % G == 0) {
    // fast path (G = 4, 8, 16, 32: every layer except the 320-channel bottleneck): a thread keeps ONE channel group for the
    // whole launch, so its per-channel constants sit in registers (no LDS read per element, no 64-bit division per item),
    // and two rows are in flight per iteration
    const int c0 = (threadIdx.x % G) * EPV;
    float kc[EPV][NK];
#pragma unroll
    for (int e = 0; e < EPV; ++e)
#pragma unroll
      for (int q = 0; q < NK; ++q) kc[e][q] = sc[(c0 + e) * NK + q];
    const int rpb = 256 / G;                                             // rows per workgroup per step
    const int64_t rstep = (int64_t)gridDim.x * rpb;
    auto one = [&](const uint4 &yv, const uint4 &gv, int64_t row) {
      float f[EPV], g[EPV], o[EPV];
      unpack16<T>(yv, f);
      if (MODE == 1) unpack16<T>(gv, g);
#pragma unroll
      for (int e = 0; e < EPV; ++e) o[e] = in_apply_elem<MODE>(f[e], MODE == 1 ? g[e] : 0.f, kc[e], slope);
      const uint4 pk = pack16<T>(o);
      if (nt) st16_nt(ob + row * ldo + c0, pk);
      else *reinterpret_cast<uint4 *>(ob + row * ldo + c0) = pk;
    };
    auto ld = [&](const T *p) {
      if (nt) return ld16_nt(p);
      return *reinterpret_cast<const uint4 *>(p);
    };
    for (int64_t row = (int64_t)blockIdx.x * rpb + threadIdx.x / G; row < V; row += 2 * rstep) {
      const int64_t row2 = row + rstep;
      const bool two = row2 < V;
      const uint4 y0 = ld(yb + row * ldy + c0);
      uint4 y1 = y0, g0 = y0, g1 = y0;
      if (two) y1 = ld(yb + row2 * ldy + c0);
      if (MODE == 1) {
        g0 = ld(gb + row * ldgz + c0);
        if (two) g1 = ld(gb + row2 * ldgz + c0);
      }
      one(y0, g0, row);
      if (two) one(y1, g1, row2);
    }
    return;
  }
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < items; i += (int64_t)gridDim.x * 256) {
    const int64_t row = i / G;
    const int c0 = (int)(i % G) * EPV;
    float f[EPV], g[EPV], o[EPV];
    unpack16<T>(*reinterpret_cast<const uint4 *>(yb + row * ldy + c0), f);
    if (MODE == 1) unpack16<T>(*reinterpret_cast<const uint4 *>(gb + row * ldgz + c0), g);
#pragma unroll
    for (int e = 0; e < EPV; ++e) o[e] = in_apply_elem<MODE>(f[e], MODE == 1 ? g[e] : 0.f, sc + (c0 + e) * NK, slope);
    *reinterpret_cast<uint4 *>(ob + row * ldo + c0) = pack16<T>(o);
  }
}

// sum of two doubles over a 256-thread workgroup (fixed order: lanes by butterfly, then waves 0..3); result in all threads
__device__ __forceinline__ void block_sum2_d(double &a, double &b, double *red /* >= 8 doubles of LDS */) {
  a = wave_sum_d(a);
  b = wave_sum_d(b);
  const int w = threadIdx.x >> 6;
  __syncthreads();
  if ((threadIdx.x & 63) == 0) {
    red[2 * w] = a;
    red[2 * w + 1] = b;
  }
  __syncthreads();
  a = (red[0] + red[2]) + (red[4] + red[6]);
  b = (red[1] + red[3]) + (red[5] + red[7]);
}


// InstanceNorm statistics finalize: mean, rstd = 1/sqrt(biased var + eps).  One 256-thread workgroup per (b,c); the number of
// partial blocks is read from the device-side header when hdr != NULL (statistics produced by the conv epilogue).
__global__ void in_stats_finalize_kernel(const double *__restrict__ partial, const long long *__restrict__ hdr, int nblk_h,
                                         int B, int C, int64_t V, float eps, float *__restrict__ mean_rstd) {
  const int i = blockIdx.x;
  const int b = i / C, c = i % C;
  const int nblk = hdr ? (int)hdr[0] : nblk_h;
  __shared__ double red[8];
  double s = 0.0, ss = 0.0;
  for (int k = threadIdx.x; k < nblk; k += 256) {
    const double2 v = *reinterpret_cast<const double2 *>(partial + ((((int64_t)b * nblk + k) * C) + c) * 2);
    s += v.x;
    ss += v.y;
  }
  block_sum2_d(s, ss, red);
  if (threadIdx.x == 0) {
    const double mean = s / (double)V;
    double var = ss / (double)V - mean * mean;
    // one voxel per sample: the variance is 0 by definition, where the one-pass form is left with the fp32 rounding of
    // y^2 (up to 2^-24 y^2 against eps: rstd 1.3 % low at |y| = 1.7 with fp32 storage, whose squares are not exact)
    if (var < 0.0 || V == 1) var = 0.0;
    mean_rstd[2 * i] = (float)mean;
    mean_rstd[2 * i + 1] = (float)(1.0 / sqrt(var + (double)eps));
  }
}

// z = lrelu(y*alpha + beta'), alpha = rstd*gamma, beta' = beta - mean*alpha  (ATen's batch_norm transform form)
template <typename T>
__global__ void in_lrelu_apply_kernel(const T *__restrict__ y, int ldy, const float *__restrict__ mean_rstd,
                                      const float *__restrict__ gamma, const float *__restrict__ beta,
                                      T *__restrict__ z, int ldz, int C, int64_t V, float slope, int64_t total) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % C);
    const int64_t row = i / C;  // b*V + v
    const int b = (int)(row / V);
    const float mu = mean_rstd[((int64_t)b * C + c) * 2], rs = mean_rstd[((int64_t)b * C + c) * 2 + 1];
    const float al = in_alpha(rs, gamma[c]);
    const float bt = in_beta(beta[c], mu, al);
    const float v = ld_f<T>(y + row * ldy + c);
    st_f<T>(z + row * ldz + c, in_fwd(v, al, bt, slope));
  }
}

// backward finalize: c1 = mean(da), c2 = mean(da*xhat); dgamma (+)= sum_b sum(da*xhat); dbeta (+)= sum_b sum(da).
// one 256-thread workgroup per channel; the number of partial blocks is read from the device-side header when hdr != NULL.
// mean_rstd != NULL: the partials are the (sum g', sum g' y) the data-gradient kernel left (conv_rows.hip / conv_ring.hip, GST) per
// (sample, tile), in the layout of the forward statistics (header = tiles per sample); sum g' xhat = rstd (sum g' y - mean sum g').
__global__ void in_bwd_finalize_kernel(const double *__restrict__ partial, const long long *__restrict__ hdr, int nblk_h, int B,
                                       int C, int64_t V, const float *__restrict__ mean_rstd, float *__restrict__ c12,
                                       float *__restrict__ dgamma, float *__restrict__ dbeta, int accumulate) {
  const int c = blockIdx.x;
  const int nblk = hdr ? (int)hdr[0] : nblk_h;
  __shared__ double red[8];
  double g_acc = 0.0, b_acc = 0.0;
  for (int b = 0; b < B; ++b) {
    double s0 = 0.0, s1 = 0.0;
    for (int k = threadIdx.x; k < nblk; k += 256) {
      const double2 v = *reinterpret_cast<const double2 *>(partial + ((((int64_t)b * nblk + k) * C) + c) * 2);
      s0 += v.x;
      s1 += v.y;
    }
    block_sum2_d(s0, s1, red);
    if (mean_rstd) {
      const double mu = (double)mean_rstd[((int64_t)b * C + c) * 2], rs = (double)mean_rstd[((int64_t)b * C + c) * 2 + 1];
      s1 = rs * (s1 - mu * s0);
    }
    if (threadIdx.x == 0) {
      c12[((int64_t)b * C + c) * 2] = (float)(s0 / (double)V);
      c12[((int64_t)b * C + c) * 2 + 1] = (float)(s1 / (double)V);
    }
    b_acc += s0;
    g_acc += s1;
  }
  if (threadIdx.x == 0) {
    dgamma[c] = accumulate ? dgamma[c] + (float)g_acc : (float)g_acc;
    dbeta[c] = accumulate ? dbeta[c] + (float)b_acc : (float)b_acc;
  }
}

// dy = gamma*rstd*(da - c1 - xhat*c2)
template <typename T>
__global__ void in_lrelu_bwd_apply_kernel(const T *__restrict__ gz, int ldgz, const T *__restrict__ y, int ldy,
                                          const float *__restrict__ mean_rstd, const float *__restrict__ gamma,
                                          const float *__restrict__ beta, const float *__restrict__ c12,
                                          T *__restrict__ dy, int lddy, int C, int64_t V, float slope, int64_t total) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % C);
    const int64_t row = i / C;
    const int b = (int)(row / V);
    const int64_t bc = (int64_t)b * C + c;
    const float mu = mean_rstd[bc * 2], rs = mean_rstd[bc * 2 + 1], ga = gamma[c];
    const float xh = in_xhat(ld_f<T>(y + row * ldy + c), mu, rs);
    const float da = in_da(in_act(xh, ga, beta[c]), ld_f<T>(gz + row * ldgz + c), slope);
    st_f<T>(dy + row * lddy + c, in_dy(da, xh, ga, rs, c12[bc * 2], c12[bc * 2 + 1]));
  }
}

__global__ void bias_finalize_kernel(const double *__restrict__ partial, int nblk, int B, int C, float *__restrict__ db,
                                     int accumulate) {
  const int c = blockIdx.x;   // one wave per channel
  double s = 0.0;
  for (int k = threadIdx.x; k < B * nblk; k += 64) s += partial[(((int64_t)k * C) + c) * 2];
  s = wave_sum_d(s);
  if (threadIdx.x == 0) db[c] = accumulate ? db[c] + (float)s : (float)s;
}

// ============================================================================ backward of the block in front of the head
// gz of that block is W^T d16: a linear function of the gathered logit gradient the fused head + warp backward leaves (rows of 16
// values in the storage type, half the bytes of a gz row).  Both passes of the backward rebuild it instead of loading it:
// gz[c] = sum_k W[sel[k]][c] * float(d16[k]) on the fp32 matrix cores (v_mfma_f32_16x16x4_f32, exact fp32 products and sums), used
// unrounded where the passes above use the loaded gz.  32 channels, 16 classes, 16-bit storage.
// A wave takes 16 rows at a time: lane l has row l & 15 and channels 8 g .. 8 g + 7 (g = l >> 4) - the 16-byte reads of y of the
// passes above, dealt to the lanes row-minor.  B operand: the lane's 8 bytes of its d16 row, classes 4 g + s in step s.  A
// operand: 8 weight registers, W[sel[4 g + s]][ch(l & 15)], where matrix row m stands for channel 8 (m >> 2) + (m & 3) in the
// first accumulator and 4 more in the second - so that D leaves exactly the lane's 8 channels on it.  Sum order per channel:
// steps s = 0..3, the four classes {s, 4 + s, 8 + s, 12 + s} inside one instruction.
// APPLY 0: partial[b][blk][c][2] = (sum da, sum da * xhat) as chan_reduce_vec_kernel<T, 1>; APPLY 1: dy as in_apply_vec_kernel<T, 1>.
constexpr int INH_C = 32, INH_NS = 16;

template <typename T, int APPLY>
__global__ __launch_bounds__(256) void in_bwd_head_kernel(const T *__restrict__ y, int ldy, const unsigned short *__restrict__ d16,
                                                          const float *__restrict__ w, const int *__restrict__ sel,
                                                          const float *__restrict__ mean_rstd, const float *__restrict__ gamma,
                                                          const float *__restrict__ beta, const float *__restrict__ c12,
                                                          float slope, double *__restrict__ partial, T *__restrict__ dy,
                                                          int lddy, int64_t V, int nt) {
  __shared__ float sred[APPLY ? 1 : 64 * INH_C * 2];      // [wave * 16 + row lane][c][2]
  const int b = blockIdx.y;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n = lane & 15, g = lane >> 4;
  float wa0[4], wa1[4];
  {
    const int ch = 8 * (n >> 2) + (n & 3);
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      const int k = 4 * g + s;
      const float *wr = w + (int64_t)(sel ? sel[k] : k) * INH_C + ch;
      wa0[s] = wr[0];
      wa1[s] = wr[4];
    }
  }
  float mu[8], rs[8], ga[8], be[8], k1[8], k2[8], s0[8], s1[8];
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    const int c = 8 * g + e;
    mu[e] = mean_rstd[((int64_t)b * INH_C + c) * 2];
    rs[e] = mean_rstd[((int64_t)b * INH_C + c) * 2 + 1];
    ga[e] = gamma[c];
    be[e] = beta[c];
    k1[e] = APPLY ? c12[((int64_t)b * INH_C + c) * 2] : 0.f;
    k2[e] = APPLY ? c12[((int64_t)b * INH_C + c) * 2 + 1] : 0.f;
    s0[e] = s1[e] = 0.f;
  }
  const T *yb = y + (int64_t)b * V * ldy + 8 * g;
  const unsigned short *db = d16 + (int64_t)b * V * INH_NS + 4 * g;
  T *ob = APPLY ? dy + (int64_t)b * V * lddy + 8 * g : nullptr;
  // W^T d of the lane's row and channels from its 8 bytes of d16 (every lane of the wave takes part: zeros for a row past V)
  auto gz_of = [&](const uint2 &dv, float *gz) {
    float d[4];
    unpack2_16<T>(dv.x, d[0], d[1]);
    unpack2_16<T>(dv.y, d[2], d[3]);
    f32x4_t a0 = {0.f, 0.f, 0.f, 0.f}, a1 = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < 4; ++s) {
      a0 = __builtin_amdgcn_mfma_f32_16x16x4f32(wa0[s], d[s], a0, 0, 0, 0);
      a1 = __builtin_amdgcn_mfma_f32_16x16x4f32(wa1[s], d[s], a1, 0, 0, 0);
    }
#pragma unroll
    for (int e = 0; e < 4; ++e) gz[e] = a0[e], gz[4 + e] = a1[e];
  };
  auto one = [&](const uint4 &yv, const uint2 &dv, int64_t row) {
    float f[8], gz[8], o[8];
    unpack16<T>(yv, f);
    gz_of(dv, gz);
    if (row >= V) return;
#pragma unroll
    for (int e = 0; e < 8; ++e) {
      const float xh = in_xhat(f[e], mu[e], rs[e]);
      const float gg = in_da(in_act(xh, ga[e], be[e]), gz[e], slope);
      if (APPLY) {
        o[e] = in_dy(gg, xh, ga[e], rs[e], k1[e], k2[e]);
      } else {
        s0[e] += gg;
        s1[e] += gg * xh;
      }
    }
    if (APPLY) {
      const uint4 pk = pack16<T>(o);
      if (nt) st16_nt(ob + row * lddy, pk);
      else *reinterpret_cast<uint4 *>(ob + row * lddy) = pk;
    }
  };
  // units of 16 rows are dealt to the waves of the grid in turn (the interleaved order of the passes above), two in flight
  // (four in flight: 132-140 registers, 3 waves per SIMD instead of 4, and 4 % slower - profiles/in_bwd_level0_ab.txt)
  const int64_t ustep = (int64_t)gridDim.x * 4;
  for (int64_t u = (int64_t)blockIdx.x * 4 + wave; u * 16 < V; u += 2 * ustep) {      // (wave-uniform)
    const int64_t r0 = u * 16 + n, r1 = (u + ustep) * 16 + n;
    const bool two = (u + ustep) * 16 < V;                                            // (wave-uniform)
    const uint4 zero4 = make_uint4(0, 0, 0, 0);
    const uint2 zero2 = make_uint2(0, 0);
    uint4 y0 = zero4, y1 = zero4;
    uint2 d0 = zero2, d1 = zero2;
    if (r0 < V) {
      y0 = ld16_nt(yb + r0 * ldy);
      d0 = ld8_nt(db + r0 * INH_NS);
    }
    if (two && r1 < V) {
      y1 = ld16_nt(yb + r1 * ldy);
      d1 = ld8_nt(db + r1 * INH_NS);
    }
    one(y0, d0, r0);
    if (two) one(y1, d1, r1);
  }
  if (APPLY) return;
#pragma unroll
  for (int e = 0; e < 8; ++e) {
    sred[((wave * 16 + n) * INH_C + 8 * g + e) * 2 + 0] = s0[e];
    sred[((wave * 16 + n) * INH_C + 8 * g + e) * 2 + 1] = s1[e];
  }
  __syncthreads();
  if (threadIdx.x < INH_C) {
    const int c = threadIdx.x;
    double t0 = 0.0, t1 = 0.0;
    for (int k = 0; k < 64; ++k) {
      t0 += (double)sred[(k * INH_C + c) * 2];
      t1 += (double)sred[(k * INH_C + c) * 2 + 1];
    }
    double *p = partial + ((((int64_t)b * gridDim.x + blockIdx.x) * INH_C) + c) * 2;
    p[0] = t0;
    p[1] = t1;
  }
}

}  // namespace

__global__ void set_header_kernel(long long *hdr, long long v) { hdr[0] = v; }

// InstanceNorm statistics of y by a separate reduction pass, in the buffer layout of the conv epilogues
// (dgtta_conv3d_stats_bytes): what the general forward kernel (conv_ref.hip), which has no such epilogue, is followed by
int conv_stats_ref(const void *y, int ldy, void *stats, int B, int C, int64_t V, int dtype, hipStream_t st) {
  const int nblk = reduce_blocks(V, B);
  hipLaunchKernelGGL(set_header_kernel, dim3(1), dim3(1), 0, st, (long long *)stats, (long long)nblk);
  DISPATCH_T(dtype, hipLaunchKernelGGL((chan_reduce_kernel<T, 0>), dim3(nblk, B), dim3(256), 0, st, (const T *)y, ldy,
                                       (const T *)nullptr, 0, nullptr, nullptr, nullptr, 0.f, (double *)stats + 32,
                                       C, V));
  DG_CHECK_LAUNCH("chan_reduce_kernel<0>");
  return DGTTA_OK;
}

// bias gradient: db[c] (+)= sum over B x V rows of dy, fixed order; ws = conv_bias_grad_ws_bytes
size_t conv_bias_grad_ws_bytes(int B, int C, int64_t V) {
  if (B <= 0 || C <= 0 || V <= 0) return 0;
  return (size_t)B * reduce_blocks(V, B) * C * 2 * sizeof(double);
}
int conv_bias_grad(const void *dy, int lddy, float *db, void *ws, int B, int C, int64_t V, int accumulate, int dtype, hipStream_t st) {
  const int nblk = reduce_blocks(V, B);
  double *partial = (double *)ws;
  DISPATCH_T(dtype, (launch_chan_reduce<T, 2>(dy, lddy, nullptr, 0, nullptr, nullptr, nullptr, 0.f, partial, nblk, B, C, V, st)));
  DG_CHECK_LAUNCH("chan_reduce_kernel<2>");
  hipLaunchKernelGGL(bias_finalize_kernel, dim3(C), dim3(64), 0, st, partial, nblk, B, C, db, accumulate);
  DG_CHECK_LAUNCH("bias_finalize_kernel");
  return DGTTA_OK;
}

// ============================================================================ InstanceNorm + LeakyReLU launchers
// Their workspace, [partial | c12]: the partial sums of the reduction pass (double) and the backward's (c1, c2) per (sample,
// channel), each region a multiple of 256 bytes.  The size query returns total(), the launchers carve their pointers with the
// accessors: one layout serves both.
struct InWsLayout {
  size_t partial, c12;
  size_t total() const { return partial + c12; }
  double *partial_of(void *ws) const { return (double *)ws; }
  float *c12_of(void *ws) const { return (float *)((char *)ws + partial); }
};
static InWsLayout in_ws_layout(int B, int C, int64_t V) {
  return {align_up((size_t)B * reduce_blocks(V, B) * C * 2 * sizeof(double), 256), align_up((size_t)B * C * 2 * sizeof(float), 256)};
}

extern "C" size_t dgtta_instnorm_ws_bytes(int B, int C, int64_t V) {
  if (B <= 0 || C <= 0 || V <= 0) return 0;      // a size query of an empty problem (the launchers reject it with DGTTA_ERR_BADARG)
  return in_ws_layout(B, C, V).total();
}

// in_apply_vec_kernel takes whole 16-byte channel groups of 16-byte aligned rows, of every operand of the pass (the forward has
// no gz: NULL, 0); its grid is one workgroup per 1024 groups of a sample, at most 4096
static bool apply_vec_ok(int epv, int C, const void *y, int ldy, const void *gz, int ldgz, const void *out, int ldo) {
  auto ok = [&](const void *p, int ld) { return ld % epv == 0 && !((uintptr_t)p & 15); };
  return C % epv == 0 && ok(y, ldy) && ok(gz, ldgz) && ok(out, ldo) && C <= 2048;
}
static int apply_vec_blocks(int epv, int C, int64_t V) {
  const int64_t n = cdiv64(V * (C / epv), 256 * 4);
  return (int)(n < 4096 ? (n > 0 ? n : 1) : 4096);
}

// the apply pass of the forward (MODE 0: out = z; gz = c12 = NULL) or of the backward (MODE 1: out = dy): the 16-byte kernel
// where the operands allow it, else the scalar one
template <int MODE>
static int launch_in_apply(const void *y, int ldy, const void *gz, int ldgz, const float *mean_rstd, const float *gamma,
                           const float *beta, const float *c12, void *out, int ldo, int B, int C, int64_t V, float slope,
                           int dtype, hipStream_t st) {
  const int epv = 16 / (int)esize(dtype);
  if (apply_vec_ok(epv, C, y, ldy, gz, ldgz, out, ldo)) {
    DISPATCH_T(dtype, hipLaunchKernelGGL((in_apply_vec_kernel<T, MODE>), dim3(apply_vec_blocks(epv, C, V), B), dim3(256),
                                         (size_t)C * (MODE == 0 ? 2 : 6) * 4, st, (const T *)y, ldy, (const T *)gz, ldgz,
                                         mean_rstd, gamma, beta, c12, (T *)out, ldo, C, V, slope,
                                         dgtta_switches().in_nt - '0'));
    DG_CHECK_LAUNCH(MODE == 0 ? "in_apply_vec_kernel<0>" : "in_apply_vec_kernel<1>");
    return DGTTA_OK;
  }
  const int64_t total = (int64_t)B * V * C;
  if (MODE == 0)
    DISPATCH_T(dtype, hipLaunchKernelGGL((in_lrelu_apply_kernel<T>), dim3(gs_blocks(total)), dim3(256), 0, st, (const T *)y,
                                         ldy, mean_rstd, gamma, beta, (T *)out, ldo, C, V, slope, total));
  else
    DISPATCH_T(dtype, hipLaunchKernelGGL((in_lrelu_bwd_apply_kernel<T>), dim3(gs_blocks(total)), dim3(256), 0, st,
                                         (const T *)gz, ldgz, (const T *)y, ldy, mean_rstd, gamma, beta, c12, (T *)out, ldo,
                                         C, V, slope, total));
  DG_CHECK_LAUNCH(MODE == 0 ? "in_lrelu_apply_kernel" : "in_lrelu_bwd_apply_kernel");
  return DGTTA_OK;
}

extern "C" int dgtta_instnorm_lrelu_fwd(const void *y, int ldy, const void *stats, const float *gamma, const float *beta,
                                        float *mean_rstd, void *z, int ldz, void *ws, size_t ws_bytes, int B, int C,
                                        int64_t V, float eps, float slope, int dtype, void *stream) {
  // z == NULL (round 5): the statistics only - the caller applies them itself (dgtta_feature_window_accumulate_norm)
  DG_REQUIRE(y && gamma && beta && mean_rstd && ws, DGTTA_ERR_BADARG, "instnorm_lrelu_fwd: null pointer");
  DG_REQUIRE(B > 0 && C > 0 && V > 0 && ldy >= C && (!z || ldz >= C), DGTTA_ERR_BADARG, "instnorm_lrelu_fwd: bad dims");
  DG_REQUIRE(ws_bytes >= dgtta_instnorm_ws_bytes(B, C, V), DGTTA_ERR_WORKSPACE, "instnorm_lrelu_fwd: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  const int nblk = reduce_blocks(V, B);
  if (stats) {   // partial sums came with the conv epilogue (header + partials)
    hipLaunchKernelGGL(in_stats_finalize_kernel, dim3(B * C), dim3(256), 0, st, (const double *)stats + 32,
                       (const long long *)stats, 0, B, C, V, eps, mean_rstd);
  } else {
    double *partial = in_ws_layout(B, C, V).partial_of(ws);
    DISPATCH_T(dtype, (launch_chan_reduce<T, 0>(y, ldy, nullptr, 0, nullptr, nullptr, nullptr, 0.f, partial, nblk, B, C, V, st)));
    DG_CHECK_LAUNCH("chan_reduce_kernel<0>");
    hipLaunchKernelGGL(in_stats_finalize_kernel, dim3(B * C), dim3(256), 0, st, (const double *)partial,
                       (const long long *)nullptr, nblk, B, C, V, eps, mean_rstd);
  }
  DG_CHECK_LAUNCH("in_stats_finalize_kernel");
  if (!z) return DGTTA_OK;
  return launch_in_apply<0>(y, ldy, nullptr, 0, mean_rstd, gamma, beta, nullptr, z, ldz, B, C, V, slope, dtype, st);
}

// gz of the block in front of the head, given as what it is a linear function of: gz = W^T d16 (in_bwd_head_kernel)
struct InBwdHead {
  const void *d16;
  const float *w;
  const int *sel;
};
// pass APPLY of in_bwd_head_kernel on `grid` workgroups per sample (16-bit storage: the entry point admits nothing else)
template <int APPLY>
static void launch_in_bwd_head(const InBwdHead &h, const void *y, int ldy, const float *mean_rstd, const float *gamma,
                               const float *beta, const float *c12, float slope, double *partial, void *dy, int lddy, int grid,
                               int B, int64_t V, int dtype, hipStream_t st) {
  auto go = [&](auto t) {
    typedef decltype(t) T;
    hipLaunchKernelGGL((in_bwd_head_kernel<T, APPLY>), dim3(grid, B), dim3(256), 0, st, (const T *)y, ldy,
                       (const unsigned short *)h.d16, h.w, h.sel, mean_rstd, gamma, beta, c12, slope, partial, (T *)dy, lddy, V,
                       dgtta_switches().in_nt - '0');
  };
  if (dtype == DGTTA_BF16) go(bf16_t{});
  else go(f16_t{});
}

// One InstanceNorm + LeakyReLU backward, arguments checked by the entry points: sums -> finalize -> apply.  The sums (sum da,
// sum da * xhat) per (sample, channel) come from a reduction pass over (y, gz); or, gstats != NULL, from the partials that the
// data-gradient kernel which produced gz left: no pass over y and gz; or, head != NULL, from a pass that rebuilds gz from the
// head's d16, as the apply then does too: gz is never stored.
static int instnorm_bwd_run(const void *gz, int ldgz, const InBwdHead *head, const void *gstats, const void *y, int ldy,
                            const float *gamma, const float *beta, const float *mean_rstd, void *dy, int lddy, float *dgamma,
                            float *dbeta, void *ws, int B, int C, int64_t V, float slope, int accumulate, int dtype,
                            hipStream_t st) {
  const InWsLayout lay = in_ws_layout(B, C, V);
  const int nblk = reduce_blocks(V, B);
  double *partial = lay.partial_of(ws);
  float *c12 = lay.c12_of(ws);
  if (head) {
    launch_in_bwd_head<0>(*head, y, ldy, mean_rstd, gamma, beta, nullptr, slope, partial, nullptr, 0, nblk, B, V, dtype, st);
    DG_CHECK_LAUNCH("in_bwd_head_kernel<0>");
  } else if (!gstats) {
    DISPATCH_T(dtype, (launch_chan_reduce<T, 1>(y, ldy, gz, ldgz, mean_rstd, gamma, beta, slope, partial, nblk, B, C, V, st)));
    DG_CHECK_LAUNCH("chan_reduce_kernel<1>");
  }
  // gstats: header + partials in the layout of the forward statistics, sums of g' y that the finalize converts with mean_rstd
  hipLaunchKernelGGL(in_bwd_finalize_kernel, dim3(C), dim3(256), 0, st, gstats ? (const double *)gstats + 32 : partial,
                     (const long long *)gstats, nblk, B, C, V, gstats ? mean_rstd : nullptr, c12, dgamma, dbeta, accumulate);
  DG_CHECK_LAUNCH("in_bwd_finalize_kernel");
  if (!head) return launch_in_apply<1>(y, ldy, gz, ldgz, mean_rstd, gamma, beta, c12, dy, lddy, B, C, V, slope, dtype, st);
  const int64_t units = cdiv64(V, 16);
  const int blocks = (int)(cdiv64(units, 4 * 4) < 4096 ? cdiv64(units, 4 * 4) : 4096);
  launch_in_bwd_head<1>(*head, y, ldy, mean_rstd, gamma, beta, c12, slope, nullptr, dy, lddy, blocks, B, V, dtype, st);
  DG_CHECK_LAUNCH("in_bwd_head_kernel<1>");
  return DGTTA_OK;
}

// the checks the two entry points that take a stored gz share
static int instnorm_bwd_stored(const void *gz, int ldgz, const void *y, int ldy, const float *gamma, const float *beta,
                               const float *mean_rstd, void *dy, int lddy, float *dgamma, float *dbeta, const void *gstats,
                               void *ws, size_t ws_bytes, int B, int C, int64_t V, float slope, int accumulate, int dtype,
                               void *stream, const char *name) {
  DG_REQUIRE(gz && y && gamma && beta && mean_rstd && dy && dgamma && dbeta && ws, DGTTA_ERR_BADARG, "%s: null pointer", name);
  DG_REQUIRE(B > 0 && C > 0 && V > 0 && ldy >= C && ldgz >= C && lddy >= C, DGTTA_ERR_BADARG, "%s: bad dims", name);
  DG_REQUIRE(ws_bytes >= dgtta_instnorm_ws_bytes(B, C, V), DGTTA_ERR_WORKSPACE, "%s: workspace too small", name);
  return instnorm_bwd_run(gz, ldgz, nullptr, gstats, y, ldy, gamma, beta, mean_rstd, dy, lddy, dgamma, dbeta, ws, B, C, V, slope,
                          accumulate, dtype, (hipStream_t)stream);
}

extern "C" int dgtta_instnorm_lrelu_bwd(const void *gz, int ldgz, const void *y, int ldy, const float *gamma,
                                        const float *beta, const float *mean_rstd, void *dy, int lddy, float *dgamma,
                                        float *dbeta, void *ws, size_t ws_bytes, int B, int C, int64_t V, float slope,
                                        int accumulate, int dtype, void *stream) {
  return instnorm_bwd_stored(gz, ldgz, y, ldy, gamma, beta, mean_rstd, dy, lddy, dgamma, dbeta, nullptr, ws, ws_bytes, B, C, V,
                             slope, accumulate, dtype, stream, "instnorm_lrelu_bwd");
}

extern "C" int dgtta_instnorm_lrelu_bwd_gstats(const void *gz, int ldgz, const void *y, int ldy, const float *gamma,
                                               const float *beta, const float *mean_rstd, void *dy, int lddy,
                                               float *dgamma, float *dbeta, const void *gstats, void *ws, size_t ws_bytes,
                                               int B, int C, int64_t V, float slope, int accumulate, int dtype,
                                               void *stream) {
  DG_REQUIRE(gstats, DGTTA_ERR_BADARG, "instnorm_lrelu_bwd_gstats: null statistics");
  return instnorm_bwd_stored(gz, ldgz, y, ldy, gamma, beta, mean_rstd, dy, lddy, dgamma, dbeta, gstats, ws, ws_bytes, B, C, V,
                             slope, accumulate, dtype, stream, "instnorm_lrelu_bwd_gstats");
}

// dgtta_instnorm_lrelu_bwd of the block in front of the head, its gz given as (d16, head weight rows, sel): gz = W^T d16 is
// rebuilt in both passes and never stored (in_bwd_head_kernel).  32 channels, 16 selected classes, 16-bit storage.
extern "C" int dgtta_instnorm_lrelu_bwd_head(const void *d16, const float *w, const int *sel, int nsel, const void *y, int ldy,
                                             const float *gamma, const float *beta, const float *mean_rstd, void *dy, int lddy,
                                             float *dgamma, float *dbeta, void *ws, size_t ws_bytes, int B, int C, int64_t V,
                                             float slope, int accumulate, int dtype, void *stream) {
  DG_REQUIRE(d16 && w && y && gamma && beta && mean_rstd && dy && dgamma && dbeta && ws, DGTTA_ERR_BADARG,
             "instnorm_lrelu_bwd_head: null pointer");
  DG_REQUIRE(B > 0 && V > 0 && ldy >= C && lddy >= C, DGTTA_ERR_BADARG, "instnorm_lrelu_bwd_head: bad dims");
  DG_REQUIRE(C == INH_C && nsel == INH_NS && (dtype == DGTTA_BF16 || dtype == DGTTA_F16), DGTTA_ERR_UNSUPPORTED,
             "instnorm_lrelu_bwd_head: built for 32 channels, 16 selected classes and 16-bit storage (C %d, nsel %d, dtype %d)", C,
             nsel, dtype);
  DG_REQUIRE(ldy % 8 == 0 && lddy % 8 == 0 && !((uintptr_t)y & 15) && !((uintptr_t)dy & 15) && !((uintptr_t)d16 & 15),
             DGTTA_ERR_BADARG, "instnorm_lrelu_bwd_head: unaligned operand");
  DG_REQUIRE(ws_bytes >= dgtta_instnorm_ws_bytes(B, C, V), DGTTA_ERR_WORKSPACE, "instnorm_lrelu_bwd_head: workspace too small");
  const InBwdHead head = {d16, w, sel};
  return instnorm_bwd_run(nullptr, 0, &head, nullptr, y, ldy, gamma, beta, mean_rstd, dy, lddy, dgamma, dbeta, ws, B, C, V, slope,
                          accumulate, dtype, (hipStream_t)stream);
}
