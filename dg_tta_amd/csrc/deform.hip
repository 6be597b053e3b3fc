// Deformable spatial augmentation (spatial_aug_type = "deformable"): what dg_tta/tta/augmentation_utils.py builds from
// torch calls - get_rf_field (:8-43), calc_consistent_diffeomorphic_field (:46-135, the inverse-consistent branch) - and the
// two F.grid_sample calls of calc_branch through the resulting dense grids (dg_tta/tta/tta.py:534-575).
//
//   rf_box_kernel     k^3 box filter (avg_pool3d, stride 1, zero padding counted in the divisor) on the low-resolution draw;
//                     three launches on ping-pong buffers of at most a few 10^4 values per plane
//   rf_stats_kernel   trilinear upsampling (align_corners=False) evaluated on the fly, per-plane sum / sum of squares in
//                     double, one partial per block (fixed order: bitwise reproducible)
//   rf_norm_kernel    the same upsampling again (the low-resolution plane lives in L1 / L2), (x - mean) / (1e-3 + std):
//                     the field is written once, 4 B / value, and never read back
//   diffeo_iter       one launch per fixed-point iteration, both fields: d' = d/2 - sample(i, id + d)/2 and
//                     i' = i/2 - sample(d, id + i)/2 (border, align_corners=True); 24 B read + 24 B written per voxel plus
//                     the gathers (neighbouring voxels: cache hits).  The first launch reads the NCDHW field, applies the
//                     pre-scaling and skips the gather from the all-zero inverse; the last one applies the post-scaling.
//                     Everything in between and the results are [N][D][H][W][3] rows, the layout the samplers read.
//   dense_warp_fwd    F.grid_sample(src, (0 * id + disp) + id, align_corners=False): 12 B of grid per voxel on top of the
//                     affine kernel's 2 * C * 4 B
//   dense_warp_bwd    its adjoint w.r.t. src: scatter-add with fp32 atomics, one lane per channel (the pre-image of a source
//                     voxel under a dense field has no closed form; with displacements of up to ~10 voxels at 128^3 a
//                     bounded-window gather would visit thousands of candidates).  Sums are order dependent in the last bits.
#include "common.h"
#include "sampler.h"

namespace {

constexpr int RF_STAT_BLOCKS = 64;   // partial sums per plane

// ------------------------------------------------------------------------------------------------ random field
__global__ __launch_bounds__(256) void rf_box_kernel(const float *__restrict__ in, float *__restrict__ out, int P, int Dl, int Hl,
                                                     int Wl, int k) {
  const int Vl = Dl * Hl * Wl, pad = k / 2;
  const float div = (float)(k * k * k);
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < P * Vl; i += gridDim.x * blockDim.x) {
    const int p = i / Vl, v = i - p * Vl;
    const int w = v % Wl, h = (v / Wl) % Hl, d = v / (Wl * Hl);
    const float *src = in + (size_t)p * Vl;
    float sum = 0.f;        // at::avg_pool3d: in-bounds taps in d, h, w order, then one division by the full window
    for (int z = max(d - pad, 0); z < min(d - pad + k, Dl); ++z)
      for (int y = max(h - pad, 0); y < min(h - pad + k, Hl); ++y)
        for (int x = max(w - pad, 0); x < min(w - pad + k, Wl); ++x) sum += src[(z * Hl + y) * Wl + x];
    out[i] = sum / div;
  }
}

struct Lin1 {
  int i0, i1;
  float l0, l1;
};
// at::native::compute_source_index_and_lambda (align_corners=False, size given: scale = in / out)
__device__ __forceinline__ Lin1 lin1(int o, int n_in, int n_out) {
  const float scale = (float)n_in / (float)n_out;
  const float real = fmaxf(scale * ((float)o + 0.5f) - 0.5f, 0.f);
  Lin1 r;
  r.i0 = min((int)real, n_in - 1);
  r.i1 = min(r.i0 + 1, n_in - 1);
  r.l1 = fminf(fmaxf(real - (float)r.i0, 0.f), 1.f);
  r.l0 = 1.f - r.l1;
  return r;
}

__device__ __forceinline__ float rf_upsample(const float *__restrict__ low, int Hl, int Wl, const Lin1 &a, const Lin1 &b,
                                             const Lin1 &c) {
  auto row = [&](int z, int y) { return c.l0 * low[(z * Hl + y) * Wl + c.i0] + c.l1 * low[(z * Hl + y) * Wl + c.i1]; };
  auto plane = [&](int z) { return b.l0 * row(z, b.i0) + b.l1 * row(z, b.i1); };
  return a.l0 * plane(a.i0) + a.l1 * plane(a.i1);
}

__device__ __forceinline__ double block_sum_d(double v, double *red) {
  v = wave_sum_d(v);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = (blockDim.x + 63) >> 6;
  __syncthreads();
  if (lane == 0) red[w] = v;
  __syncthreads();
  double r = 0.0;
  for (int i = 0; i < nw; ++i) r += red[i];
  return r;
}

// grid (RF_STAT_BLOCKS, P)
__global__ __launch_bounds__(256) void rf_stats_kernel(const float *__restrict__ low, double *__restrict__ partial, int Dl, int Hl,
                                                       int Wl, int D, int H, int W) {
  __shared__ double red[4];
  const int p = blockIdx.y;
  const float *src = low + (size_t)p * Dl * Hl * Wl;
  const int64_t V = (int64_t)D * H * W;
  double s = 0.0, s2 = 0.0;
  for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < V; v += (int64_t)gridDim.x * blockDim.x) {
    const int w = (int)(v % W), h = (int)((v / W) % H), d = (int)(v / ((int64_t)W * H));
    const float x = rf_upsample(src, Hl, Wl, lin1(d, Dl, D), lin1(h, Hl, H), lin1(w, Wl, W));
    s += (double)x;
    s2 += (double)x * (double)x;
  }
  s = block_sum_d(s, red);
  s2 = block_sum_d(s2, red);
  if (threadIdx.x == 0) {
    partial[((size_t)p * gridDim.x + blockIdx.x) * 2] = s;
    partial[((size_t)p * gridDim.x + blockIdx.x) * 2 + 1] = s2;
  }
}

// grid (blocks, P): field[p] = (x - mean) / (1e-3 + std), unbiased std
__global__ __launch_bounds__(256) void rf_norm_kernel(const float *__restrict__ low, const double *__restrict__ partial,
                                                      float *__restrict__ field, int Dl, int Hl, int Wl, int D, int H, int W) {
  const int p = blockIdx.y;
  const float *src = low + (size_t)p * Dl * Hl * Wl;
  const int64_t V = (int64_t)D * H * W;
  double s = 0.0, s2 = 0.0;
  for (int i = 0; i < RF_STAT_BLOCKS; ++i) {      // same order in every thread
    s += partial[((size_t)p * RF_STAT_BLOCKS + i) * 2];
    s2 += partial[((size_t)p * RF_STAT_BLOCKS + i) * 2 + 1];
  }
  const double mean = s / (double)V;
  const double var = V > 1 ? fmax(s2 - s * mean, 0.0) / (double)(V - 1) : 0.0;
  const float meanf = (float)mean, den = 1e-3f + (float)sqrt(var);
  float *dst = field + (size_t)p * V;
  for (int64_t v = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; v < V; v += (int64_t)gridDim.x * blockDim.x) {
    const int w = (int)(v % W), h = (int)((v / W) % H), d = (int)(v / ((int64_t)W * H));
    const float x = rf_upsample(src, Hl, Wl, lin1(d, Dl, D), lin1(h, Hl, H), lin1(w, Wl, W));
    dst[v] = (x - meanf) / den;
  }
}

// ------------------------------------------------------------------------------------------------ fixed-point iteration
// torch.linspace(-1, 1, n)[j]: the identity grid of F.affine_grid(eye, align_corners=True)
__device__ __forceinline__ float lin_coord(int j, int n) {
  if (n <= 1) return 0.f;
  const float step = 2.0f / (float)(n - 1);
  return (j < n / 2) ? (-1.0f + step * (float)j) : (1.0f - step * (float)(n - 1 - j));
}

struct PreScale {
  float factor, dim[3], pow2, dt;
  // (field * factor) / [D,H,W][c] / 2^steps * dt, in the reference's order of operations
  __device__ __forceinline__ float operator()(float f, int c) const { return (((f * factor) / dim[c]) / pow2) * dt; }
};

// F.grid_sample(src, grid, padding_mode="border", align_corners=True) of a 3-channel field at one position.
// FIRST: src is the NCDHW random field, pre-scaled as it is read; else [D][H][W][3] rows.
template <bool FIRST>
__device__ __forceinline__ void sample3(const float *__restrict__ src, const PreScale &pre, float gx, float gy, float gz, int D,
                                        int H, int W, float out[3]) {
  Sample s;
  s.ix = fminf((float)(W - 1), fmaxf(((gx + 1.0f) / 2.0f) * (float)(W - 1), 0.f));
  s.iy = fminf((float)(H - 1), fmaxf(((gy + 1.0f) / 2.0f) * (float)(H - 1), 0.f));
  s.iz = fminf((float)(D - 1), fmaxf(((gz + 1.0f) / 2.0f) * (float)(D - 1), 0.f));
  const Corners cr = corners(s);
  const int64_t V = (int64_t)D * H * W;
  out[0] = out[1] = out[2] = 0.f;
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    const int xx = cr.x0 + (k & 1), yy = cr.y0 + ((k >> 1) & 1), zz = cr.z0 + (k >> 2);
    if (!((unsigned)xx < (unsigned)W && (unsigned)yy < (unsigned)H && (unsigned)zz < (unsigned)D)) continue;
    const int64_t off = ((int64_t)zz * H + yy) * W + xx;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const float val = FIRST ? pre(src[c * V + off], c) : src[off * 3 + c];
      out[c] += val * cr.w[k];
    }
  }
}

template <bool FIRST, bool LAST>
__global__ __launch_bounds__(256) void diffeo_iter_kernel(const float *__restrict__ d_in, const float *__restrict__ i_in,
                                                          float *__restrict__ d_out, float *__restrict__ i_out, PreScale pre,
                                                          int N, int D, int H, int W) {
  const int64_t V = (int64_t)D * H * W, total = (int64_t)N * V;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int n = (int)(i / V);
    const int64_t v = i - (int64_t)n * V;
    const int w = (int)(v % W), h = (int)((v / W) % H), d = (int)(v / ((int64_t)W * H));
    const float id[3] = {lin_coord(w, W), lin_coord(h, H), lin_coord(d, D)};
    const float *dsrc = d_in + (int64_t)n * V * 3;
    float ds[3], is[3], nd[3], ni[3], s[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      ds[c] = FIRST ? pre(dsrc[c * V + v], c) : dsrc[v * 3 + c];
      is[c] = FIRST ? 0.f : i_in[i * 3 + c];
    }
    if (FIRST) {        // the inverse starts as zeros: its samples are exact zeros
#pragma unroll
      for (int c = 0; c < 3; ++c) nd[c] = 0.5f * ds[c];
    } else {
      sample3<false>(i_in + (int64_t)n * V * 3, pre, id[0] + ds[0], id[1] + ds[1], id[2] + ds[2], D, H, W, s);
#pragma unroll
      for (int c = 0; c < 3; ++c) nd[c] = 0.5f * ds[c] - 0.5f * s[c];
    }
    sample3<FIRST>(dsrc, pre, id[0] + is[0], id[1] + is[1], id[2] + is[2], D, H, W, s);
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      ni[c] = 0.5f * is[c] - 0.5f * s[c];
      if (LAST) {       // * 2^steps * [D,H,W][c]
        nd[c] = (nd[c] * pre.pow2) * pre.dim[c];
        ni[c] = (ni[c] * pre.pow2) * pre.dim[c];
      }
      d_out[i * 3 + c] = nd[c];
      i_out[i * 3 + c] = ni[c];
    }
  }
}

// ------------------------------------------------------------------------------------------------ dense-grid sampler
struct Item {
  int b, g, d, h, w;
  int64_t v;
};
__device__ __forceinline__ Item item_of(int64_t i, int cg, int64_t V, int H, int W, bool idx32) {
  Item t;
  if (idx32) {      // (uniform) 64-bit divisions cost more than the gather itself
    const unsigned ii = (unsigned)i, vox = ii / (unsigned)cg, vd = (unsigned)V;
    t.g = (int)(ii - vox * (unsigned)cg);
    t.b = (int)(vox / vd);
    const unsigned vv = vox - (unsigned)t.b * vd, r = vv / (unsigned)W;
    t.w = (int)(vv - r * (unsigned)W);
    t.d = (int)(r / (unsigned)H);
    t.h = (int)(r - (unsigned)t.d * (unsigned)H);
    t.v = vv;
  } else {
    t.g = (int)(i % cg);
    const int64_t vox = i / cg;
    t.b = (int)(vox / V);
    t.v = vox % V;
    t.w = (int)(t.v % W), t.h = (int)((t.v / W) % H), t.d = (int)(t.v / ((int64_t)W * H));
  }
  return t;
}

// tta.py:523-575: grid = (0 * identity + disp) + identity, then grid_sample(..., align_corners=False)
__device__ __forceinline__ Sample dense_sample(const float *__restrict__ disp, const Item &t, int64_t V, int D, int H, int W,
                                               int pad_mode) {
  const float *q = disp + ((int64_t)t.b * V + t.v) * 3;
  const float x = base_coord(t.w, W), y = base_coord(t.h, H), z = base_coord(t.d, D);
  const float gx = (0.0f * x + q[0]) + x, gy = (0.0f * y + q[1]) + y, gz = (0.0f * z + q[2]) + z;
  Sample s;
  s.ix = ((gx + 1.0f) * (float)W - 1.0f) / 2.0f;
  s.iy = ((gy + 1.0f) * (float)H - 1.0f) / 2.0f;
  s.iz = ((gz + 1.0f) * (float)D - 1.0f) / 2.0f;
  if (pad_mode == DGTTA_PAD_BORDER) {
    s.ix = fminf((float)(W - 1), fmaxf(s.ix, 0.f));
    s.iy = fminf((float)(H - 1), fmaxf(s.iy, 0.f));
    s.iz = fminf((float)(D - 1), fmaxf(s.iz, 0.f));
  }
  // far outside (or not a number): no corner is in bounds; keep the float -> int conversion in corners() defined
  const float lim = 1.0e8f;
  s.ix = (s.ix == s.ix) ? fminf(lim, fmaxf(s.ix, -lim)) : -lim;
  s.iy = (s.iy == s.iy) ? fminf(lim, fmaxf(s.iy, -lim)) : -lim;
  s.iz = (s.iz == s.iz) ? fminf(lim, fmaxf(s.iz, -lim)) : -lim;
  return s;
}

// VEC channels per thread (NDHWC: contiguous; NCDHW: VEC = 1 and the thread loops over the channels)
template <int VEC, bool NDHWC>
__global__ __launch_bounds__(256) void dense_warp_fwd_kernel(const float *__restrict__ src, const float *__restrict__ disp,
                                                             float *__restrict__ dst, int C, int D, int H, int W, int src_ldc,
                                                             int dst_ldc, int pad_mode, int64_t total) {
  const int cg = NDHWC ? (C / VEC) : 1;
  const int64_t V = (int64_t)D * H * W;
  const bool idx32 = total <= 0x7fffffffll;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const Item t = item_of(i, cg, V, H, W, idx32);
    const Corners cr = corners(dense_sample(disp, t, V, D, H, W, pad_mode));
    int64_t off[8];
    bool ok[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int xx = cr.x0 + (k & 1), yy = cr.y0 + ((k >> 1) & 1), zz = cr.z0 + (k >> 2);
      ok[k] = (unsigned)xx < (unsigned)W && (unsigned)yy < (unsigned)H && (unsigned)zz < (unsigned)D;
      // every corner is read at its CLAMPED address (eight loads in flight); one outside the volume then counts as 0
      off[k] = ((int64_t)min(max(zz, 0), D - 1) * H + min(max(yy, 0), H - 1)) * W + min(max(xx, 0), W - 1);
    }
    if (NDHWC) {
      float acc[VEC];
#pragma unroll
      for (int q = 0; q < VEC; ++q) acc[q] = 0.f;
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const float *sp = src + ((int64_t)t.b * V + off[k]) * src_ldc + t.g * VEC;
        if constexpr (VEC == 4) {
          const float4 x = *reinterpret_cast<const float4 *>(sp);
          acc[0] += ok[k] ? x.x * cr.w[k] : 0.f;
          acc[1] += ok[k] ? x.y * cr.w[k] : 0.f;
          acc[2] += ok[k] ? x.z * cr.w[k] : 0.f;
          acc[3] += ok[k] ? x.w * cr.w[k] : 0.f;
        } else {
#pragma unroll
          for (int q = 0; q < VEC; ++q) acc[q] += ok[k] ? sp[q] * cr.w[k] : 0.f;
        }
      }
      float *dp = dst + ((int64_t)t.b * V + t.v) * dst_ldc + t.g * VEC;
      if constexpr (VEC == 4) {
        *reinterpret_cast<float4 *>(dp) = make_float4(acc[0], acc[1], acc[2], acc[3]);
      } else {
#pragma unroll
        for (int q = 0; q < VEC; ++q) dp[q] = acc[q];
      }
    } else {
      for (int c = 0; c < C; ++c) {
        const float *sp = src + ((int64_t)t.b * C + c) * V;
        float acc = 0.f;
#pragma unroll
        for (int k = 0; k < 8; ++k) acc += ok[k] ? sp[off[k]] * cr.w[k] : 0.f;
        dst[((int64_t)t.b * C + c) * V + t.v] = acc;
      }
    }
  }
}

// adjoint w.r.t. src: scatter-add into a zeroed grad_src.  NDHWC: one lane per channel, so that the atomics of one
// wave-instruction cover whole rows of C floats
template <bool NDHWC>
__global__ __launch_bounds__(256) void dense_warp_bwd_kernel(const float *__restrict__ gdst, const float *__restrict__ disp,
                                                             float *__restrict__ gsrc, int C, int D, int H, int W, int src_ldc,
                                                             int dst_ldc, int pad_mode, int64_t total) {
  const int cg = NDHWC ? C : 1;
  const int64_t V = (int64_t)D * H * W;
  const bool idx32 = total <= 0x7fffffffll;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const Item t = item_of(i, cg, V, H, W, idx32);
    const Corners cr = corners(dense_sample(disp, t, V, D, H, W, pad_mode));
    const float g1 = NDHWC ? gdst[((int64_t)t.b * V + t.v) * dst_ldc + t.g] : 0.f;
#pragma unroll
    for (int k = 0; k < 8; ++k) {
      const int xx = cr.x0 + (k & 1), yy = cr.y0 + ((k >> 1) & 1), zz = cr.z0 + (k >> 2);
      if (!((unsigned)xx < (unsigned)W && (unsigned)yy < (unsigned)H && (unsigned)zz < (unsigned)D)) continue;
      const int64_t off = ((int64_t)zz * H + yy) * W + xx;
      if (NDHWC) {
        atomicAdd(gsrc + ((int64_t)t.b * V + off) * src_ldc + t.g, g1 * cr.w[k]);
      } else {
        for (int c = 0; c < C; ++c)
          atomicAdd(gsrc + ((int64_t)t.b * C + c) * V + off, gdst[((int64_t)t.b * C + c) * V + t.v] * cr.w[k]);
      }
    }
  }
}

int check_rf(const char *name, int P, int k, int Dl, int Hl, int Wl, int D, int H, int W) {
  DG_REQUIRE(P > 0 && Dl > 0 && Hl > 0 && Wl > 0 && D > 0 && H > 0 && W > 0, DGTTA_ERR_BADARG, "%s: bad dims", name);
  DG_REQUIRE(k >= 1 && (k & 1), DGTTA_ERR_UNSUPPORTED, "%s: the box width must be odd (got %d)", name, k);
  DG_REQUIRE(Dl >= k && Hl >= k && Wl >= k, DGTTA_ERR_BADARG,
             "%s: the low-resolution draw (%d x %d x %d) is smaller than the %d-wide box filter", name, Dl, Hl, Wl, k);
  DG_REQUIRE((int64_t)P * Dl * Hl * Wl < (1ll << 31), DGTTA_ERR_UNSUPPORTED, "%s: low-resolution draw too large", name);
  return DGTTA_OK;
}

size_t rf_low_bytes(int P, int Dl, int Hl, int Wl) { return align_up((size_t)P * Dl * Hl * Wl * sizeof(float), 256); }

int check_dense(const char *name, const void *a, const void *b, const void *c, int B, int C, int D, int H, int W, int ndhwc,
                int src_ldc, int dst_ldc, int pad_mode) {
  DG_REQUIRE(a && b && c, DGTTA_ERR_BADARG, "%s: null pointer", name);
  DG_REQUIRE(B > 0 && C > 0 && D > 0 && H > 0 && W > 0, DGTTA_ERR_BADARG, "%s: bad dims", name);
  DG_REQUIRE(!ndhwc || (src_ldc >= C && dst_ldc >= C), DGTTA_ERR_BADARG, "%s: ldc < C", name);
  DG_REQUIRE(pad_mode == DGTTA_PAD_ZEROS || pad_mode == DGTTA_PAD_BORDER, DGTTA_ERR_BADARG, "%s: bad pad_mode", name);
  return DGTTA_OK;
}

}  // namespace

extern "C" size_t dgtta_rf_field_ws_bytes(int P, int Dl, int Hl, int Wl) {
  if (P <= 0 || Dl <= 0 || Hl <= 0 || Wl <= 0) return 0;
  return 2 * rf_low_bytes(P, Dl, Hl, Wl) + (size_t)P * RF_STAT_BLOCKS * 2 * sizeof(double);
}

extern "C" int dgtta_rf_field_fwd(const float *draw, float *field, void *ws, size_t ws_bytes, int P, int k, int Dl, int Hl,
                                  int Wl, int D, int H, int W, void *stream) {
  DG_REQUIRE(draw && field && ws, DGTTA_ERR_BADARG, "rf_field_fwd: null pointer");
  int rc = check_rf("rf_field_fwd", P, k, Dl, Hl, Wl, D, H, W);
  if (rc) return rc;
  DG_REQUIRE(P <= 65535, DGTTA_ERR_UNSUPPORTED, "rf_field_fwd: at most 65535 planes per call");
  DG_REQUIRE(ws_bytes >= dgtta_rf_field_ws_bytes(P, Dl, Hl, Wl), DGTTA_ERR_WORKSPACE, "rf_field_fwd: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  float *a = (float *)ws, *b = (float *)((char *)ws + rf_low_bytes(P, Dl, Hl, Wl));
  double *partial = (double *)((char *)ws + 2 * rf_low_bytes(P, Dl, Hl, Wl));
  const int nlow = P * Dl * Hl * Wl, gl = grid_for(nlow);
  hipLaunchKernelGGL(rf_box_kernel, dim3(gl), dim3(256), 0, st, draw, a, P, Dl, Hl, Wl, k);
  hipLaunchKernelGGL(rf_box_kernel, dim3(gl), dim3(256), 0, st, (const float *)a, b, P, Dl, Hl, Wl, k);
  hipLaunchKernelGGL(rf_box_kernel, dim3(gl), dim3(256), 0, st, (const float *)b, a, P, Dl, Hl, Wl, k);
  DG_CHECK_LAUNCH("rf_box_kernel");
  hipLaunchKernelGGL(rf_stats_kernel, dim3(RF_STAT_BLOCKS, P), dim3(256), 0, st, (const float *)a, partial, Dl, Hl, Wl, D, H, W);
  DG_CHECK_LAUNCH("rf_stats_kernel");
  const int64_t V = (int64_t)D * H * W;
  const int gn = (int)std::min<int64_t>(cdiv64(V, 256 * 4), 1024);
  hipLaunchKernelGGL(rf_norm_kernel, dim3(gn, P), dim3(256), 0, st, (const float *)a, (const double *)partial, field, Dl, Hl, Wl,
                     D, H, W);
  DG_CHECK_LAUNCH("rf_norm_kernel");
  return DGTTA_OK;
}

extern "C" size_t dgtta_diffeo_fields_ws_bytes(int N, int D, int H, int W) {
  if (N <= 0 || D <= 0 || H <= 0 || W <= 0) return 0;
  return 2 * align_up((size_t)N * D * H * W * 3 * sizeof(float), 256);
}

extern "C" int dgtta_diffeo_fields(const float *field, float factor, float *disp, float *inverse, void *ws, size_t ws_bytes,
                                   int N, int D, int H, int W, int time_steps, void *stream) {
  DG_REQUIRE(field && disp && inverse && ws, DGTTA_ERR_BADARG, "diffeo_fields: null pointer");
  DG_REQUIRE(N > 0 && D > 0 && H > 0 && W > 0, DGTTA_ERR_BADARG, "diffeo_fields: bad dims");
  DG_REQUIRE(time_steps >= 1 && time_steps <= 30, DGTTA_ERR_BADARG, "diffeo_fields: time_steps must be in 1..30");
  DG_REQUIRE(ws_bytes >= dgtta_diffeo_fields_ws_bytes(N, D, H, W), DGTTA_ERR_WORKSPACE, "diffeo_fields: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  const size_t half = align_up((size_t)N * D * H * W * 3 * sizeof(float), 256);
  float *wd = (float *)ws, *wi = (float *)((char *)ws + half);
  PreScale pre;
  pre.factor = factor;
  pre.dim[0] = (float)D, pre.dim[1] = (float)H, pre.dim[2] = (float)W;   // as written: channel 0 (the x displacement) by D
  pre.pow2 = (float)(1u << time_steps);
  pre.dt = (float)(1.0 / (double)time_steps);
  const int g = grid_for((int64_t)N * D * H * W);
  // ping-pong between the outputs and the workspace so that the last iteration lands in the outputs
  const float *din = field, *iin = nullptr;
  for (int it = 0; it < time_steps; ++it) {
    const bool first = it == 0, last = it == time_steps - 1;
    const bool to_out = ((time_steps - 1 - it) & 1) == 0;
    float *dout = to_out ? disp : wd, *iout = to_out ? inverse : wi;
#define DIFFEO_LAUNCH(F, L) \
  hipLaunchKernelGGL((diffeo_iter_kernel<F, L>), dim3(g), dim3(256), 0, st, din, iin, dout, iout, pre, N, D, H, W)
    if (first && last) DIFFEO_LAUNCH(true, true);
    else if (first) DIFFEO_LAUNCH(true, false);
    else if (last) DIFFEO_LAUNCH(false, true);
    else DIFFEO_LAUNCH(false, false);
#undef DIFFEO_LAUNCH
    DG_CHECK_LAUNCH("diffeo_iter_kernel");
    din = dout, iin = iout;
  }
  return DGTTA_OK;
}

extern "C" int dgtta_dense_warp3d_fwd(const float *src, const float *disp, float *dst, int B, int C, int D, int H, int W,
                                      int ndhwc, int src_ldc, int dst_ldc, int pad_mode, void *stream) {
  int rc = check_dense("dense_warp3d_fwd", src, disp, dst, B, C, D, H, W, ndhwc, src_ldc, dst_ldc, pad_mode);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  const int64_t V = (int64_t)D * H * W;
  if (ndhwc) {
    const bool v4 = (C % 4 == 0) && (src_ldc % 4 == 0) && (dst_ldc % 4 == 0) && ((uintptr_t)src % 16 == 0) &&
                    ((uintptr_t)dst % 16 == 0);
    if (v4) {
      const int64_t total = (int64_t)B * V * (C / 4);
      hipLaunchKernelGGL((dense_warp_fwd_kernel<4, true>), dim3(grid_for(total)), dim3(256), 0, st, src, disp, dst, C, D, H, W,
                         src_ldc, dst_ldc, pad_mode, total);
    } else {
      const int64_t total = (int64_t)B * V * C;
      hipLaunchKernelGGL((dense_warp_fwd_kernel<1, true>), dim3(grid_for(total)), dim3(256), 0, st, src, disp, dst, C, D, H, W,
                         src_ldc, dst_ldc, pad_mode, total);
    }
  } else {
    const int64_t total = (int64_t)B * V;
    hipLaunchKernelGGL((dense_warp_fwd_kernel<1, false>), dim3(grid_for(total)), dim3(256), 0, st, src, disp, dst, C, D, H, W,
                       src_ldc, dst_ldc, pad_mode, total);
  }
  DG_CHECK_LAUNCH("dense_warp_fwd_kernel");
  return DGTTA_OK;
}

extern "C" int dgtta_dense_warp3d_bwd(const float *grad_dst, const float *disp, float *grad_src, int B, int C, int D, int H,
                                      int W, int ndhwc, int src_ldc, int dst_ldc, int pad_mode, void *stream) {
  int rc = check_dense("dense_warp3d_bwd", grad_dst, disp, grad_src, B, C, D, H, W, ndhwc, src_ldc, dst_ldc, pad_mode);
  if (rc) return rc;
  hipStream_t st = (hipStream_t)stream;
  const int64_t V = (int64_t)D * H * W;
  const size_t nb = (size_t)B * V * (ndhwc ? src_ldc : C) * sizeof(float);
  hipError_t e = hipMemsetAsync(grad_src, 0, nb, st);
  DG_REQUIRE(e == hipSuccess, DGTTA_ERR_LAUNCH, "dense_warp3d_bwd: memset failed: %s", hipGetErrorString(e));
  if (ndhwc) {
    const int64_t total = (int64_t)B * V * C;
    hipLaunchKernelGGL((dense_warp_bwd_kernel<true>), dim3(grid_for(total)), dim3(256), 0, st, grad_dst, disp, grad_src, C, D, H,
                       W, src_ldc, dst_ldc, pad_mode, total);
  } else {
    const int64_t total = (int64_t)B * V;
    hipLaunchKernelGGL((dense_warp_bwd_kernel<false>), dim3(grid_for(total)), dim3(256), 0, st, grad_dst, disp, grad_src, C, D, H,
                       W, src_ldc, dst_ldc, pad_mode, total);
  }
  DG_CHECK_LAUNCH("dense_warp_bwd_kernel");
  return DGTTA_OK;
}
