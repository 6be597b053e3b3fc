// nnU-Net's intensity augmentation for pre-training (pretraining/intensity.py draws the parameters and chains the stages):
// Gaussian noise, Gaussian blur, brightness, contrast and the two gamma transforms on a batch [B][V] of fp32 patches.  Three
// entry points; each takes up to 16 item descriptors that travel in the kernel arguments (nothing is uploaded), and a batch
// item that no descriptor names is neither read nor written.  Definitions and operation order: include/dgtta.h.
//   dgtta_intensity_stats  per item min, max, mean, population std as doubles on the device.  HBM-bound, 1 read per voxel.
//                          dgtta_grad_sumsq's scheme: every workgroup writes one partial (S1, S2, min, max) of its 4096
//                          voxels into the caller's workspace at a slot fixed by (descriptor, chunk); one last workgroup adds
//                          the slots in a fixed order in double.  No floating-point atomics, no hand-off inside a launch.
//                          Sums are taken about the pivot p = the item's first voxel, so a constant item has std 0 exactly.
//   dgtta_intensity_map    one elementwise pass, 1 read + 1 write per voxel; the grid carries (chunk, descriptor), so mode and
//                          parameters are uniform per workgroup.  Data-dependent parameters (the statistics) are read on the
//                          device: the chain needs no host synchronisation.  The noise of mode LINEAR is generated in the
//                          kernel (csrc/philox.h), one Philox call per four voxels on the 16-byte path.
//   dgtta_gauss_blur3      separable, per-item taps, scipy's "reflect" boundary.  D and H passes: one thread per four
//                          consecutive W (one 16-byte access per tap row; lanes along W, every row coalesced), loads
//                          unconditional at reflected indices.  W pass: one wave per row, the row staged in LDS (16-byte
//                          loads), taps read at lane stride 1 (no bank conflict), the result staged in LDS again and stored
//                          with 16-byte stores; a row is complete in LDS before it is written, so the pass runs in place.
// 16-byte accesses on aligned full chunks, a scalar path for the rest; which of the two runs depends only on addresses and
// extents, never on the run.
#include "common.h"
#include "philox.h"
#include <math.h>

namespace {

constexpr int MAXI = DGTTA_INTENSITY_MAX_ITEMS;
constexpr int CHUNK = 256 * 16;   // voxels per workgroup of the stats and map kernels
constexpr int BLUR_MAX_W = 2048;  // W pass: two staged rows per wave, four waves, 64 KiB of LDS

struct StatItems {
  int item[MAXI];
};
struct MapItems {
  DgttaIntensityItem it[MAXI];
};
struct BlurItems {
  DgttaBlurItem it[MAXI];
};

__device__ __forceinline__ bool aligned16(const void *a) { return ((uintptr_t)a & 15) == 0; }

__device__ __forceinline__ double wave_min_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmin(v, __shfl_xor(v, o, 64));
  return v;
}
__device__ __forceinline__ double wave_max_d(double v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v = fmax(v, __shfl_xor(v, o, 64));
  return v;
}

// ------------------------------------------------------------------------------------------------ statistics
__device__ __forceinline__ void stat_add(float v, double p, double &s1, double &s2, float &mn, float &mx) {
  const double d = (double)v - p;
  s1 += d;
  s2 += d * d;
  mn = fminf(mn, v);
  mx = fmaxf(mx, v);
}

// partial[(blockIdx.y * chunks + blockIdx.x) * 4 ..] = (S1, S2, min, max) of this workgroup's chunk.  Per thread 16 voxels in
// index order, across the workgroup a fixed tree.
__global__ __launch_bounds__(256) void intensity_stats_partial_kernel(StatItems a, const float *__restrict__ x, int64_t V,
                                                                      double *__restrict__ partial) {
  __shared__ double red[4][4];
  const float *xi = x + (int64_t)a.item[blockIdx.y] * V;
  const int64_t base = (int64_t)blockIdx.x * CHUNK;      // < V: the grid has ceil(V / CHUNK) chunks
  const double p = (double)xi[0];
  double s1 = 0.0, s2 = 0.0;
  float mn = xi[base], mx = mn;
  if (base + CHUNK <= V && aligned16(xi)) {
    const float4 *x4 = reinterpret_cast<const float4 *>(xi + base);
#pragma unroll
    for (int k = 0; k < CHUNK / 1024; ++k) {
      const float4 v = x4[k * 256 + threadIdx.x];
      stat_add(v.x, p, s1, s2, mn, mx);
      stat_add(v.y, p, s1, s2, mn, mx);
      stat_add(v.z, p, s1, s2, mn, mx);
      stat_add(v.w, p, s1, s2, mn, mx);
    }
  } else {
#pragma unroll 4
    for (int k = 0; k < CHUNK / 256; ++k) {
      const int64_t i = base + k * 256 + threadIdx.x;
      if (i < V) stat_add(xi[i], p, s1, s2, mn, mx);
    }
  }
  s1 = wave_sum_d(s1);
  s2 = wave_sum_d(s2);
  const double dmn = wave_min_d((double)mn), dmx = wave_max_d((double)mx);
  const int w = threadIdx.x >> 6;
  if ((threadIdx.x & 63) == 0) {
    red[w][0] = s1;
    red[w][1] = s2;
    red[w][2] = dmn;
    red[w][3] = dmx;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    double *o = partial + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * 4;
    o[0] = ((red[0][0] + red[1][0]) + red[2][0]) + red[3][0];
    o[1] = ((red[0][1] + red[1][1]) + red[2][1]) + red[3][1];
    o[2] = fmin(fmin(red[0][2], red[1][2]), fmin(red[2][2], red[3][2]));
    o[3] = fmax(fmax(red[0][3], red[1][3]), fmax(red[2][3], red[3][3]));
  }
}

// One workgroup, descriptor after descriptor: thread t adds slots t, t + 256, ... in double, then the same fixed tree.
__global__ __launch_bounds__(256) void intensity_stats_final_kernel(StatItems a, int n_items, const float *__restrict__ x, int64_t V,
                                                                    const double *__restrict__ partial, int chunks,
                                                                    double *__restrict__ stats) {
  __shared__ double red[4][4];
  for (int k = 0; k < n_items; ++k) {
    const double *p = partial + (int64_t)k * chunks * 4;
    double s1 = 0.0, s2 = 0.0, mn = p[2], mx = p[3];
    for (int i = threadIdx.x; i < chunks; i += 256) {
      s1 += p[4 * i];
      s2 += p[4 * i + 1];
      mn = fmin(mn, p[4 * i + 2]);
      mx = fmax(mx, p[4 * i + 3]);
    }
    s1 = wave_sum_d(s1);
    s2 = wave_sum_d(s2);
    mn = wave_min_d(mn);
    mx = wave_max_d(mx);
    const int w = threadIdx.x >> 6;
    __syncthreads();                      // the previous descriptor's result has been read
    if ((threadIdx.x & 63) == 0) {
      red[w][0] = s1;
      red[w][1] = s2;
      red[w][2] = mn;
      red[w][3] = mx;
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      const double pivot = (double)x[(int64_t)a.item[k] * V];
      const double m1 = (((red[0][0] + red[1][0]) + red[2][0]) + red[3][0]) / (double)V;
      const double m2 = (((red[0][1] + red[1][1]) + red[2][1]) + red[3][1]) / (double)V;
      const double var = m2 - m1 * m1;
      double *o = stats + (int64_t)a.item[k] * 4;
      o[0] = fmin(fmin(red[0][2], red[1][2]), fmin(red[2][2], red[3][2]));
      o[1] = fmax(fmax(red[0][3], red[1][3]), fmax(red[2][3], red[3][3]));
      o[2] = pivot + m1;
      o[3] = var > 0.0 ? sqrt(var) : 0.0;
    }
  }
}

// ------------------------------------------------------------------------------------------------ elementwise map
struct MapParams {      // uniform per workgroup
  int mode, negate;
  float a, s, c0, c1, c2, c3;
};

// include/dgtta.h gives these formulas in this order
__device__ __forceinline__ float map_one(const MapParams &q, float x, float n) {
  switch (q.mode) {
    case DGTTA_IMAP_LINEAR:
      return q.s != 0.f ? x * q.a + q.s * n : x * q.a;
    case DGTTA_IMAP_CONTRAST: {      // c0 mean, c1 lo, c2 hi
      const float y = (x - q.c0) * q.a + q.c0;
      return fminf(fmaxf(y, q.c1), q.c2);
    }
    case DGTTA_IMAP_GAMMA: {         // c0 lo, c1 r, c2 r + 1e-7f
      const float xi = q.negate ? -x : x;
      return powf((xi - q.c0) / q.c2, q.a) * q.c1 + q.c0;
    }
    default: {                       // RESTORE: c0 mn, c1 sd, c2 mn2, c3 sd2 + 1e-8f
      const float y = (x - q.c2) / q.c3 * q.c1 + q.c0;
      return q.negate ? -y : y;
    }
  }
}

__global__ __launch_bounds__(256) void intensity_map_kernel(MapItems items, const float *src_, float *dst_,
                                                            int64_t V, const double *__restrict__ stats,
                                                            const double *__restrict__ stats2) {
  const DgttaIntensityItem &it = items.it[blockIdx.y];
  MapParams q;
  q.mode = it.mode;
  q.negate = it.negate;
  q.a = it.a;
  q.s = it.s;
  q.c0 = q.c1 = q.c2 = q.c3 = 0.f;
  if (q.mode != DGTTA_IMAP_LINEAR) {
    const double *st = stats + (int64_t)it.item * 4;       // min, max, mean, std
    if (q.mode == DGTTA_IMAP_CONTRAST) {
      q.c0 = (float)st[2];
      q.c1 = (float)st[0];
      q.c2 = (float)st[1];
    } else if (q.mode == DGTTA_IMAP_GAMMA) {
      q.c0 = q.negate ? -(float)st[1] : (float)st[0];
      q.c1 = (float)(st[1] - st[0]);
      q.c2 = q.c1 + 1e-7f;
    } else {
      const double *s2 = stats2 + (int64_t)it.item * 4;
      q.c0 = q.negate ? -(float)st[2] : (float)st[2];
      q.c1 = (float)st[3];
      q.c2 = (float)s2[2];
      q.c3 = (float)s2[3] + 1e-8f;
    }
  }
  const bool noisy = q.mode == DGTTA_IMAP_LINEAR && q.s != 0.f;
  const float *src = src_ + (int64_t)it.item * V;
  float *dst = dst_ + (int64_t)it.item * V;
  const int64_t base = (int64_t)blockIdx.x * CHUNK;
  if (base + CHUNK <= V && aligned16(src) && aligned16(dst)) {
    const float4 *s4 = reinterpret_cast<const float4 *>(src + base);
    float4 *d4 = reinterpret_cast<float4 *>(dst + base);
#pragma unroll
    for (int k = 0; k < CHUNK / 1024; ++k) {
      const int j = k * 256 + threadIdx.x;
      const float4 v = s4[j];
      float n[4] = {0.f, 0.f, 0.f, 0.f};
      if (noisy) {                                      // voxels 4 g .. 4 g + 3 are the four normals of Philox call g
        uint32_t w[4];
        philox4x32_10((uint32_t)(base / 4 + j), (uint32_t)it.noise_b, it.off_lo, it.off_hi, it.seed_lo, it.seed_hi, w);
        philox_normal_pair(w[0], w[1], n[0], n[1]);
        philox_normal_pair(w[2], w[3], n[2], n[3]);
      }
      d4[j] = make_float4(map_one(q, v.x, n[0]), map_one(q, v.y, n[1]), map_one(q, v.z, n[2]), map_one(q, v.w, n[3]));
    }
  } else {
#pragma unroll 2
    for (int k = 0; k < CHUNK / 256; ++k) {
      const int64_t i = base + k * 256 + threadIdx.x;
      if (i < V) {
        float n = 0.f;
        if (noisy) {
          uint32_t w[4];
          float n0, n1;
          philox4x32_10((uint32_t)(i >> 2), (uint32_t)it.noise_b, it.off_lo, it.off_hi, it.seed_lo, it.seed_hi, w);
          const bool hi = (i & 2) != 0;
          philox_normal_pair(hi ? w[2] : w[0], hi ? w[3] : w[1], n0, n1);
          n = (i & 1) ? n1 : n0;
        }
        dst[i] = map_one(q, src[i], n);
      }
    }
  }
}

// ------------------------------------------------------------------------------------------------ Gaussian blur
// scipy's "reflect": j mod 2n, mirrored when >= n.  The taps reach at most 4 past either end: one fold when n > 4.
__device__ __forceinline__ int reflect_idx(int j, int n) {
  if (n > 4) {
    j = j < 0 ? -1 - j : j;
    return j >= n ? 2 * n - 1 - j : j;
  }
  const int p = 2 * n;
  j %= p;
  j = j < 0 ? j + p : j;
  return j >= n ? p - 1 - j : j;
}

// D (axis 0) or H (axis 1) pass: thread = VEC consecutive W of one row, block 64 x 4 = (w, h), grid.z = d + D * descriptor.
template <int VEC>
__global__ __launch_bounds__(256) void gauss_blur_dh_kernel(BlurItems items, const float *__restrict__ src, float *__restrict__ dst,
                                                            int D, int H, int W, int axis) {
  const int w = ((int)blockIdx.x * 64 + (int)threadIdx.x) * VEC, h = (int)blockIdx.y * 4 + (int)threadIdx.y;
  const int d = (int)blockIdx.z % D;
  if (w >= W || h >= H) return;
  const DgttaBlurItem &it = items.it[(int)blockIdx.z / D];
  const int n = axis == 0 ? D : H, pos = axis == 0 ? d : h, r = it.radius;
  const int64_t stride = axis == 0 ? (int64_t)H * W : W;
  const int64_t o = (((int64_t)it.item * D + d) * H + h) * W + w, line = o - pos * stride;
  if (VEC == 4) {
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int k = 0; k <= 2 * r; ++k) {
      const float t = it.taps[k];
      const float4 v = *reinterpret_cast<const float4 *>(src + line + reflect_idx(pos + k - r, n) * stride);
      acc.x += t * v.x;
      acc.y += t * v.y;
      acc.z += t * v.z;
      acc.w += t * v.w;
    }
    *reinterpret_cast<float4 *>(dst + o) = acc;
  } else {
    float acc = 0.f;
    for (int k = 0; k <= 2 * r; ++k) acc += it.taps[k] * src[line + reflect_idx(pos + k - r, n) * stride];
    dst[o] = acc;
  }
}

// W pass: wave = one row (rows = descriptors x D x H), staged whole in LDS; dst may be src.
__global__ __launch_bounds__(256) void gauss_blur_w_kernel(BlurItems items, const float *src_, float *dst_,
                                                           int64_t total_rows, int rows_per_item, int W, int Wp, int vec) {
  extern __shared__ float4 blur_lds[];
  const int wave = (int)threadIdx.x >> 6, lane = (int)threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + wave;
  const bool live = row < total_rows;
  float *in = reinterpret_cast<float *>(blur_lds) + wave * 2 * Wp, *out = in + Wp;
  const int k = live ? (int)(row / rows_per_item) : 0;
  const DgttaBlurItem &it = items.it[k];
  const int64_t off = ((int64_t)it.item * rows_per_item + (live ? row % rows_per_item : 0)) * W;
  const float *src = src_ + off;
  float *dst = dst_ + off;
  if (live) {
    if (vec) {
      for (int c = lane; c < W / 4; c += 64) reinterpret_cast<float4 *>(in)[c] = reinterpret_cast<const float4 *>(src)[c];
    } else {
      for (int c = lane; c < W; c += 64) in[c] = src[c];
    }
  }
  __syncthreads();
  if (live) {
    const int r = it.radius;
    for (int c = lane; c < W; c += 64) {
      float acc = 0.f;
      for (int t = 0; t <= 2 * r; ++t) acc += it.taps[t] * in[reflect_idx(c + t - r, W)];
      out[c] = acc;
    }
  }
  __syncthreads();
  if (live) {
    if (vec) {
      for (int c = lane; c < W / 4; c += 64) reinterpret_cast<float4 *>(dst)[c] = reinterpret_cast<const float4 *>(out)[c];
    } else {
      for (int c = lane; c < W; c += 64) dst[c] = out[c];
    }
  }
}

inline uint64_t chunks_of(int64_t n) { return n > 0 ? ((uint64_t)n + CHUNK - 1) / CHUNK : 0; }

}  // namespace

extern "C" size_t dgtta_intensity_stats_ws_bytes(int n_items, int64_t V) {
  // four doubles per (descriptor, chunk); one spare slot keeps the size non-zero.  Unsigned: 2^31 descriptors of 2^40 voxels
  // stay below 2^64 bytes.
  const uint64_t slots = (n_items > 0 ? (uint64_t)n_items : 0) * chunks_of(V) + 1;
  return (size_t)(slots * 4 * sizeof(double));
}

extern "C" int dgtta_intensity_stats(const float *x, int B, int64_t V, const int *h_items, int n_items, double *stats, void *ws,
                                     size_t ws_bytes, void *stream) {
  DG_REQUIRE(x && h_items && stats && ws, DGTTA_ERR_BADARG, "intensity_stats: null pointer");
  DG_REQUIRE(n_items >= 1 && n_items <= MAXI, DGTTA_ERR_BADARG, "intensity_stats: 1..%d items per launch (got %d)", MAXI, n_items);
  DG_REQUIRE(B >= 1 && V >= 1, DGTTA_ERR_BADARG, "intensity_stats: bad batch %d x %lld", B, (long long)V);
  DG_REQUIRE(V < (1ll << 31), DGTTA_ERR_UNSUPPORTED, "intensity_stats: 2^31 voxels or more per item");
  DG_REQUIRE(((uintptr_t)ws & 7) == 0, DGTTA_ERR_WORKSPACE, "intensity_stats: workspace must be 8-byte aligned");
  const uint64_t chunks = chunks_of(V), need = (uint64_t)n_items * chunks * 4 * sizeof(double);
  DG_REQUIRE(need <= ws_bytes, DGTTA_ERR_WORKSPACE, "intensity_stats: workspace of %zu bytes, %llu needed (dgtta_intensity_stats_ws_bytes)",
             ws_bytes, (unsigned long long)need);
  StatItems a{};
  for (int k = 0; k < n_items; ++k) {
    DG_REQUIRE(h_items[k] >= 0 && h_items[k] < B, DGTTA_ERR_BADARG, "intensity_stats: descriptor %d names item %d of %d", k, h_items[k], B);
    a.item[k] = h_items[k];
  }
  const hipStream_t st = (hipStream_t)stream;
  double *partial = (double *)ws;
  hipLaunchKernelGGL(intensity_stats_partial_kernel, dim3((unsigned)chunks, (unsigned)n_items), dim3(256), 0, st, a, x, V, partial);
  DG_CHECK_LAUNCH("intensity_stats_partial_kernel");
  hipLaunchKernelGGL(intensity_stats_final_kernel, dim3(1), dim3(256), 0, st, a, n_items, x, V, (const double *)partial, (int)chunks, stats);
  DG_CHECK_LAUNCH("intensity_stats_final_kernel");
  return DGTTA_OK;
}

extern "C" int dgtta_intensity_map(const float *src, float *dst, int B, int64_t V, const DgttaIntensityItem *h_items, int n_items,
                                   const double *stats, const double *stats2, void *stream) {
  DG_REQUIRE(src && dst && h_items, DGTTA_ERR_BADARG, "intensity_map: null pointer");
  DG_REQUIRE(n_items >= 1 && n_items <= MAXI, DGTTA_ERR_BADARG, "intensity_map: 1..%d items per launch (got %d)", MAXI, n_items);
  DG_REQUIRE(B >= 1 && V >= 1, DGTTA_ERR_BADARG, "intensity_map: bad batch %d x %lld", B, (long long)V);
  DG_REQUIRE(V < (1ll << 31), DGTTA_ERR_UNSUPPORTED, "intensity_map: 2^31 voxels or more per item");
  MapItems a{};
  for (int k = 0; k < n_items; ++k) {
    const DgttaIntensityItem &it = h_items[k];
    DG_REQUIRE(it.item >= 0 && it.item < B, DGTTA_ERR_BADARG, "intensity_map: descriptor %d names item %d of %d", k, it.item, B);
    DG_REQUIRE(it.mode >= DGTTA_IMAP_LINEAR && it.mode <= DGTTA_IMAP_RESTORE, DGTTA_ERR_UNSUPPORTED, "intensity_map: descriptor %d: mode %d", k, it.mode);
    DG_REQUIRE(isfinite(it.a) && isfinite(it.s), DGTTA_ERR_BADARG, "intensity_map: descriptor %d: a parameter is not finite", k);
    DG_REQUIRE(it.mode == DGTTA_IMAP_LINEAR || stats, DGTTA_ERR_BADARG, "intensity_map: descriptor %d: mode %d reads `stats`", k, it.mode);
    DG_REQUIRE(it.mode != DGTTA_IMAP_RESTORE || stats2, DGTTA_ERR_BADARG, "intensity_map: descriptor %d: RESTORE reads `stats2`", k);
    DG_REQUIRE(it.mode != DGTTA_IMAP_GAMMA || it.a > 0.f, DGTTA_ERR_BADARG, "intensity_map: descriptor %d: the gamma exponent must be positive", k);
    a.it[k] = it;
  }
  hipLaunchKernelGGL(intensity_map_kernel, dim3((unsigned)chunks_of(V), (unsigned)n_items), dim3(256), 0, (hipStream_t)stream, a, src, dst,
                     V, stats, stats2);
  DG_CHECK_LAUNCH("intensity_map_kernel");
  return DGTTA_OK;
}

extern "C" int dgtta_gauss_blur3(const float *src, float *dst, float *scratch, int B, int D, int H, int W, const DgttaBlurItem *h_items,
                                 int n_items, void *stream) {
  DG_REQUIRE(src && dst && scratch && h_items, DGTTA_ERR_BADARG, "gauss_blur3: null pointer");
  DG_REQUIRE(scratch != src && scratch != dst, DGTTA_ERR_BADARG, "gauss_blur3: scratch must be a buffer of its own");
  DG_REQUIRE(n_items >= 1 && n_items <= MAXI, DGTTA_ERR_BADARG, "gauss_blur3: 1..%d items per launch (got %d)", MAXI, n_items);
  DG_REQUIRE(B >= 1 && D > 0 && H > 0 && W > 0, DGTTA_ERR_BADARG, "gauss_blur3: bad batch %d x %d x %d x %d", B, D, H, W);
  DG_REQUIRE((int64_t)D * H * W < (1ll << 31), DGTTA_ERR_UNSUPPORTED, "gauss_blur3: 2^31 voxels or more per item");
  DG_REQUIRE(W <= BLUR_MAX_W, DGTTA_ERR_UNSUPPORTED, "gauss_blur3: W = %d above %d (a row is staged in LDS)", W, BLUR_MAX_W);
  DG_REQUIRE((int64_t)D * n_items <= 65535 && cdiv(H, 4) <= 65535, DGTTA_ERR_UNSUPPORTED, "gauss_blur3: patch too large for one grid");
  BlurItems a{};
  for (int k = 0; k < n_items; ++k) {
    const DgttaBlurItem &it = h_items[k];
    DG_REQUIRE(it.item >= 0 && it.item < B, DGTTA_ERR_BADARG, "gauss_blur3: descriptor %d names item %d of %d", k, it.item, B);
    DG_REQUIRE(it.radius >= 1 && it.radius <= 4, DGTTA_ERR_BADARG, "gauss_blur3: descriptor %d: radius %d not in 1..4", k, it.radius);
    for (int t = 0; t <= 2 * it.radius; ++t)
      DG_REQUIRE(isfinite(it.taps[t]), DGTTA_ERR_BADARG, "gauss_blur3: descriptor %d: tap %d is not finite", k, t);
    a.it[k] = it;
  }
  const hipStream_t st = (hipStream_t)stream;
  const bool vec = W % 4 == 0 && (((uintptr_t)src | (uintptr_t)dst | (uintptr_t)scratch) & 15) == 0;
  const dim3 block(64, 4), grid((unsigned)cdiv(W, vec ? 256 : 64), (unsigned)cdiv(H, 4), (unsigned)(D * n_items));
  if (vec) {
    hipLaunchKernelGGL(gauss_blur_dh_kernel<4>, grid, block, 0, st, a, src, scratch, D, H, W, 0);
    hipLaunchKernelGGL(gauss_blur_dh_kernel<4>, grid, block, 0, st, a, (const float *)scratch, dst, D, H, W, 1);
  } else {
    hipLaunchKernelGGL(gauss_blur_dh_kernel<1>, grid, block, 0, st, a, src, scratch, D, H, W, 0);
    hipLaunchKernelGGL(gauss_blur_dh_kernel<1>, grid, block, 0, st, a, (const float *)scratch, dst, D, H, W, 1);
  }
  DG_CHECK_LAUNCH("gauss_blur_dh_kernel");
  const int Wp = (W + 3) / 4 * 4;
  const int64_t rows = (int64_t)n_items * D * H;
  hipLaunchKernelGGL(gauss_blur_w_kernel, dim3((unsigned)cdiv64(rows, 4)), dim3(256), (size_t)8 * Wp * sizeof(float), st, a,
                     (const float *)dst, dst, rows, D * H, W, Wp, vec ? 1 : 0);
  DG_CHECK_LAUNCH("gauss_blur_w_kernel");
  return DGTTA_OK;
}
