// nnU-Net's rotation / scaling augmentation for pre-training (pretraining/spatial.py draws the maps): patches are SAMPLED
// from the resident case through an affine voxel map instead of cropped.  nnU-Net 2.2 samples with
// scipy.ndimage.map_coordinates - cubic B-spline for the image, order 1 per label with a 0.5 threshold for the segmentation
// (restated from memory of batchgenerators' SpatialTransform, UNPINNED).  Two entry points:
//   dgtta_bspline3_prefilter  scipy.ndimage.spline_filter(order=3, mode="mirror") of one fp32 volume, in fp32: per axis and
//                             line, gain 6, pole z = sqrt(3) - 2, the causal and the anticausal recursion with scipy's mirror
//                             initialisation (csrc/resample.hip has the float64 recursion for padded lines).  One thread per
//                             line, three launches of one kernel: along D and H consecutive lanes hold consecutive W, so every
//                             step of the recursion is one coalesced row; along W a lane walks its own row (each 128-byte line
//                             is then read by one lane 32 times in a row, out of the cache).  Runs once per case.
//   dgtta_patch_sample_aug    one launch, up to 16 items whose descriptors travel in the kernel arguments; one thread per output
//                             voxel, lanes along the patch's W, the grid carries (w tile, h tile, d * B + b): no division by a
//                             runtime extent per voxel.  Source position x(v) = A v + t from the item's fp32 3x4 map, evaluated
//                             in DOUBLE (9 products of an fp32 by a small integer, exact, + 9 sums: ~20 fp64 operations beside
//                             64 loads): the position is then exact to 1e-14 voxel and the only fp32 rounding left in it is the
//                             one of the fractional part, so the inside / outside decision and the label masses do not carry an
//                             error that grows with the coordinate.
//                             Image, ORDER 3: 0 when x leaves [0, n - 1] on any axis (mode="constant", cval=0), else the 4x4x4
//                             taps at floor(x) - 1 .. floor(x) + 2 with scipy's mirrored tap indices on the coefficient volume;
//                             ORDER 1: the same rule with 2x2x2 taps on the raw volume.  Every load is unconditional at a
//                             clamped / mirrored index and the result is selected afterwards (a conditional load costs a
//                             dependent round trip).  Summation order: w innermost, then h, then d, plain fp32, no FMA.
//                             Label: the 8 trilinear corners of x in registers; a corner outside the volume carries label 0;
//                             mass(l) = sum of the weights of the corners that carry l; result = the largest l > 0 with
//                             mass >= 0.5, else 0, written as int64.  No atomics, no LDS.
#include "common.h"
#include <math.h>

namespace {

struct PatchItems {
  DgttaPatchItem it[DGTTA_PATCH_MAX_ITEMS];
};

// scipy's tap index on a mirrored line (ni_interpolation.c) for the taps this kernel can ask for: -1 .. n + 1.  For n >= 3
// that is the reflection about 0 and n - 1; on a line of 1 or 2 samples the final clamp only moves taps of weight 0.
__device__ __forceinline__ int mirror_idx(int i, int n) {
  i = i < 0 ? -i : i;
  i = i >= n ? 2 * n - 2 - i : i;
  return min(max(i, 0), n - 1);
}

// cubic B-spline weights of the taps at offsets -1, 0, 1, 2 from floor(x), t = x - floor(x).  The outer two are written as
// cubes (scipy forms the last as 1 - the others in double): every weight then has a RELATIVE error bound in fp32.
__device__ __forceinline__ void bspline3_weights(float t, float *w) {
  const float u = 1.f - t;
  w[0] = u * u * u / 6.f;
  w[1] = (t * t * (t - 2.f) * 3.f + 4.f) / 6.f;
  w[2] = (u * u * (u - 2.f) * 3.f + 4.f) / 6.f;
  w[3] = t * t * t / 6.f;
}

template <int ORDER>
__global__ __launch_bounds__(256) void patch_sample_aug_kernel(const PatchItems items, float *__restrict__ image,
                                                               int64_t *__restrict__ labels, int PD, int PH, int PW) {
  const int w = (int)blockIdx.x * 64 + (int)threadIdx.x, h = (int)blockIdx.y * 4 + (int)threadIdx.y;
  const int d = (int)blockIdx.z % PD, b = (int)blockIdx.z / PD;
  if (w >= PW || h >= PH) return;
  const DgttaPatchItem &it = items.it[b];
  const int n[3] = {it.D, it.H, it.W};
  const int stride[3] = {it.H * it.W, it.W, 1};
  double x[3];
#pragma unroll
  for (int a = 0; a < 3; ++a)
    x[a] = (double)it.map[4 * a] * (double)d + (double)it.map[4 * a + 1] * (double)h + (double)it.map[4 * a + 2] * (double)w +
           (double)it.map[4 * a + 3];

  // ---- image
  constexpr int NT = ORDER == 3 ? 4 : 2;
  bool inside = true;
  int idx[3][NT];
  float wt[3][NT];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const bool in = x[a] >= 0.0 && x[a] <= (double)(n[a] - 1);      // false for NaN
    inside = inside && in;
    const double xc = in ? x[a] : 0.0, fl = floor(xc);
    const float t = (float)(xc - fl);
    const int j = (int)fl - (ORDER == 3 ? 1 : 0);
    if (ORDER == 3) {
      bspline3_weights(t, wt[a]);
    } else {
      wt[a][0] = 1.f - t;
      wt[a][1] = t;
    }
#pragma unroll
    for (int k = 0; k < NT; ++k) idx[a][k] = mirror_idx(j + k, n[a]) * stride[a];
  }
  const float *__restrict__ vol = it.image;
  float acc = 0.f;
#pragma unroll
  for (int i = 0; i < NT; ++i) {
    float acc_h = 0.f;
#pragma unroll
    for (int j = 0; j < NT; ++j) {
      const float *row = vol + (idx[0][i] + idx[1][j]);
      float acc_w = 0.f;
#pragma unroll
      for (int k = 0; k < NT; ++k) acc_w += wt[2][k] * row[idx[2][k]];
      acc_h += wt[1][j] * acc_w;
    }
    acc += wt[0][i] * acc_h;
  }
  const int64_t o = (((int64_t)b * PD + d) * PH + h) * PW + w;
  image[o] = inside ? acc : 0.f;

  // ---- label
  int lidx[3][2];
  bool lval[3][2];
  float lw[3][2];
#pragma unroll
  for (int a = 0; a < 3; ++a) {
    const double hi = (double)(n[a] + 1);
    const double xl = x[a] >= -2.0 ? (x[a] <= hi ? x[a] : hi) : -2.0;      // NaN -> -2: every corner outside
    const double fl = floor(xl);
    const float t = (float)(xl - fl);
    const int j = (int)fl;
    lw[a][0] = 1.f - t;
    lw[a][1] = t;
#pragma unroll
    for (int k = 0; k < 2; ++k) {
      lval[a][k] = j + k >= 0 && j + k < n[a];
      lidx[a][k] = min(max(j + k, 0), n[a] - 1) * stride[a];
    }
  }
  const float *__restrict__ lab = it.label;
  int cl[8];
  float cw[8];
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    const int i = c >> 2, j = (c >> 1) & 1, k = c & 1;
    const float v = lab[lidx[0][i] + lidx[1][j] + lidx[2][k]];
    cl[c] = lval[0][i] && lval[1][j] && lval[2][k] ? (int)v : 0;
    cw[c] = lw[0][i] * lw[1][j] * lw[2][k];
  }
  int best = 0;
#pragma unroll
  for (int c = 0; c < 8; ++c) {
    float mass = 0.f;
#pragma unroll
    for (int e = 0; e < 8; ++e) mass += cl[e] == cl[c] ? cw[e] : 0.f;
    best = cl[c] > best && mass >= 0.5f ? cl[c] : best;
  }
  labels[o] = (int64_t)best;
}

constexpr int HORIZON = 64;      // |z|^64 = 2.5e-37: below every fp32 sum it could enter

// One line per thread: element k of line (o, i) at (o * n + k) * inner + i.  src may equal dst.
__global__ __launch_bounds__(256) void bspline3_prefilter_kernel(const float *__restrict__ src, float *__restrict__ dst, int nlines,
                                                                 int n, int inner) {
  const int line = (int)blockIdx.x * 256 + (int)threadIdx.x;
  if (line >= nlines) return;
  const int o = line / inner, i = line % inner;
  const int64_t base = (int64_t)o * n * inner + i, st = inner;
  const float *s = src + base;
  float *c = dst + base;
  if (n == 1) {               // scipy leaves a line of one sample as it is
    c[0] = s[0];
    return;
  }
  const float z = -0.26794919243112270647f, gain = 6.f;
  // causal initialisation, mirror boundary (scipy ni_splines.c: _init_causal_mirror), the sum cut at HORIZON terms
  float z_n_1 = 0.f;
  if (n - 1 <= HORIZON) {
    z_n_1 = 1.f;
    for (int k = 0; k < n - 1; ++k) z_n_1 *= z;
  }
  float c0 = gain * s[0] + z_n_1 * (gain * s[(n - 1) * st]);
  float z_i = z;
  const int last = min(n - 2, HORIZON);
  for (int k = 1; k <= last; ++k) {
    c0 += z_i * (gain * s[k * st] + z_n_1 * (gain * s[(n - 1 - k) * st]));
    z_i *= z;
  }
  c0 /= 1.f - z_n_1 * z_n_1;
  float prev = c0;
  c[0] = c0;
  for (int k = 1; k < n; ++k) {
    prev = gain * s[k * st] + z * prev;
    c[k * st] = prev;
  }
  // anticausal pass (scipy: _init_anticausal_mirror)
  float cur = (z * c[(n - 2) * st] + prev) * z / (z * z - 1.f);
  c[(n - 1) * st] = cur;
  for (int k = n - 2; k >= 0; --k) {
    cur = z * (cur - c[k * st]);
    c[k * st] = cur;
  }
}

}  // namespace

extern "C" int dgtta_bspline3_prefilter(const float *src, float *dst, int D, int H, int W, void *stream) {
  DG_REQUIRE(src && dst, DGTTA_ERR_BADARG, "bspline3_prefilter: null pointer");
  DG_REQUIRE(D > 0 && H > 0 && W > 0, DGTTA_ERR_BADARG, "bspline3_prefilter: bad dims %d x %d x %d", D, H, W);
  DG_REQUIRE((int64_t)D * H * W < (1ll << 31), DGTTA_ERR_UNSUPPORTED, "bspline3_prefilter: 2^31 voxels or more");
  const hipStream_t st = (hipStream_t)stream;
  const int nl_d = H * W, nl_h = D * W, nl_w = D * H;
  hipLaunchKernelGGL(bspline3_prefilter_kernel, dim3(cdiv(nl_d, 256)), dim3(256), 0, st, src, dst, nl_d, D, H * W);
  hipLaunchKernelGGL(bspline3_prefilter_kernel, dim3(cdiv(nl_h, 256)), dim3(256), 0, st, (const float *)dst, dst, nl_h, H, W);
  hipLaunchKernelGGL(bspline3_prefilter_kernel, dim3(cdiv(nl_w, 256)), dim3(256), 0, st, (const float *)dst, dst, nl_w, W, 1);
  DG_CHECK_LAUNCH("bspline3_prefilter_kernel");
  return DGTTA_OK;
}

extern "C" int dgtta_patch_sample_aug(const DgttaPatchItem *items, int n_items, int PD, int PH, int PW, int order, float *image,
                                      int64_t *labels, void *stream) {
  DG_REQUIRE(items && image && labels, DGTTA_ERR_BADARG, "patch_sample_aug: null pointer");
  DG_REQUIRE(n_items >= 1 && n_items <= DGTTA_PATCH_MAX_ITEMS, DGTTA_ERR_BADARG, "patch_sample_aug: 1..%d items per launch (got %d)",
             DGTTA_PATCH_MAX_ITEMS, n_items);
  DG_REQUIRE(PD > 0 && PH > 0 && PW > 0, DGTTA_ERR_BADARG, "patch_sample_aug: bad patch %d x %d x %d", PD, PH, PW);
  DG_REQUIRE(order == 1 || order == 3, DGTTA_ERR_UNSUPPORTED, "patch_sample_aug: order %d not in {1, 3}", order);
  DG_REQUIRE((int64_t)PD * n_items <= 65535 && cdiv(PH, 4) <= 65535, DGTTA_ERR_UNSUPPORTED, "patch_sample_aug: patch too large for one grid");
  PatchItems args{};
  for (int b = 0; b < n_items; ++b) {
    const DgttaPatchItem &it = items[b];
    DG_REQUIRE(it.image && it.label, DGTTA_ERR_BADARG, "patch_sample_aug: item %d: null pointer", b);
    DG_REQUIRE(it.D > 0 && it.H > 0 && it.W > 0, DGTTA_ERR_BADARG, "patch_sample_aug: item %d: bad dims %d x %d x %d", b, it.D, it.H, it.W);
    DG_REQUIRE((int64_t)it.D * it.H * it.W < (1ll << 31), DGTTA_ERR_UNSUPPORTED, "patch_sample_aug: item %d: 2^31 voxels or more", b);
    for (int k = 0; k < 12; ++k) DG_REQUIRE(isfinite(it.map[k]), DGTTA_ERR_BADARG, "patch_sample_aug: item %d: map entry %d is not finite", b, k);
    args.it[b] = it;
  }
  const dim3 grid((unsigned)cdiv(PW, 64), (unsigned)cdiv(PH, 4), (unsigned)(PD * n_items)), block(64, 4);
  if (order == 3)
    hipLaunchKernelGGL(patch_sample_aug_kernel<3>, grid, block, 0, (hipStream_t)stream, args, image, labels, PD, PH, PW);
  else
    hipLaunchKernelGGL(patch_sample_aug_kernel<1>, grid, block, 0, (hipStream_t)stream, args, image, labels, PD, PH, PW);
  DG_CHECK_LAUNCH("patch_sample_aug_kernel");
  return DGTTA_OK;
}
