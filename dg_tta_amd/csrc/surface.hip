// Surface-distance metrics of the folder evaluation (tta/evaluation.py): per-label bounding boxes of two label maps, the surface
// voxels of one label inside a crop box, and the exact squared Euclidean distance transform to a set of sites.
#include "conv_api.h"

#include <limits.h>
#include <math.h>

namespace {

// ============================================================================ bounding boxes
constexpr int BB_MAXLAB = 1024;               // LDS table [nlab][6] ints: 24 KB

__global__ void bbox_init_kernel(int *__restrict__ boxes, int n6) {
  for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n6; i += gridDim.x * blockDim.x) boxes[i] = i % 6 < 3 ? INT_MAX : -1;
}

__device__ __forceinline__ void bbox_flush(int *sbox, int lab, const int *lo, const int *hi) {
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    atomicMin(&sbox[6 * lab + k], lo[k]);
    atomicMax(&sbox[6 * lab + 3 + k], hi[k]);
  }
}

// A thread keeps the box of the label it saw last in registers and goes to the LDS table only when the label changes (most
// voxels are background, and a thread's voxels of one organ come in runs); the table goes to global memory once per workgroup.
__global__ __launch_bounds__(256) void label_bboxes_kernel(const int64_t *__restrict__ a, const int64_t *__restrict__ b, int nlab,
                                                           int H, int W, int64_t total, int *__restrict__ boxes) {
  extern __shared__ int sbox[];               // [nlab][6]: lo d, h, w, hi d, h, w
  for (int i = threadIdx.x; i < 6 * nlab; i += blockDim.x) sbox[i] = i % 6 < 3 ? INT_MAX : -1;
  __syncthreads();
  int cur = -1, lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / W;
    const int p[3] = {(int)(r / H), (int)(r % H), (int)(i % W)};
#pragma unroll
    for (int m = 0; m < 2; ++m) {
      const int64_t lv = m ? b[i] : a[i];
      if ((uint64_t)lv >= (uint64_t)nlab) continue;       // a label outside the table has no box
      if ((int)lv != cur) {
        if (cur >= 0) bbox_flush(sbox, cur, lo, hi);
        cur = (int)lv;
#pragma unroll
        for (int k = 0; k < 3; ++k) lo[k] = hi[k] = p[k];
      } else {
#pragma unroll
        for (int k = 0; k < 3; ++k) lo[k] = min(lo[k], p[k]), hi[k] = max(hi[k], p[k]);
      }
    }
  }
  if (cur >= 0) bbox_flush(sbox, cur, lo, hi);
  __syncthreads();
  for (int l = threadIdx.x; l < nlab; l += blockDim.x)
    if (sbox[6 * l] <= sbox[6 * l + 3]) {
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        atomicMin(&boxes[6 * l + k], sbox[6 * l + k]);
        atomicMax(&boxes[6 * l + 3 + k], sbox[6 * l + 3 + k]);
      }
    }
}

// ============================================================================ surface of one label
// S(M) = voxels of M = (map == label) with a face neighbour outside M; outside the VOLUME counts as outside M, the crop box
// does not: neighbours are read from the full map.
__global__ void label_surface_kernel(const int64_t *__restrict__ map, int D, int H, int W, int64_t label, int d0, int h0, int w0,
                                     int ch, int cw, int64_t total, uint8_t *__restrict__ surf) {
  const int64_t HW = (int64_t)H * W;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = i / cw;
    const int d = d0 + (int)(r / ch), h = h0 + (int)(r % ch), w = w0 + (int)(i % cw);
    const int64_t c = ((int64_t)d * H + h) * W + w;
    bool s = false;
    if (map[c] == label)
      s = d == 0 || map[c - HW] != label || d == D - 1 || map[c + HW] != label ||
          h == 0 || map[c - W] != label || h == H - 1 || map[c + W] != label ||
          w == 0 || map[c - 1] != label || w == W - 1 || map[c + 1] != label;
    surf[i] = s ? 1 : 0;
  }
}

// ============================================================================ squared Euclidean distance transform
// One operator along one axis, three times (W, H, D):  out[i] = min_j ( in[j] + (s * (float)(i - j))^2 ), in fp32 in exactly
// this order: the product, its square, the add, the min (the build has -ffp-contract=off: no fused multiply-add).  The scan is
// the brute-force min-plus: O(n) per output, branch free, every trip count a dimension.  (float)(i - j) is carried as a float
// that is decremented by one per step, which is exact for these integers.
constexpr int EDT_MAX_AXIS = DGTTA_EDT_MAX_AXIS;
constexpr int EDT_R = 4;                      // outputs per thread and LDS read in the H / D passes
constexpr int EDT_W_TILE = 4096;              // floats of LDS per workgroup in the W pass

__device__ __forceinline__ float edt_term(float f, float s, float dj) {
  const float t = s * dj;
  return f + t * t;
}

// W pass: the lines are contiguous, a workgroup stages L whole lines (rows `ld` = n | 1 words apart, so that the lanes of a wave
// that spans several short lines read different banks) and thread (line, i) scans its line: the lanes of one line read the same
// LDS word, which broadcasts.  Starts the transform: a site is 0, everything else +inf.
__global__ __launch_bounds__(256) void edt_w_kernel(const uint8_t *__restrict__ site, float *__restrict__ out, int n, int L,
                                                    int64_t lines, float s) {
  extern __shared__ float tile[];             // [L][ld]
  const int ld = n | 1;
  const int64_t ntile = cdiv64(lines, L);
  for (int64_t t = blockIdx.x; t < ntile; t += gridDim.x) {
    const int64_t l0 = t * L;
    const int cnt = (int)(lines - l0 < L ? lines - l0 : L) * n;
    const uint8_t *sp = site + l0 * n;
    __syncthreads();                          // previous tile scanned
    for (int e = threadIdx.x; e < cnt; e += 256) tile[(e / n) * ld + e % n] = sp[e] ? 0.f : __builtin_inff();
    __syncthreads();
    for (int e = threadIdx.x; e < cnt; e += 256) {
      const float *row = tile + (e / n) * ld;
      float m = __builtin_inff(), dj = (float)(e % n);
      for (int j = 0; j < n; ++j) {
        m = fminf(m, edt_term(row[j], s, dj));
        dj -= 1.f;
      }
      out[l0 * n + e] = m;
    }
  }
}

// H and D passes over [outer][n][inner] (inner > 1 elements between neighbours of a line): TI adjacent lines in LDS, the lanes
// along `inner` so that global loads and stores are coalesced and LDS reads conflict free; a thread carries EDT_R outputs of
// its line per LDS read.
template <int TI>
__global__ __launch_bounds__(256) void edt_axis_kernel(const float *__restrict__ in, float *__restrict__ out, int n, int64_t inner,
                                                       int64_t outer, float s) {
  extern __shared__ float tile[];             // [n][TI]
  constexpr int G = 256 / TI;
  const int t = threadIdx.x % TI, g = threadIdx.x / TI;
  const int64_t tin = cdiv64(inner, TI), ntile = outer * tin;
  for (int64_t tt = blockIdx.x; tt < ntile; tt += gridDim.x) {
    const int64_t o = tt / tin, c = (tt % tin) * TI + t;
    const bool ok = c < inner;
    const int64_t base = o * n * inner + c;
    __syncthreads();                          // previous tile scanned
    for (int j = g; j < n; j += G) tile[j * TI + t] = ok ? in[base + j * inner] : __builtin_inff();
    __syncthreads();
    for (int i0 = g; i0 < n; i0 += G * EDT_R) {
      float m[EDT_R], dj[EDT_R];
#pragma unroll
      for (int k = 0; k < EDT_R; ++k) m[k] = __builtin_inff(), dj[k] = (float)(i0 + k * G);
      for (int j = 0; j < n; ++j) {
        const float f = tile[j * TI + t];
#pragma unroll
        for (int k = 0; k < EDT_R; ++k) {
          m[k] = fminf(m[k], edt_term(f, s, dj[k]));
          dj[k] -= 1.f;
        }
      }
#pragma unroll
      for (int k = 0; k < EDT_R; ++k) {
        const int i = i0 + k * G;
        if (ok && i < n) out[base + i * inner] = m[k];
      }
    }
  }
}

int edt_axis_launch(const float *in, float *out, int n, int64_t inner, int64_t outer, float s, hipStream_t st) {
  // the widest tile whose n lines fit 64 KB of LDS, no wider than the lines there are
  int ti = n <= 256 ? 64 : n <= 512 ? 32 : 16;
  while (ti > 16 && inner <= ti / 2) ti /= 2;
  const int64_t ntile = outer * cdiv64(inner, ti);
  const dim3 grid((unsigned)(ntile < 16384 ? ntile : 16384));
  const size_t lds = (size_t)n * ti * sizeof(float);
  if (ti == 64)
    hipLaunchKernelGGL(edt_axis_kernel<64>, grid, dim3(256), lds, st, in, out, n, inner, outer, s);
  else if (ti == 32)
    hipLaunchKernelGGL(edt_axis_kernel<32>, grid, dim3(256), lds, st, in, out, n, inner, outer, s);
  else
    hipLaunchKernelGGL(edt_axis_kernel<16>, grid, dim3(256), lds, st, in, out, n, inner, outer, s);
  DG_CHECK_LAUNCH("edt_axis_kernel");
  return DGTTA_OK;
}

bool spacing_ok(float s) { return s > 0.f && s <= 1e6f; }      // also false for NaN; (s n)^2 stays far below FLT_MAX

}  // namespace

extern "C" int dgtta_label_bboxes(const int64_t *a, const int64_t *b, int D, int H, int W, int nlab, int *boxes, void *stream) {
  DG_REQUIRE(a && b && boxes && D > 0 && H > 0 && W > 0 && nlab > 0, DGTTA_ERR_BADARG, "label_bboxes: bad args");
  DG_REQUIRE(nlab <= BB_MAXLAB, DGTTA_ERR_UNSUPPORTED, "label_bboxes: %d labels (at most %d)", nlab, BB_MAXLAB);
  const int64_t total = (int64_t)D * H * W;
  hipLaunchKernelGGL(bbox_init_kernel, dim3(gs_blocks(6 * nlab)), dim3(256), 0, (hipStream_t)stream, boxes, 6 * nlab);
  DG_CHECK_LAUNCH("bbox_init_kernel");
  hipLaunchKernelGGL(label_bboxes_kernel, dim3(gs_blocks(total, 2048)), dim3(256), 6 * nlab * sizeof(int), (hipStream_t)stream, a, b,
                     nlab, H, W, total, boxes);
  DG_CHECK_LAUNCH("label_bboxes_kernel");
  return DGTTA_OK;
}

extern "C" int dgtta_label_surface(const int64_t *map, int D, int H, int W, int64_t label, int d0, int h0, int w0, int cd, int ch,
                                   int cw, uint8_t *surf, void *stream) {
  DG_REQUIRE(map && surf && D > 0 && H > 0 && W > 0, DGTTA_ERR_BADARG, "label_surface: bad args");
  DG_REQUIRE(cd > 0 && ch > 0 && cw > 0 && d0 >= 0 && h0 >= 0 && w0 >= 0 && d0 <= D - cd && h0 <= H - ch && w0 <= W - cw,
             DGTTA_ERR_BADARG, "label_surface: box [%d+%d, %d+%d, %d+%d] outside the %d x %d x %d volume", d0, cd, h0, ch, w0, cw, D,
             H, W);
  const int64_t total = (int64_t)cd * ch * cw;
  hipLaunchKernelGGL(label_surface_kernel, dim3(gs_blocks(total)), dim3(256), 0, (hipStream_t)stream, map, D, H, W, label, d0, h0, w0,
                     ch, cw, total, surf);
  DG_CHECK_LAUNCH("label_surface_kernel");
  return DGTTA_OK;
}

extern "C" size_t dgtta_edt_ws_bytes(int D, int H, int W) {
  if (D <= 0 || H <= 0 || W <= 0) return 0;
  return align_up((size_t)D * (size_t)H * (size_t)W * sizeof(float), 256);
}

extern "C" int dgtta_edt_sq(const uint8_t *site, float *dist2, void *ws, size_t ws_bytes, int D, int H, int W, float sd, float sh,
                            float sw, void *stream) {
  DG_REQUIRE(site && dist2 && ws && D > 0 && H > 0 && W > 0, DGTTA_ERR_BADARG, "edt_sq: bad args");
  DG_REQUIRE(spacing_ok(sd) && spacing_ok(sh) && spacing_ok(sw), DGTTA_ERR_BADARG, "edt_sq: spacing (%g, %g, %g) must be in (0, 1e6]",
             (double)sd, (double)sh, (double)sw);
  DG_REQUIRE(D <= EDT_MAX_AXIS && H <= EDT_MAX_AXIS && W <= EDT_MAX_AXIS, DGTTA_ERR_UNSUPPORTED,
             "edt_sq: %d x %d x %d (at most %d voxels per axis)", D, H, W, EDT_MAX_AXIS);
  DG_REQUIRE(ws_bytes >= dgtta_edt_ws_bytes(D, H, W), DGTTA_ERR_WORKSPACE, "edt_sq: workspace %zu < %zu", ws_bytes,
             dgtta_edt_ws_bytes(D, H, W));
  DG_REQUIRE(((uintptr_t)ws & 3) == 0 && ((uintptr_t)dist2 & 3) == 0, DGTTA_ERR_BADARG, "edt_sq: buffers must be 4-byte aligned");
  const hipStream_t st = (hipStream_t)stream;
  float *tmp = (float *)ws;
  const int64_t lines = (int64_t)D * H;
  const int L = EDT_W_TILE / (W | 1) > 0 ? EDT_W_TILE / (W | 1) : 1;
  const int64_t ntile = cdiv64(lines, L);
  hipLaunchKernelGGL(edt_w_kernel, dim3((unsigned)(ntile < 16384 ? ntile : 16384)), dim3(256), (size_t)L * (W | 1) * sizeof(float), st,
                     site, dist2, W, L, lines, sw);
  DG_CHECK_LAUNCH("edt_w_kernel");
  int rc = edt_axis_launch(dist2, tmp, H, W, D, sh, st);
  if (rc != DGTTA_OK) return rc;
  return edt_axis_launch(tmp, dist2, D, (int64_t)H * W, 1, sd, st);
}
