// nnU-Net's optimiser step for source-domain pre-training: gradient-norm clipping + SGD with (Nesterov) momentum and L2
// weight decay, dampening 0.  Two entry points, both multi-tensor in the manner of adamw.hip (up to 32 tensors per launch
// through the kernel-argument buffer, no device-side table, nothing allocated here):
//   dgtta_grad_sumsq  sum over every gradient element of g*g -> one fp32 device scalar.  HBM-bound: 1 read per element.
//                     Reproducible bit for bit: every workgroup writes ONE double partial into the caller's workspace at a
//                     slot fixed by (tensor order, chunk index); one last workgroup adds the slots in a fixed order in
//                     double.  No floating-point atomics, no hand-off between workgroups inside a launch.
//   dgtta_sgd_step    one fused pass, HBM-bound: 3 reads (p, g, buf) + 2 writes (p, buf) of fp32 per element; the clip
//                     coefficient is computed in the kernel from the device scalar, so clipping costs no host synchronisation.
// Operation order = torch.nn.utils.clip_grad_norm_ followed by torch.optim.SGD(dampening=0) (the file is built with
// -ffp-contract=off: no operation below is fused into an FMA):
//   norm = sqrt(sumsq) * inv_scale;  coef = min(1, max_norm / (norm + 1e-6))          (coef = 1 without a sumsq pointer)
//   g' = (g * inv_scale) * coef;  d = g' + wd * p;  buf = first_step ? d : mu * buf + d
//   u = nesterov ? d + mu * buf : buf;  p = p - lr * u
#include "common.h"
#include <math.h>

namespace {

constexpr int TPL = 32;           // tensors per launch
constexpr int CHUNK = 256 * 16;   // elements per workgroup

struct SgdArgs {
  float *p[TPL];
  const float *g[TPL];
  float *buf[TPL];
  int64_t n[TPL];
  int blk_start[TPL + 1];  // first workgroup of tensor i
};

struct SumsqArgs {
  const float *g[TPL];
  int64_t n[TPL];
  int blk_start[TPL + 1];
};

__device__ __forceinline__ bool aligned16(const void *a) { return ((uintptr_t)a & 15) == 0; }

// partial[part_base + blockIdx.x] = sum of squares of this workgroup's chunk.  Per thread: 16 squares added in fp32 in index
// order (4 float4 of a full aligned chunk, or 16 strided scalars: which of the two depends only on the tensor's address and
// length, never on the run); across the workgroup: a fixed tree in double.
__global__ __launch_bounds__(256) void grad_sumsq_partial_kernel(SumsqArgs a, int nt, double *__restrict__ partial,
                                                                 int64_t part_base) {
  __shared__ double red[4];
  int t = 0;
  while (t + 1 < nt && (int)blockIdx.x >= a.blk_start[t + 1]) ++t;
  const int64_t base = (int64_t)((int)blockIdx.x - a.blk_start[t]) * CHUNK;
  const float *g = a.g[t];
  const int64_t n = a.n[t];
  float s = 0.f;
  if (base + CHUNK <= n && aligned16(g)) {
    const float4 *g4 = reinterpret_cast<const float4 *>(g + base);
#pragma unroll
    for (int k = 0; k < CHUNK / 1024; ++k) {
      const float4 v = g4[k * 256 + threadIdx.x];
      s += v.x * v.x;
      s += v.y * v.y;
      s += v.z * v.z;
      s += v.w * v.w;
    }
  } else {
#pragma unroll 4
    for (int k = 0; k < CHUNK / 256; ++k) {
      const int64_t i = base + k * 256 + threadIdx.x;
      if (i < n) {
        const float v = g[i];
        s += v * v;
      }
    }
  }
  double d = wave_sum_d((double)s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = d;
  __syncthreads();
  if (threadIdx.x == 0) partial[part_base + blockIdx.x] = ((red[0] + red[1]) + red[2]) + red[3];
}

// One workgroup: thread t adds slots t, t + 256, ... in double, then the same fixed tree; the fp32 result is rounded once.
__global__ __launch_bounds__(256) void grad_sumsq_final_kernel(const double *__restrict__ partial, int64_t nparts,
                                                               float *__restrict__ out) {
  __shared__ double red[4];
  double s = 0.0;
  for (int64_t i = threadIdx.x; i < nparts; i += 256) s += partial[i];
  s = wave_sum_d(s);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) out[0] = (float)(((red[0] + red[1]) + red[2]) + red[3]);
}

__device__ __forceinline__ void sgd_update(float &p, float g, float &buf, float inv_scale, float coef, float wd, float mu,
                                           float lr, bool first_step, bool nesterov) {
  const float gc = (g * inv_scale) * coef;
  const float d = gc + wd * p;
  buf = first_step ? d : mu * buf + d;
  const float u = nesterov ? d + mu * buf : buf;
  p = p - lr * u;
}

__global__ __launch_bounds__(256) void sgd_kernel(SgdArgs a, int nt, float lr, float mu, float wd, int nesterov, int first_step,
                                                  float inv_scale, const float *__restrict__ sumsq, float max_norm,
                                                  const int *__restrict__ skip) {
  if (skip != nullptr && *skip != 0) return;      // a gradient overflowed (fp16 loss scale too high): the step is skipped
  float coef = 1.0f;
  if (sumsq != nullptr) {
    const float norm = sqrtf(*sumsq) * inv_scale;
    const float c = max_norm / (norm + 1e-6f);
    coef = c > 1.0f ? 1.0f : c;                   // a NaN norm stays NaN, as torch.clamp(max=1) leaves it
  }
  int t = 0;
  while (t + 1 < nt && (int)blockIdx.x >= a.blk_start[t + 1]) ++t;
  const int64_t base = (int64_t)((int)blockIdx.x - a.blk_start[t]) * CHUNK;
  float *p = a.p[t], *buf = a.buf[t];
  const float *g = a.g[t];
  const int64_t n = a.n[t];
  const bool first = first_step != 0, nest = nesterov != 0;
  if (base + CHUNK <= n && aligned16(p) && aligned16(g) && aligned16(buf)) {
    float4 *p4 = reinterpret_cast<float4 *>(p + base), *b4 = reinterpret_cast<float4 *>(buf + base);
    const float4 *g4 = reinterpret_cast<const float4 *>(g + base);
#pragma unroll
    for (int k = 0; k < CHUNK / 1024; ++k) {
      const int j = k * 256 + threadIdx.x;
      float4 pv = p4[j], bv = make_float4(0.f, 0.f, 0.f, 0.f);
      const float4 gv = g4[j];
      if (!first) bv = b4[j];                      // the first step never reads the (uninitialised) buffer
      sgd_update(pv.x, gv.x, bv.x, inv_scale, coef, wd, mu, lr, first, nest);
      sgd_update(pv.y, gv.y, bv.y, inv_scale, coef, wd, mu, lr, first, nest);
      sgd_update(pv.z, gv.z, bv.z, inv_scale, coef, wd, mu, lr, first, nest);
      sgd_update(pv.w, gv.w, bv.w, inv_scale, coef, wd, mu, lr, first, nest);
      p4[j] = pv;
      b4[j] = bv;
    }
  } else {
#pragma unroll 4
    for (int k = 0; k < CHUNK / 256; ++k) {
      const int64_t i = base + k * 256 + threadIdx.x;
      if (i < n) {
        float pi = p[i], bi = first ? 0.f : buf[i];
        sgd_update(pi, g[i], bi, inv_scale, coef, wd, mu, lr, first, nest);
        p[i] = pi;
        buf[i] = bi;
      }
    }
  }
}

// workgroups a tensor of n elements takes; 0 for an empty / negative count
inline uint64_t chunks_of(int64_t n) { return n > 0 ? ((uint64_t)n + CHUNK - 1) / CHUNK : 0; }

}  // namespace

extern "C" size_t dgtta_grad_sumsq_ws_bytes(int64_t total_elements, int ntensors) {
  // every tensor takes ceil(n / CHUNK) slots: at most total / CHUNK + one ragged chunk per tensor; one spare slot keeps the
  // size non-zero.  Unsigned arithmetic: 2^63 elements and 2^31 tensors stay far below 2^64 bytes.
  const uint64_t slots = (total_elements > 0 ? (uint64_t)total_elements / CHUNK : 0) + (ntensors > 0 ? (uint64_t)ntensors : 0) + 1;
  return (size_t)(slots * sizeof(double));
}

extern "C" int dgtta_grad_sumsq(const float *const *h_g, const int64_t *h_n, int ntensors, float *out, void *ws,
                                size_t ws_bytes, void *stream) {
  DG_REQUIRE(h_g && h_n && out && ws, DGTTA_ERR_BADARG, "grad_sumsq: null pointer");
  DG_REQUIRE(ntensors >= 0, DGTTA_ERR_BADARG, "grad_sumsq: bad ntensors");
  DG_REQUIRE(((uintptr_t)ws & 7) == 0, DGTTA_ERR_WORKSPACE, "grad_sumsq: workspace must be 8-byte aligned");
  uint64_t need = 0;
  for (int i = 0; i < ntensors; ++i)
    if (h_g[i] != nullptr) {
      DG_REQUIRE(h_n[i] >= 0, DGTTA_ERR_BADARG, "grad_sumsq: negative element count of tensor %d", i);
      need += chunks_of(h_n[i]);
    }
  DG_REQUIRE(need * sizeof(double) <= ws_bytes, DGTTA_ERR_WORKSPACE,
             "grad_sumsq: workspace of %zu bytes, %llu needed (dgtta_grad_sumsq_ws_bytes)", ws_bytes,
             (unsigned long long)(need * sizeof(double)));
  hipStream_t st = (hipStream_t)stream;
  double *partial = (double *)ws;
  int64_t part_base = 0;
  int i = 0;
  while (i < ntensors) {
    SumsqArgs a;
    int nt = 0;
    int64_t blocks = 0;
    while (i < ntensors && nt < TPL) {
      if (h_g[i] != nullptr && h_n[i] > 0) {
        const int64_t c = (int64_t)chunks_of(h_n[i]);
        if (blocks + c > 0x7fffffff) {            // the grid index is an int: this tensor opens the next launch
          DG_REQUIRE(nt > 0, DGTTA_ERR_UNSUPPORTED, "grad_sumsq: tensor %d has more than 2^31 chunks", i);
          break;
        }
        a.g[nt] = h_g[i];
        a.n[nt] = h_n[i];
        a.blk_start[nt] = (int)blocks;
        blocks += c;
        ++nt;
      }
      ++i;
    }
    if (nt == 0) break;
    a.blk_start[nt] = (int)blocks;
    hipLaunchKernelGGL(grad_sumsq_partial_kernel, dim3((unsigned)blocks), dim3(256), 0, st, a, nt, partial, part_base);
    DG_CHECK_LAUNCH("grad_sumsq_partial_kernel");
    part_base += blocks;
  }
  hipLaunchKernelGGL(grad_sumsq_final_kernel, dim3(1), dim3(256), 0, st, partial, part_base, out);
  DG_CHECK_LAUNCH("grad_sumsq_final_kernel");
  return DGTTA_OK;
}

extern "C" int dgtta_sgd_step(float *const *h_p, const float *const *h_g, float *const *h_buf, const int64_t *h_n,
                              int ntensors, float lr, float momentum, float weight_decay, int nesterov, int first_step,
                              float grad_scale, const float *sumsq, float max_norm, const int *skip_if_nonzero,
                              void *stream) {
  DG_REQUIRE(h_p && h_g && h_buf && h_n, DGTTA_ERR_BADARG, "sgd_step: null table");
  DG_REQUIRE(ntensors >= 0, DGTTA_ERR_BADARG, "sgd_step: bad ntensors");
  DG_REQUIRE(grad_scale > 0.f, DGTTA_ERR_BADARG, "sgd_step: grad_scale must be positive (1 = gradients are unscaled)");
  DG_REQUIRE(sumsq == nullptr || max_norm > 0.f, DGTTA_ERR_BADARG, "sgd_step: max_norm must be positive when sumsq is given");
  hipStream_t st = (hipStream_t)stream;
  int i = 0;
  while (i < ntensors) {
    SgdArgs a;
    int nt = 0;
    int64_t blocks = 0;
    while (i < ntensors && nt < TPL) {
      if (h_g[i] != nullptr && h_n[i] > 0) {
        DG_REQUIRE(h_p[i] && h_buf[i], DGTTA_ERR_BADARG, "sgd_step: null tensor %d", i);
        const int64_t c = (int64_t)chunks_of(h_n[i]);
        if (blocks + c > 0x7fffffff) {
          DG_REQUIRE(nt > 0, DGTTA_ERR_UNSUPPORTED, "sgd_step: tensor %d has more than 2^31 chunks", i);
          break;
        }
        a.p[nt] = h_p[i];
        a.g[nt] = h_g[i];
        a.buf[nt] = h_buf[i];
        a.n[nt] = h_n[i];
        a.blk_start[nt] = (int)blocks;
        blocks += c;
        ++nt;
      }
      ++i;
    }
    if (nt == 0) break;
    a.blk_start[nt] = (int)blocks;
    hipLaunchKernelGGL(sgd_kernel, dim3((unsigned)blocks), dim3(256), 0, st, a, nt, lr, momentum, weight_decay, nesterov,
                       first_step, 1.0f / grad_scale, sumsq, max_norm, skip_if_nonzero);
    DG_CHECK_LAUNCH("sgd_kernel");
  }
  return DGTTA_OK;
}
