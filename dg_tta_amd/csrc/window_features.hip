// Sliding-window inference in FEATURE space (round 5; BASELINE config 3); window_logits.hip is the
// logit-space form it replaces.
//
// What the reference does (nnunetv2==2.2.1 predict_sliding_window_return_logits, reached from
// dg_tta/tta/nnunet_utils.py:116-125, 208-230; ensemble loop dg_tta/tta/tta.py:396-413): every window's logits over ALL
// pretrain classes are multiplied by the Gaussian importance map and added into a [classes, X, Y, Z] volume; the volume is
// divided by the summed weights, the members' volumes are averaged and the label map is the argmax.
//
// The segmentation head is a 1x1x1 convolution - LINEAR - and it is the last thing in the network:
//     sum_w g_w(v) (W z_w(v) + b) = W (sum_w g_w(v) z_w(v)) + b sum_w g_w(v).
// So the volume-sized accumulator can hold the 32 Gaussian-weighted FEATURE channels of the last decoder block instead of
// the 105 logits, and the head runs ONCE per voxel at the end, fused with the argmax:
//   * read-modify-write per window voxel: 64 B of features + 2 x 128 B instead of 64 B + 2 x 420 B (2.8x less HBM traffic in
//     the pass that was 20 % of a member's time: 343 windows x 1.9 GB at 512^3);
//   * accumulator of a 512^3 volume: 16 GiB per member instead of 52.5 GiB - and a member needs its own (the members' heads
//     differ), so an ensemble of three is 48 GiB: still below ONE logits volume;
//   * the 105-class volume never exists: the label map is argmax_c sum_m (W_m F_m(v) + b_m n(v)) straight from the features
//     (no division: n(v) > 0 is shared by all classes and members).
// Floating point: the sums are re-associated (fp32 throughout; products g * z are exact up to one rounding, the head runs on
// fp32 features with the fp32 weights instead of on 16-bit features window by window), so labels can differ from the
// logits-space accumulator where the top-2 margin is at rounding level - tests/test_inference.py compares both forms with the
// CPU restatement outside such ties.  nnU-Net itself is absent from /root/reference: this stage is "parity unpinned" either way.
//
// Layout: ONE accumulate kernel template (feature_accumulate_kernel<T, NS, NORM, MIR>: storage type, windows per launch, folded
// InstanceNorm apply, mirrored source) behind one host launcher that the five dgtta_feature_window_accumulate* entries forward to;
// the window's place in the volume, its checks and the index arithmetic are window_api.h's, shared with window_logits.hip.  Then the
// head kernels that read the accumulator (argmax, softmax, region label map, export chunk).
#include "gfx950.h"
#include "instnorm_math.h"
#include "window_api.h"

namespace {

constexpr int WF_CIN = 32;

// 4 channels of a voxel as floats
template <typename T>
__device__ __forceinline__ void wf_load4(const T *p, float (&f)[4]);
template <>
__device__ __forceinline__ void wf_load4<float>(const float *p, float (&f)[4]) {
  const float4 v = *reinterpret_cast<const float4 *>(p);
  f[0] = v.x, f[1] = v.y, f[2] = v.z, f[3] = v.w;
}
template <>
__device__ __forceinline__ void wf_load4<bf16_t>(const bf16_t *p, float (&f)[4]) {
  const uint2 v = *reinterpret_cast<const uint2 *>(p);
  f[0] = __uint_as_float(v.x << 16), f[1] = __uint_as_float(v.x & 0xffff0000u);
  f[2] = __uint_as_float(v.y << 16), f[3] = __uint_as_float(v.y & 0xffff0000u);
}
template <>
__device__ __forceinline__ void wf_load4<f16_t>(const f16_t *p, float (&f)[4]) {
  const uint2 v = *reinterpret_cast<const uint2 *>(p);
  f[0] = f16_to_f32((unsigned short)(v.x & 0xffffu)), f[1] = f16_to_f32((unsigned short)(v.x >> 16));
  f[2] = f16_to_f32((unsigned short)(v.y & 0xffffu)), f[3] = f16_to_f32((unsigned short)(v.y >> 16));
}

// value -> storage type T and back (what the network's apply pass writes and the head would read)
template <typename T>
__device__ __forceinline__ float wf_round(float v);
template <>
__device__ __forceinline__ float wf_round<float>(float v) { return v; }
template <>
__device__ __forceinline__ float wf_round<bf16_t>(float v) { return bf16_to_f32(f32_to_bf16(v)); }
template <>
__device__ __forceinline__ float wf_round<f16_t>(float v) { return f16_to_f32(f32_to_f16(v)); }

// The NS windows of a launch: a whole window (NS = 1, zoff 0), or the windows of one network pass that cover a SEGMENT of the last axis
struct WfSources {
  const void *src[4];            // window k: [PD][PH][PW][32]
  const float *mean_rstd[4];     // NORM: the window's statistics [32][2]
  int zoff[4];                   // the segment's first voxel along the last axis, in window k's coordinates
};

// facc[(x0 + pd, y0 + ph, z0 + zz)][c] += gauss[p_k] * z_k[p_k][c], nsum[..] += gauss[p_k] over the [PD][PH][SL] voxels of a segment
// of the last axis that starts at z0 in the volume and at zoff[k] in window k (p_k = (pd, ph, zoff[k] + zz)); a whole window is the
// segment SL = PW, zoff = 0.  8 threads per voxel, 4 channels each: every load and store instruction of a wave covers one contiguous
// run (z: 512 B, facc: 1 KiB; a row is contiguous in the volume along its last axis).  A launch touches every accumulator element
// once - overlapping windows are separate launches in stream order, as in the logits-space form - unless they overlap along the
// last axis only (consecutive origins of a sliding-window row): then NS > 1 windows share a launch per segment, every voxel receives
// the contributions of all NS windows that cover it, added in window order in registers - (acc + t_0) + t_1: the bits the one-window
// launches produce - and the accumulator is read and written ONCE instead of NS times.  With 50 % overlap a row of 7 windows is 8
// half-window segments: 57 % of the read-modify-write traffic.
// NORM: the sources are raw conv outputs y of the last block and its InstanceNorm + LeakyReLU apply is folded in: z = round_T(lrelu(y *
// alpha + beta')) is formed in registers (alpha = rstd * gamma, beta' = beta - mean * alpha: the arithmetic of in_apply_vec_kernel, so
// the SAME z values) and never written - the apply pass (read y, write z) and the read of z disappear for the layer in front of the
// head: 64 + 256 B per voxel instead of 128 + 320.  No backward exists in inference, so nothing else needs that z.
// MIR (a mirrored pass of nnU-Net's test-time mirroring, NS = 1 only): the thread-to-destination mapping and gauss[p] stay, the source
// is read at the mirrored voxel - a wave row's 512 B of z are the same run, reversed voxel by voxel when the last axis is flipped.
template <typename T, int NS, bool NORM, bool MIR>
__global__ __launch_bounds__(256) void feature_accumulate_kernel(WfSources ws, const float *__restrict__ gamma,
                                                                 const float *__restrict__ beta, float slope,
                                                                 const float *__restrict__ gauss, float *__restrict__ facc,
                                                                 float *__restrict__ nsum, WindowPlace wp, int SL, int64_t total) {
  static_assert(!MIR || NS == 1, "mirrored passes go one window per launch");
  __shared__ float sal[NS][WF_CIN], sbe[NS][WF_CIN];      // the windows' per-channel constants, once per workgroup
  if (NORM) {
    if (threadIdx.x < NS * WF_CIN) {
      const int k = threadIdx.x / WF_CIN, c = threadIdx.x % WF_CIN;
      const float al = in_alpha(ws.mean_rstd[k][c * 2 + 1], gamma[c]);
      sal[k][c] = al;
      sbe[k][c] = in_beta(beta[c], ws.mean_rstd[k][c * 2], al);
    }
    __syncthreads();
  }
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= total) return;
  const int q = (int)(i & 7);
  const WindowVoxel s = wp_voxel(i >> 3, wp.PH, SL);      // voxel of the segment [PD][PH][SL]
  const int64_t v = wp_volume(wp, s.pd, s.ph, s.pw);
  float4 *dst = reinterpret_cast<float4 *>(facc + v * WF_CIN + q * 4);
  float4 a = *dst;
  float n = (q == 0 && nsum) ? nsum[v] : 0.f;
  float f[NS][4], g[NS];
#pragma unroll
  for (int k = 0; k < NS; ++k) {             // all loads first
    const int pw = ws.zoff[k] + s.pw;
    g[k] = gauss[wp_window(wp, s.pd, s.ph, pw)];
    wf_load4<T>(reinterpret_cast<const T *>(ws.src[k]) + wp_source<MIR>(wp, s.pd, s.ph, pw) * WF_CIN + q * 4, f[k]);
  }
#pragma unroll
  for (int k = 0; k < NS; ++k) {
    float zv[4];
#pragma unroll
    for (int e = 0; e < 4; ++e) zv[e] = NORM ? wf_round<T>(in_fwd(f[k][e], sal[k][q * 4 + e], sbe[k][q * 4 + e], slope)) : f[k][e];
    a.x += g[k] * zv[0], a.y += g[k] * zv[1], a.z += g[k] * zv[2], a.w += g[k] * zv[3];
    n += g[k];
  }
  *dst = a;
  if (q == 0 && nsum) nsum[v] = n;
}

// Label map from the members' feature accumulators: argmax_c sum_m (W_m[c] . F_m(v)) + n(v) bsum[c], bsum = sum_m b_m (formed
// by the caller).  One thread per voxel; a member's 32 features sit in registers, the weights are wave-uniform (scalar
// loads).  With several members the classes' partial sums wait in LDS ([C][256] floats, own column per thread: no bank
// conflicts, no barrier); with one member they are compared as they are produced.  First maximum wins, as argmax does.
__global__ __launch_bounds__(256) void feature_head_argmax_kernel(const float *__restrict__ facc, int64_t member_stride,
                                                                  const float *__restrict__ nsum, const float *__restrict__ w,
                                                                  const float *__restrict__ bsum, int M, int C, int64_t V,
                                                                  int64_t *__restrict__ amax) {
  extern __shared__ float part[];      // [C][256] when M > 1
  const int tid = threadIdx.x;
  for (int64_t v0 = (int64_t)blockIdx.x * 256; v0 < V; v0 += (int64_t)gridDim.x * 256) {
    const int64_t v = v0 + tid < V ? v0 + tid : V - 1;      // (the tail repeats the last voxel: no divergent exit above LDS use)
    const float n = nsum[v];
    float best = -INFINITY;
    int bi = 0;
    for (int m = 0; m < M; ++m) {
      float f[WF_CIN];
      const float4 *src = reinterpret_cast<const float4 *>(facc + m * member_stride + v * WF_CIN);
#pragma unroll
      for (int k = 0; k < WF_CIN / 4; ++k) {
        const float4 t = src[k];
        f[4 * k] = t.x, f[4 * k + 1] = t.y, f[4 * k + 2] = t.z, f[4 * k + 3] = t.w;
      }
      const float *wm = w + (int64_t)m * C * WF_CIN;
      for (int c = 0; c < C; ++c) {
        // four independent FMA chains over the channels (a single chain of 32 waits for itself)
        float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
#pragma unroll
        for (int k = 0; k < WF_CIN; k += 4) {
          s0 = fmaf(wm[c * WF_CIN + k], f[k], s0);
          s1 = fmaf(wm[c * WF_CIN + k + 1], f[k + 1], s1);
          s2 = fmaf(wm[c * WF_CIN + k + 2], f[k + 2], s2);
          s3 = fmaf(wm[c * WF_CIN + k + 3], f[k + 3], s3);
        }
        float s = (s0 + s1) + (s2 + s3);
        if (m == 0) s += n * bsum[c];
        else s += part[c * 256 + tid];
        if (m + 1 < M) {
          part[c * 256 + tid] = s;
        } else if (s > best) {
          best = s;
          bi = c;
        }
      }
    }
    if (v0 + tid < V) amax[v] = bi;
  }
}

// The same on the fp32 matrix cores (v_mfma_f32_32x32x2_f32: M = 32 classes, N = 32 voxels, K = the 32 channels of every member in
// turn): a wave owns 32 voxels, the weights of all members sit in LDS ([member][class, padded to a multiple of 32][36 floats]: the
// 144-byte pitch keeps the 16-byte reads of 8 consecutive class rows on distinct bank groups), a lane's 16 bytes of features /
// weights feed four instructions (lane half h holds channels 8 s + 4 h .. + 3 of k-step s, as conv_common.h's fp32 mfma_step).
// Accumulators start at n(v) bsum[c]; the members add up in the accumulators (no LDS partials).  C/D map: a lane holds voxel
// lane & 31 and classes 32 cb + (q & 3) + 8 (q >> 2) + 4 (lane >> 5) - ascending in (cb, q), so a strict comparison in that order
// keeps the first maximum; the two lane halves of a voxel are merged with the lower class winning a tie.
// Measured at 512^3 x 105 classes (profiles/tools/headargmax_bench.py): one member 14.3 ms (vector-ALU kernel 15.5: the per-tile
// initialisation and argmax scan cost as much as one member's products), the plan's ensemble of three 29.0 ms against 179 ms - the
// vector-ALU kernel keeps several members' partial sums in LDS and is bound by that traffic; here a further member is 7.3 ms of MFMAs.
constexpr int WF_WPITCH = 36;

// The sequential scan's rule (best = -inf, class 0; strictly greater replaces; NaNs never do) over a tile's accumulators, per lane
// half and then merged; every lane of a voxel ends with the voxel's (best, bi).
template <int NCB>
__device__ __forceinline__ void wf_first_max(const f32x16_t (&acc)[NCB], int C, int h, float &best, int &bi) {
  best = -INFINITY;
  bi = 4 * h < C ? 4 * h : 0x7fffffff;      // this half's first class
#pragma unroll
  for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int c = cb * 32 + (q & 3) + 8 * (q >> 2) + 4 * h;
      const float x = acc[cb][q];
      if ((cb + 1 < NCB || c < C) && x > best) {      // (only the last class block can hold padding: C > 32 (NCB - 1))
        best = x;
        bi = c;
      }
    }
  const float ob = __shfl_xor(best, 32, 64);
  const int oi = __shfl_xor(bi, 32, 64);
  if (ob > best || (ob == best && oi < bi)) {
    best = ob;
    bi = oi;
  }
}

// The tile loop both matrix-core head kernels run (one accumulation order: their labels are the same integers).  sw: the LDS
// image [M][32 NCB][WF_WPITCH], then bsum [32 NCB]; epi(acc, n, v, valid, h) consumes a tile's accumulators - the UNSCALED sums
// sum_m W_m F_m(v) + n(v) bsum of voxel v (valid = 0 on the tail lanes, which repeat the last voxel).
template <int NCB, typename Epi>
__device__ __forceinline__ void feature_head_tiles(const float *__restrict__ facc, int64_t member_stride, const float *__restrict__ nsum,
                                                   const float *__restrict__ w, const float *__restrict__ bsum, int M, int C, int64_t V,
                                                   float *sw, Epi epi) {
  float *sb = sw + (size_t)M * 32 * NCB * WF_WPITCH;
  const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  for (int i = tid; i < M * 32 * NCB * WF_CIN; i += 256) {
    const int k = i % WF_CIN, c = (i / WF_CIN) % (32 * NCB), m = i / (WF_CIN * 32 * NCB);
    sw[(m * 32 * NCB + c) * WF_WPITCH + k] = c < C ? w[((int64_t)m * C + c) * WF_CIN + k] : 0.f;
  }
  for (int c = tid; c < 32 * NCB; c += 256) sb[c] = c < C ? bsum[c] : 0.f;
  __syncthreads();
  const int j = lane & 31, h = lane >> 5;
  const int64_t ntile = (V + 31) / 32;
  const int64_t tstep = (int64_t)gridDim.x * 4;
  // the features of (tile, member) pair p + 1 are requested before the 16 NCB MFMAs of pair p issue: at 2 waves per SIMD (161
  // registers with four class blocks) a load - wait - multiply sequence per pair left the matrix pipe idle for the memory latency
  auto voxel_of = [&](int64_t t) { return t * 32 + j < V ? t * 32 + j : V - 1; };
  auto load_fb = [&](int64_t t, int m, float4(&fb)[4]) {
    const float4 *fv = reinterpret_cast<const float4 *>(facc + m * member_stride + voxel_of(t) * WF_CIN) + h;
#pragma unroll
    for (int s = 0; s < 4; ++s) fb[s] = fv[2 * s];      // channels 8 s + 4 h .. + 3
  };
  float4 fb[4], fn[4];
  int64_t t = (int64_t)blockIdx.x * 4 + wave;
  if (t < ntile) load_fb(t, 0, fb);
  for (; t < ntile; t += tstep) {
    const int64_t v = voxel_of(t);
    const float n = nsum[v];
    f32x16_t acc[NCB];
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
      for (int q4 = 0; q4 < 4; ++q4) {      // a lane's classes come in runs of four
        const float4 b4 = *reinterpret_cast<const float4 *>(sb + cb * 32 + 8 * q4 + 4 * h);
        acc[cb][4 * q4 + 0] = n * b4.x, acc[cb][4 * q4 + 1] = n * b4.y, acc[cb][4 * q4 + 2] = n * b4.z, acc[cb][4 * q4 + 3] = n * b4.w;
      }
    for (int m = 0; m < M; ++m) {
      if (m + 1 < M) load_fb(t, m + 1, fn);
      else if (t + tstep < ntile) load_fb(t + tstep, 0, fn);
      const float *wm = sw + ((size_t)m * 32 * NCB + j) * WF_WPITCH + 4 * h;
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        float4 wa[NCB];
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb) wa[cb] = *reinterpret_cast<const float4 *>(wm + (size_t)cb * 32 * WF_WPITCH + 8 * s);
        // (consecutive instructions on different accumulators: a chain on one accumulator waits for itself)
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb) acc[cb] = __builtin_amdgcn_mfma_f32_32x32x2f32(wa[cb].x, fb[s].x, acc[cb], 0, 0, 0);
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb) acc[cb] = __builtin_amdgcn_mfma_f32_32x32x2f32(wa[cb].y, fb[s].y, acc[cb], 0, 0, 0);
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb) acc[cb] = __builtin_amdgcn_mfma_f32_32x32x2f32(wa[cb].z, fb[s].z, acc[cb], 0, 0, 0);
#pragma unroll
        for (int cb = 0; cb < NCB; ++cb) acc[cb] = __builtin_amdgcn_mfma_f32_32x32x2f32(wa[cb].w, fb[s].w, acc[cb], 0, 0, 0);
      }
#pragma unroll
      for (int s = 0; s < 4; ++s) fb[s] = fn[s];
    }
    epi(acc, n, v, t * 32 + j < V, h);
  }
}

template <int NCB>      // class blocks of 32 (C <= 32 NCB)
__global__ __launch_bounds__(256) void feature_head_argmax_mfma_kernel(const float *__restrict__ facc, int64_t member_stride,
                                                                       const float *__restrict__ nsum, const float *__restrict__ w,
                                                                       const float *__restrict__ bsum, int M, int C, int64_t V,
                                                                       int64_t *__restrict__ amax) {
  extern __shared__ __attribute__((aligned(16))) float sw[];      // [M][32 NCB][WF_WPITCH], then bsum [32 NCB]
  feature_head_tiles<NCB>(facc, member_stride, nsum, w, bsum, M, C, V, sw, [&](const f32x16_t(&acc)[NCB], float, int64_t v, bool valid, int h) {
    float best;
    int bi;
    wf_first_max<NCB>(acc, C, h, best, bi);
    if (h == 0 && valid) amax[v] = bi;
  });
}

// Head + softmax of the ensemble-MEAN logits l_c = acc_c / (M n) on the same tile loop: label (the argmax kernel's integers: the scan
// runs on the unscaled accumulators, and a positive scale keeps their order), confidence = p[label] = 1 / S and entropy =
// ln S - D / S with S = sum_c exp(l_c - l_max), D = sum_c (l_c - l_max) exp(l_c - l_max) - one exp and one FMA per class, one log
// per voxel - and the probabilities of the K selected classes, plane-major ([K][V]: a lane half's 32 voxels of a class are one
// contiguous run).  All reductions stay inside a lane plus one exchange between the lane halves.  The padding classes of the last
// block (accumulators 0, not -inf) are masked out of every sum.  The scale is rounded once (formed in double) and applied with one
// multiplication: two roundings on top of the dot product's.  slot: class -> row of `probs` (LDS, 128 bytes, -1 = not selected),
// read four classes at a time - a lane's classes come in aligned runs of four.
// Measured at 512^3 x 105 classes (profiles/tools/headprobs_bench.py): 20.1 ms with one member and one fp16 plane, 25.5 ms with 16
// planes (argmax kernel 13.5); three members 35.5 / 40.8 ms (28.7).  The difference is the epilogue's vector instructions (about 9
// issue slots per class and lane), which nothing overlaps at one wave per SIMD (326 registers with four class blocks); DESIGN.md.
struct WfSel {
  int c[32];
};

template <int NCB, typename PT>
__global__ __launch_bounds__(256) void feature_head_softmax_mfma_kernel(const float *__restrict__ facc, int64_t member_stride,
                                                                        const float *__restrict__ nsum, const float *__restrict__ w,
                                                                        const float *__restrict__ bsum, int M, int C, int64_t V,
                                                                        WfSel sel, int K, int64_t *__restrict__ label,
                                                                        float *__restrict__ conf, float *__restrict__ entropy,
                                                                        PT *__restrict__ probs) {
  extern __shared__ __attribute__((aligned(16))) float sw[];      // [M][32 NCB][WF_WPITCH], bsum [32 NCB], slot [128] (bytes)
  signed char *slot = reinterpret_cast<signed char *>(sw + (size_t)M * 32 * NCB * WF_WPITCH + 32 * NCB);
  const int tid = threadIdx.x;
  if (tid < 128) slot[tid] = -1;
  __syncthreads();
  {
    int mine = 0;
#pragma unroll
    for (int k = 0; k < 32; ++k) mine = tid == k ? sel.c[k] : mine;      // (no runtime index into the kernel argument)
    if (tid < K) slot[mine] = (signed char)tid;
  }      // (feature_head_tiles synchronises before the first tile)
  const double dM = (double)M;
  feature_head_tiles<NCB>(facc, member_stride, nsum, w, bsum, M, C, V, sw, [&](const f32x16_t(&acc)[NCB], float n, int64_t v, bool valid, int h) {
    float best;
    int bi;
    wf_first_max<NCB>(acc, C, h, best, bi);
    const float inv = (float)(1.0 / (dM * (double)n));
    const float lmax = best * inv;
    float Sp[4] = {0.f, 0.f, 0.f, 0.f}, Dp[4] = {0.f, 0.f, 0.f, 0.f};      // four independent chains: one waits for itself
#pragma unroll
    for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
      for (int q = 0; q < 16; ++q) {
        const int c = cb * 32 + (q & 3) + 8 * (q >> 2) + 4 * h;
        if (cb + 1 < NCB || c < C) {
          const float x = acc[cb][q] * inv - lmax;
          const float e = __expf(x);
          Sp[q & 3] += e;
          Dp[q & 3] = fmaf(x, e, Dp[q & 3]);
        }
      }
    float S = (Sp[0] + Sp[1]) + (Sp[2] + Sp[3]), D = (Dp[0] + Dp[1]) + (Dp[2] + Dp[3]);
    S += __shfl_xor(S, 32, 64);
    D += __shfl_xor(D, 32, 64);
    const float invS = 1.f / S;
    if (valid) {
      if (h == 0) {
        label[v] = bi;
        conf[v] = invS;
        entropy[v] = fmaxf(__logf(S) - D * invS, 0.f);
      }
#pragma unroll
      for (int cb = 0; cb < NCB; ++cb)
#pragma unroll
        for (int q4 = 0; q4 < 4; ++q4) {
          const unsigned s4 = *reinterpret_cast<const unsigned *>(slot + cb * 32 + 8 * q4 + 4 * h);
          if (s4 == 0xffffffffu) continue;
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int k = (int)(signed char)(s4 >> (8 * r));
            if (k >= 0) st_f<PT>(probs + (int64_t)k * V + v, __expf(acc[cb][4 * q4 + r] * inv - lmax) * invS);
          }
        }
    }
  });
}

// Label map of a REGION-based head (region_loss.hip's header: R <= 32 sigmoid outputs, one class block) on the same tile loop:
// seg = 0; for i = 0 .. R-1 in order: seg = order[i] where the ensemble-mean logit l_i > 0 - nnU-Net's
// convert_probabilities_to_segmentation for regions, from memory, UNPINNED.  The mean is a positive multiple of the unscaled
// accumulator, so its sign decides (a sum of exactly 0 is not in the region).  A lane's classes ascend with q, so the last q with
// acc > 0 is the half's last positive region; the voxel's is the larger of the two halves'.  The same accumulation order as the
// argmax and softmax kernels.  order sits behind bsum in LDS.
struct WfOrder {
  int c[32];
};

__global__ __launch_bounds__(256) void feature_head_regions_mfma_kernel(const float *__restrict__ facc, int64_t member_stride,
                                                                        const float *__restrict__ nsum, const float *__restrict__ w,
                                                                        const float *__restrict__ bsum, int M, int R, int64_t V,
                                                                        WfOrder order, int64_t *__restrict__ label) {
  extern __shared__ __attribute__((aligned(16))) float sw[];      // [M][32][WF_WPITCH], bsum [32], order [32] (ints)
  int *s_ord = reinterpret_cast<int *>(sw + (size_t)M * 32 * WF_WPITCH + 32);
  const int tid = threadIdx.x;
  {
    int mine = 0;
#pragma unroll
    for (int k = 0; k < 32; ++k) mine = tid == k ? order.c[k] : mine;      // (no runtime index into the kernel argument)
    if (tid < 32) s_ord[tid] = mine;
  }      // (feature_head_tiles synchronises before the first tile)
  feature_head_tiles<1>(facc, member_stride, nsum, w, bsum, M, R, V, sw, [&](const f32x16_t(&acc)[1], float, int64_t v, bool valid, int h) {
    int li = -1;
#pragma unroll
    for (int q = 0; q < 16; ++q) {
      const int c = (q & 3) + 8 * (q >> 2) + 4 * h;
      if (c < R && acc[0][q] > 0.f) li = c;
    }
    const int oi = __shfl_xor(li, 32, 64);
    li = oi > li ? oi : li;
    if (h == 0 && valid) label[v] = li >= 0 ? s_ord[li] : 0;
  });
}

// Export path (original geometry): classes c0 .. c0 + cg - 1 of the normalised ensemble logits as doubles,
// dst[x][y][z][j] = sum_m (W_m[c0 + j] . F_m(sv)) / n(sv) + bsum[c0 + j] - the input of the dgtta_resample_axis passes, as
// dgtta_logits_chunk_f64 is for the logits-space accumulator (products and sums in double).
__global__ void feature_logits_chunk_kernel(const float *__restrict__ facc, int64_t member_stride, const float *__restrict__ nsum,
                                            const float *__restrict__ w, const float *__restrict__ bsum, double *__restrict__ dst,
                                            int M, int C, int Y, int Z, int x0, int y0, int z0, int ys, int zs, int c0, int cg,
                                            int64_t total) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= total) return;
  const int j = (int)(i % cg);
  const int64_t v = i / cg;
  const int z = (int)(v % zs), y = (int)((v / zs) % ys);
  const int64_t x = v / ((int64_t)zs * ys);
  const int64_t sv = ((x + x0) * Y + (y + y0)) * Z + (z + z0);
  double s = 0.0;
  for (int m = 0; m < M; ++m) {
    const float *f = facc + m * member_stride + sv * WF_CIN;
    const float *wr = w + ((int64_t)m * C + c0 + j) * WF_CIN;
    for (int k = 0; k < WF_CIN; ++k) s += (double)wr[k] * (double)f[k];
  }
  dst[i] = s / (double)nsum[sv] + (double)bsum[c0 + j];
}

}  // namespace

// The one launcher of feature_accumulate_kernel: nsrc windows on a segment of seg_len voxels of the last axis (a whole window: nsrc = 1,
// seg_len = PW); `what` names that block in the message.  mirror = 0 launches the kernel the unmirrored entries launch: their bits.
template <typename T, bool NORM>
static void feature_accumulate_launch_t(const WfSources &ws, int nsrc, const float *gamma, const float *beta, float slope, const float *gauss,
                                        float *facc, float *nsum, const WindowPlace &wp, int seg_len, int64_t total, hipStream_t st) {
  const auto kernel = wp.mirror   ? feature_accumulate_kernel<T, 1, NORM, true>
                      : nsrc == 1 ? feature_accumulate_kernel<T, 1, NORM, false>
                      : nsrc == 2 ? feature_accumulate_kernel<T, 2, NORM, false>
                      : nsrc == 3 ? feature_accumulate_kernel<T, 3, NORM, false>
                                  : feature_accumulate_kernel<T, 4, NORM, false>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)cdiv64(total, 256)), dim3(256), 0, st, ws, gamma, beta, slope, gauss, facc, nsum, wp, seg_len,
                     total);
}

static int feature_accumulate_launch(const char *who, const char *what, const WfSources &ws, int nsrc, bool norm, const float *gamma,
                                     const float *beta, float slope, const float *gauss, float *facc, float *nsum, const WindowPlace &wp,
                                     int seg_len, int dtype, void *stream) {
  const int64_t total = (int64_t)wp.PD * wp.PH * seg_len * 8;
  DG_REQUIRE(cdiv64(total, 256) < (1ll << 31), DGTTA_ERR_UNSUPPORTED, "%s: %s too large", who, what);
  DISPATCH_T(dtype, (norm ? feature_accumulate_launch_t<T, true> : feature_accumulate_launch_t<T, false>)(
                        ws, nsrc, gamma, beta, slope, gauss, facc, nsum, wp, seg_len, total, (hipStream_t)stream));
  DG_CHECK_LAUNCH("feature_accumulate_kernel");
  return DGTTA_OK;
}

static int feature_storage_check(const char *who, int Cin, int dtype) {
  DG_REQUIRE(Cin == WF_CIN, DGTTA_ERR_UNSUPPORTED, "%s: built for %d feature channels (got %d)", who, WF_CIN, Cin);
  DG_REQUIRE(dtype == DGTTA_F32 || dtype == DGTTA_BF16 || dtype == DGTTA_F16, DGTTA_ERR_BADARG, "%s: dtype %d", who, dtype);
  return DGTTA_OK;
}

// The four one-window entries: src = the window's features, or (norm) its raw conv output with the statistics mean_rstd
static int feature_window_accumulate_one(const char *who, const void *src, bool norm, const float *mean_rstd, const float *gamma,
                                         const float *beta, float slope, const float *gauss, float *facc, float *nsum, int Cin,
                                         const WindowPlace &wp, int dtype, void *stream) {
  DG_REQUIRE(src && gauss && facc && (!norm || (mean_rstd && gamma && beta)), DGTTA_ERR_BADARG, "%s: null pointer", who);
  if (const int rc = feature_storage_check(who, Cin, dtype)) return rc;
  if (const int rc = window_place_check(who, wp)) return rc;
  DG_REQUIRE(((uintptr_t)src & 15) == 0 && ((uintptr_t)facc & 15) == 0, DGTTA_ERR_BADARG, "%s: unaligned buffer", who);
  WfSources ws{};
  ws.src[0] = src;
  ws.mean_rstd[0] = mean_rstd;
  return feature_accumulate_launch(who, "window", ws, 1, norm, gamma, beta, slope, gauss, facc, nsum, wp, wp.PW, dtype, stream);
}

extern "C" int dgtta_feature_window_accumulate(const void *z, const float *gauss, float *facc, float *nsum, int Cin, int PD, int PH,
                                               int PW, int X, int Y, int Z, int x0, int y0, int z0, int dtype, void *stream) {
  return feature_window_accumulate_one("feature_window_accumulate", z, false, nullptr, nullptr, nullptr, 0.f, gauss, facc, nsum, Cin,
                                       {PD, PH, PW, X, Y, Z, x0, y0, z0, 0}, dtype, stream);
}

extern "C" int dgtta_feature_window_accumulate_mirror(const void *z, const float *gauss, float *facc, float *nsum, int Cin, int PD, int PH,
                                                      int PW, int X, int Y, int Z, int x0, int y0, int z0, int dtype, int mirror,
                                                      void *stream) {
  return feature_window_accumulate_one("feature_window_accumulate_mirror", z, false, nullptr, nullptr, nullptr, 0.f, gauss, facc, nsum, Cin,
                                       {PD, PH, PW, X, Y, Z, x0, y0, z0, mirror}, dtype, stream);
}

extern "C" int dgtta_feature_window_accumulate_norm(const void *y, const float *mean_rstd, const float *gamma, const float *beta, float slope,
                                                    const float *gauss, float *facc, float *nsum, int Cin, int PD, int PH, int PW, int X,
                                                    int Y, int Z, int x0, int y0, int z0, int dtype, void *stream) {
  return feature_window_accumulate_one("feature_window_accumulate_norm", y, true, mean_rstd, gamma, beta, slope, gauss, facc, nsum, Cin,
                                       {PD, PH, PW, X, Y, Z, x0, y0, z0, 0}, dtype, stream);
}

extern "C" int dgtta_feature_window_accumulate_norm_mirror(const void *y, const float *mean_rstd, const float *gamma, const float *beta,
                                                           float slope, const float *gauss, float *facc, float *nsum, int Cin, int PD, int PH,
                                                           int PW, int X, int Y, int Z, int x0, int y0, int z0, int dtype, int mirror,
                                                           void *stream) {
  return feature_window_accumulate_one("feature_window_accumulate_norm_mirror", y, true, mean_rstd, gamma, beta, slope, gauss, facc, nsum, Cin,
                                       {PD, PH, PW, X, Y, Z, x0, y0, z0, mirror}, dtype, stream);
}

extern "C" int dgtta_feature_window_accumulate_multi(const void *const *h_srcs, const float *const *h_mean_rstds, const int *h_zoffs, int nsrc,
                                                     const float *gamma, const float *beta, float slope, const float *gauss, float *facc,
                                                     float *nsum, int Cin, int PD, int PH, int PW, int seg_len, int X, int Y, int Z, int x0,
                                                     int y0, int z0, int dtype, void *stream) {
  const char *who = "feature_window_accumulate_multi";
  DG_REQUIRE(h_srcs && h_zoffs && gauss && facc, DGTTA_ERR_BADARG, "%s: null pointer", who);
  DG_REQUIRE(nsrc >= 1 && nsrc <= 4, DGTTA_ERR_UNSUPPORTED, "%s: 1..4 windows per segment (got %d)", who, nsrc);
  if (const int rc = feature_storage_check(who, Cin, dtype)) return rc;
  const bool norm = h_mean_rstds != nullptr;
  DG_REQUIRE(!norm || (gamma && beta), DGTTA_ERR_BADARG, "%s: statistics without gamma / beta", who);
  DG_REQUIRE(PD > 0 && PH > 0 && PW > 0 && seg_len > 0 && seg_len <= PW && x0 >= 0 && y0 >= 0 && z0 >= 0 && x0 + PD <= X && y0 + PH <= Y &&
                 z0 + seg_len <= Z, DGTTA_ERR_BADARG, "%s: segment outside the volume", who);
  WfSources ws{};
  for (int k = 0; k < nsrc; ++k) {
    DG_REQUIRE(h_srcs[k] && ((uintptr_t)h_srcs[k] & 15) == 0 && h_zoffs[k] >= 0 && h_zoffs[k] + seg_len <= PW && (!norm || h_mean_rstds[k]),
               DGTTA_ERR_BADARG, "%s: window %d (null / unaligned source or segment outside the window)", who, k);
    ws.src[k] = h_srcs[k];
    ws.mean_rstd[k] = norm ? h_mean_rstds[k] : nullptr;
    ws.zoff[k] = h_zoffs[k];
  }
  DG_REQUIRE(((uintptr_t)facc & 15) == 0, DGTTA_ERR_BADARG, "%s: unaligned accumulator", who);
  return feature_accumulate_launch(who, "segment", ws, nsrc, norm, gamma, beta, slope, gauss, facc, nsum, {PD, PH, PW, X, Y, Z, x0, y0, z0, 0},
                                   seg_len, dtype, stream);
}

extern "C" int dgtta_feature_head_argmax(const float *facc, int64_t member_stride, const float *nsum, const float *w, const float *bsum,
                                         int M, int Cin, int C, int64_t V, int64_t *argmax_out, void *stream) {
  DG_REQUIRE(facc && nsum && w && bsum && argmax_out, DGTTA_ERR_BADARG, "feature_head_argmax: null pointer");
  DG_REQUIRE(Cin == WF_CIN, DGTTA_ERR_UNSUPPORTED, "feature_head_argmax: built for %d feature channels (got %d)", WF_CIN, Cin);
  DG_REQUIRE(M >= 1 && C >= 1 && V >= 1 && (M == 1 || member_stride >= V * WF_CIN), DGTTA_ERR_BADARG, "feature_head_argmax: bad sizes");
  DG_REQUIRE(((uintptr_t)facc & 15) == 0 && (member_stride & 3) == 0, DGTTA_ERR_BADARG, "feature_head_argmax: unaligned accumulator");
  // the matrix-core kernel when its weight image fits the LDS (DGTTA_FEATURE_HEAD_MFMA=0: the vector-ALU kernel)
  const int ncb = (C + 31) / 32;
  const size_t lds_m = ((size_t)M * 32 * ncb * WF_WPITCH + 32 * ncb) * sizeof(float);
  const bool use_mfma = dgtta_switches().feature_head_mfma != '0';
  if (use_mfma && ncb <= 4 && lds_m <= 160 * 1024) {
    static DynLdsOnce once_m[4];
    const int64_t ntile = cdiv64(V, 32);
    const unsigned grid = (unsigned)(cdiv64(ntile, 4) < 2048 ? cdiv64(ntile, 4) : 2048);
#define WF_MFMA(N)                                                                                                                   \
  do {                                                                                                                               \
    DG_REQUIRE(ensure_dyn_lds(once_m[N - 1], (const void *)feature_head_argmax_mfma_kernel<N>, 160 * 1024) == hipSuccess,            \
               DGTTA_ERR_LAUNCH, "feature_head_argmax: cannot raise the dynamic LDS limit");                                         \
    hipLaunchKernelGGL(feature_head_argmax_mfma_kernel<N>, dim3(grid), dim3(256), lds_m, (hipStream_t)stream, facc, member_stride,    \
                       nsum, w, bsum, M, C, V, argmax_out);                                                                          \
  } while (0)
    if (ncb == 1) WF_MFMA(1);
    else if (ncb == 2) WF_MFMA(2);
    else if (ncb == 3) WF_MFMA(3);
    else WF_MFMA(4);
#undef WF_MFMA
    DG_CHECK_LAUNCH("feature_head_argmax_mfma_kernel");
    return DGTTA_OK;
  }
  const size_t lds = M > 1 ? (size_t)C * 256 * sizeof(float) : 0;
  DG_REQUIRE(lds <= 160 * 1024, DGTTA_ERR_UNSUPPORTED, "feature_head_argmax: %d classes x several members exceed the LDS (<= 160)", C);
  static DynLdsOnce once;
  if (lds > 64 * 1024)
    DG_REQUIRE(ensure_dyn_lds(once, (const void *)feature_head_argmax_kernel, 160 * 1024) == hipSuccess, DGTTA_ERR_LAUNCH,
               "feature_head_argmax: cannot raise the dynamic LDS limit");
  const int64_t nblk = cdiv64(V, 256);
  const unsigned grid = (unsigned)(nblk < 8192 ? nblk : 8192);
  hipLaunchKernelGGL(feature_head_argmax_kernel, dim3(grid), dim3(256), lds, (hipStream_t)stream, facc, member_stride, nsum, w, bsum, M, C,
                     V, argmax_out);
  DG_CHECK_LAUNCH("feature_head_argmax_kernel");
  return DGTTA_OK;
}

extern "C" int dgtta_feature_head_softmax(const float *facc, int64_t member_stride, const float *nsum, const float *w, const float *bsum,
                                          int M, int Cin, int C, int64_t V, const int *h_sel, int K, int prob_dtype, int64_t *label_out,
                                          float *conf_out, float *entropy_out, void *probs_out, void *stream) {
  DG_REQUIRE(facc && nsum && w && bsum && h_sel && label_out && conf_out && entropy_out && probs_out, DGTTA_ERR_BADARG,
             "feature_head_softmax: null pointer");
  DG_REQUIRE(Cin == WF_CIN, DGTTA_ERR_UNSUPPORTED, "feature_head_softmax: built for %d feature channels (got %d)", WF_CIN, Cin);
  DG_REQUIRE(M >= 1 && C >= 1 && V >= 1 && (M == 1 || member_stride >= V * WF_CIN), DGTTA_ERR_BADARG, "feature_head_softmax: bad sizes");
  DG_REQUIRE(((uintptr_t)facc & 15) == 0 && (member_stride & 3) == 0, DGTTA_ERR_BADARG, "feature_head_softmax: unaligned accumulator");
  DG_REQUIRE(prob_dtype == DGTTA_F32 || prob_dtype == DGTTA_F16, DGTTA_ERR_BADARG, "feature_head_softmax: probabilities are fp32 or fp16");
  DG_REQUIRE(K >= 1 && K <= 32, DGTTA_ERR_BADARG, "feature_head_softmax: 1..32 selected classes (got %d)", K);
  WfSel sel{};
  for (int k = 0; k < K; ++k) {
    DG_REQUIRE(h_sel[k] >= 0 && h_sel[k] < C, DGTTA_ERR_BADARG, "feature_head_softmax: selected class %d outside [0,%d)", h_sel[k], C);
    for (int i = 0; i < k; ++i) DG_REQUIRE(h_sel[i] != h_sel[k], DGTTA_ERR_BADARG, "feature_head_softmax: class %d selected twice", h_sel[k]);
    sel.c[k] = h_sel[k];
  }
  const int ncb = (C + 31) / 32;
  const size_t lds = ((size_t)M * 32 * ncb * WF_WPITCH + 32 * ncb) * sizeof(float) + 128;
  DG_REQUIRE(ncb <= 4 && lds <= 160 * 1024, DGTTA_ERR_UNSUPPORTED,
             "feature_head_softmax: %d classes x %d members: at most 128 classes and a weight image that fits the LDS", C, M);
  static DynLdsOnce once[2][4];
  const int64_t ntile = cdiv64(V, 32);
  const unsigned grid = (unsigned)(cdiv64(ntile, 4) < 2048 ? cdiv64(ntile, 4) : 2048);
#define WF_SOFTMAX(N, PT, pi)                                                                                                           \
  do {                                                                                                                                  \
    DG_REQUIRE(ensure_dyn_lds(once[pi][N - 1], (const void *)feature_head_softmax_mfma_kernel<N, PT>, 160 * 1024) == hipSuccess,         \
               DGTTA_ERR_LAUNCH, "feature_head_softmax: cannot raise the dynamic LDS limit");                                           \
    hipLaunchKernelGGL((feature_head_softmax_mfma_kernel<N, PT>), dim3(grid), dim3(256), lds, (hipStream_t)stream, facc, member_stride, \
                       nsum, w, bsum, M, C, V, sel, K, label_out, conf_out, entropy_out, (PT *)probs_out);                              \
  } while (0)
#define WF_SOFTMAX_N(PT, pi)           \
  do {                                 \
    if (ncb == 1) WF_SOFTMAX(1, PT, pi); \
    else if (ncb == 2) WF_SOFTMAX(2, PT, pi); \
    else if (ncb == 3) WF_SOFTMAX(3, PT, pi); \
    else WF_SOFTMAX(4, PT, pi);        \
  } while (0)
  if (prob_dtype == DGTTA_F32) WF_SOFTMAX_N(float, 0);
  else WF_SOFTMAX_N(f16_t, 1);
#undef WF_SOFTMAX_N
#undef WF_SOFTMAX
  DG_CHECK_LAUNCH("feature_head_softmax_mfma_kernel");
  return DGTTA_OK;
}

extern "C" int dgtta_feature_head_regions(const float *facc, int64_t member_stride, const float *nsum, const float *w, const float *bsum,
                                          int M, int Cin, int R, int64_t V, const int *h_order, int64_t *label_out, void *stream) {
  DG_REQUIRE(facc && nsum && w && bsum && h_order && label_out, DGTTA_ERR_BADARG, "feature_head_regions: null pointer");
  DG_REQUIRE(Cin == WF_CIN, DGTTA_ERR_UNSUPPORTED, "feature_head_regions: built for %d feature channels (got %d)", WF_CIN, Cin);
  DG_REQUIRE(M >= 1 && R >= 1 && V >= 1 && (M == 1 || member_stride >= V * WF_CIN), DGTTA_ERR_BADARG, "feature_head_regions: bad sizes");
  DG_REQUIRE(((uintptr_t)facc & 15) == 0 && (member_stride & 3) == 0, DGTTA_ERR_BADARG, "feature_head_regions: unaligned accumulator");
  const size_t lds = ((size_t)M * 32 * WF_WPITCH + 32) * sizeof(float) + 32 * sizeof(int);
  DG_REQUIRE(R <= 32 && lds <= 160 * 1024, DGTTA_ERR_UNSUPPORTED,
             "feature_head_regions: %d regions x %d members: at most 32 regions and a weight image that fits the LDS", R, M);
  WfOrder order{};
  for (int i = 0; i < R; ++i) {
    DG_REQUIRE(h_order[i] > 0, DGTTA_ERR_BADARG, "feature_head_regions: regions_class_order[%d] = %d is not a positive label", i, h_order[i]);
    order.c[i] = h_order[i];
  }
  static DynLdsOnce once;
  DG_REQUIRE(ensure_dyn_lds(once, (const void *)feature_head_regions_mfma_kernel, 160 * 1024) == hipSuccess, DGTTA_ERR_LAUNCH,
             "feature_head_regions: cannot raise the dynamic LDS limit");
  const int64_t ntile = cdiv64(V, 32);
  const unsigned grid = (unsigned)(cdiv64(ntile, 4) < 2048 ? cdiv64(ntile, 4) : 2048);
  hipLaunchKernelGGL(feature_head_regions_mfma_kernel, dim3(grid), dim3(256), lds, (hipStream_t)stream, facc, member_stride, nsum, w, bsum,
                     M, R, V, order, label_out);
  DG_CHECK_LAUNCH("feature_head_regions_mfma_kernel");
  return DGTTA_OK;
}

extern "C" int dgtta_feature_logits_chunk_f64(const float *facc, int64_t member_stride, const float *nsum, const float *w,
                                              const float *bsum, double *dst, int M, int Cin, int C, int X, int Y, int Z, int x0, int y0,
                                              int z0, int xs, int ys, int zs, int c0, int cg, void *stream) {
  DG_REQUIRE(facc && nsum && w && bsum && dst, DGTTA_ERR_BADARG, "feature_logits_chunk: null pointer");
  DG_REQUIRE(Cin == WF_CIN, DGTTA_ERR_UNSUPPORTED, "feature_logits_chunk: built for %d feature channels (got %d)", WF_CIN, Cin);
  DG_REQUIRE(M >= 1 && C > 0 && cg > 0 && c0 >= 0 && c0 + cg <= C, DGTTA_ERR_BADARG, "feature_logits_chunk: class range outside [0,%d)", C);
  DG_REQUIRE(x0 >= 0 && y0 >= 0 && z0 >= 0 && xs > 0 && ys > 0 && zs > 0 && x0 + xs <= X && y0 + ys <= Y && z0 + zs <= Z, DGTTA_ERR_BADARG,
             "feature_logits_chunk: crop outside the volume");
  DG_REQUIRE(M == 1 || member_stride >= (int64_t)X * Y * Z * WF_CIN, DGTTA_ERR_BADARG, "feature_logits_chunk: member stride");
  const int64_t total = (int64_t)xs * ys * zs * cg;
  DG_REQUIRE(cdiv64(total, 256) < (1ll << 31), DGTTA_ERR_UNSUPPORTED, "feature_logits_chunk: too many values");
  hipLaunchKernelGGL(feature_logits_chunk_kernel, dim3((unsigned)cdiv64(total, 256)), dim3(256), 0, (hipStream_t)stream, facc, member_stride,
                     nsum, w, bsum, dst, M, C, Y, Z, x0, y0, z0, ys, zs, c0, cg, total);
  DG_CHECK_LAUNCH("feature_logits_chunk_kernel");
  return DGTTA_OK;
}
