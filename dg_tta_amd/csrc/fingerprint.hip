// Dataset fingerprint (dg_tta_amd/planning/fingerprint.py): exact pooled statistics of the foreground voxels (seg > 0) of all
// training cases of one image channel - count, min, max, mean, population std and the order statistics under the median and
// the 0.5 / 99.5 percentiles.  One entry point, dgtta_fingerprint_sweep, called once per case and sweep; HBM-bound: one read of
// the channel (4 B) and of the label map (1 / 2 / 4 B) per voxel, as 16-byte image loads and 4 / 8 / 16-byte label loads.
//
// Order statistics: radix select on the order-preserving 32-bit key of the float (sign bit flipped for a non-negative value, all
// bits inverted for a negative one), digit by digit (11 + 11 + 10 bits in the driver).  A sweep counts, for each of up to
// DGTTA_FP_MAX_PREFIXES prefixes, the next digit of every foreground key that starts with the prefix.  A CT foreground piles into a
// few bins, so nothing is counted with global atomics: a workgroup counts in LDS (integer LDS adds), writes its histogram to a slab
// of its own in the workspace with plain stores, and a reducer adds the slabs in ascending order into the caller's 64-bit counters,
// which persist across the cases of a sweep.  Integer counts: exact in any order.
//
// Moments: moment = 1 leaves count, min, max, sum x and the number of non-finite foreground values; moment = 2 leaves
// sum (x - mean)^2 around the caller's mean.  Both sums are double: per thread in index order, across the workgroup in a fixed
// tree, one partial per workgroup, the partials added in workgroup order by one thread, the case's sum added to the running
// state - the same bits on every run for a given case order.  No floating-point atomics.  Non-finite foreground values are
// counted and left out of every other statistic; the state keeps the index of the first case that had one.
#include "common.h"
#include <math.h>

namespace {

constexpr int BINS = DGTTA_FP_BINS;
constexpr int MAXT = DGTTA_FP_MAX_PREFIXES;
constexpr int CHUNK = 256 * 16;   // voxels per workgroup and step: 16 per thread, in four groups of four consecutive ones
constexpr int MAX_WG = 512;       // two workgroups per CU: the slabs stay a small fraction of the case

struct FpPartial {
  double sum;
  unsigned long long count, nonfinite;
  float mn, mx;
};
static_assert(sizeof(FpPartial) == 32, "FpPartial is 32 bytes");

// four consecutive labels, loaded as one 4 / 8 / 16-byte word
template <typename L>
struct alignas(4 * sizeof(L)) Lab4 {
  L v[4];
};

struct FpPrefixes {
  unsigned p[MAXT];
};

__device__ __forceinline__ unsigned key_of(float v) {
  const unsigned u = __float_as_uint(v);
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

// workgroups of a case of V voxels: a function of V alone, so that the partition of the sums is fixed for a given case and
// does not depend on which cases were resident or on anything else of the run
inline int fp_workgroups(int64_t V) {
  const int64_t c = (V + CHUNK - 1) / CHUNK;
  return (int)(c < MAX_WG ? (c < 1 ? 1 : c) : MAX_WG);
}

// MOMENT 0: histogram only; 1: count / min / max / sum / non-finite; 2: sum (x - mean)^2
template <typename L, int MOMENT>
__global__ __launch_bounds__(256) void fp_sweep_kernel(const float *__restrict__ x, const L *__restrict__ seg, int64_t V,
                                                       int prefix_bits, int digit_shift, unsigned digit_mask, FpPrefixes pre, int T,
                                                       double mean, unsigned *__restrict__ slabs, FpPartial *__restrict__ partials) {
  __shared__ unsigned hist[MAXT * BINS];
  __shared__ double red_d[4];
  __shared__ unsigned long long red_c[4], red_n[4];
  __shared__ float red_mn[4], red_mx[4];
  const int nbin = T * BINS;
  for (int i = threadIdx.x; i < nbin; i += 256) hist[i] = 0u;
  __syncthreads();
  const int prefix_shift = 32 - prefix_bits;   // 32 when there is no prefix: never shifted by
  double acc = 0.0;
  unsigned long long cnt = 0, bad = 0;
  float mn = INFINITY, mx = -INFINITY;
  // thread t of a step owns the voxels base + 4 (256 k + t) + j, k, j = 0 .. 3: four 16-byte loads of the image and four 4 / 8 / 16
  // byte loads of the labels, all issued before the first value is consumed.  Unaligned pointers and the ragged end of the case
  // take scalar loads of the SAME voxels, so the order of every sum does not depend on the path.
  const bool vec = (((uintptr_t)x & 15) == 0) && (((uintptr_t)seg & (4 * sizeof(L) - 1)) == 0);
  for (int64_t base = (int64_t)blockIdx.x * CHUNK; base < V; base += (int64_t)gridDim.x * CHUNK) {
    float xv[4][4];
    L sv[4][4];
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int64_t i0 = base + (int64_t)(k * 256 + (int)threadIdx.x) * 4;
      if (vec && i0 + 4 <= V) {
        const float4 f = *reinterpret_cast<const float4 *>(x + i0);
        const Lab4<L> l = *reinterpret_cast<const Lab4<L> *>(seg + i0);
        xv[k][0] = f.x, xv[k][1] = f.y, xv[k][2] = f.z, xv[k][3] = f.w;
#pragma unroll
        for (int j = 0; j < 4; ++j) sv[k][j] = l.v[j];
      } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
          const bool in = i0 + j < V;
          sv[k][j] = in ? seg[i0 + j] : (L)0;
          xv[k][j] = in ? x[i0 + j] : 0.f;
        }
      }
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        if (!(sv[k][j] > (L)0)) continue;
        const float v = xv[k][j];
        if (!isfinite(v)) {
          ++bad;
          continue;
        }
        if (MOMENT == 1) {
          acc += (double)v;
          ++cnt;
          mn = fminf(mn, v);
          mx = fmaxf(mx, v);
        } else if (MOMENT == 2) {
          const double d = (double)v - mean;
          acc += d * d;
        }
        const unsigned key = key_of(v);
        int t = 0;
        if (prefix_bits > 0) {
          const unsigned p = key >> prefix_shift;
          t = -1;
#pragma unroll
          for (int q = 0; q < MAXT; ++q)
            if (q < T && pre.p[q] == p) t = q;
        }
        if (t >= 0) atomicAdd(&hist[t * BINS + (int)((key >> digit_shift) & digit_mask)], 1u);
      }
    }
  }
  __syncthreads();
  unsigned *slab = slabs + (size_t)blockIdx.x * nbin;
  for (int i = threadIdx.x; i < nbin; i += 256) slab[i] = hist[i];
  if (MOMENT == 0) return;
  // fixed tree: the 64 lanes of a wave, then the four waves in order
  acc = wave_sum_d(acc);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    cnt += __shfl_xor(cnt, o, 64);
    bad += __shfl_xor(bad, o, 64);
    mn = fminf(mn, __shfl_xor(mn, o, 64));
    mx = fmaxf(mx, __shfl_xor(mx, o, 64));
  }
  if ((threadIdx.x & 63) == 0) {
    const int w = threadIdx.x >> 6;
    red_d[w] = acc;
    red_c[w] = cnt;
    red_n[w] = bad;
    red_mn[w] = mn;
    red_mx[w] = mx;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    FpPartial r;
    r.sum = ((red_d[0] + red_d[1]) + red_d[2]) + red_d[3];
    r.count = red_c[0] + red_c[1] + red_c[2] + red_c[3];
    r.nonfinite = red_n[0] + red_n[1] + red_n[2] + red_n[3];
    r.mn = fminf(fminf(red_mn[0], red_mn[1]), fminf(red_mn[2], red_mn[3]));
    r.mx = fmaxf(fmaxf(red_mx[0], red_mx[1]), fmaxf(red_mx[2], red_mx[3]));
    partials[blockIdx.x] = r;
  }
}

// counters[i] += slab_0[i] + slab_1[i] + ... (ascending), one thread per counter
__global__ __launch_bounds__(256) void fp_reduce_hist_kernel(const unsigned *__restrict__ slabs, int nwg, int nbin,
                                                             unsigned long long *__restrict__ counters) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= nbin) return;
  unsigned long long s = 0;
  for (int w = 0; w < nwg; ++w) s += slabs[(size_t)w * nbin + i];
  counters[i] += s;
}

// One workgroup: the partials are staged in LDS, thread 0 adds them in workgroup order and folds the case into the state.
__global__ __launch_bounds__(256) void fp_reduce_moments_kernel(const FpPartial *__restrict__ partials, int nwg, int moment,
                                                                long long case_index, DgttaFingerprintState *__restrict__ state) {
  __shared__ FpPartial part[MAX_WG];
  for (int i = threadIdx.x; i < nwg; i += 256) part[i] = partials[i];
  __syncthreads();
  if (threadIdx.x != 0) return;
  double sum = 0.0;
  unsigned long long cnt = 0, bad = 0;
  float mn = INFINITY, mx = -INFINITY;
  for (int i = 0; i < nwg; ++i) {
    sum += part[i].sum;
    cnt += part[i].count;
    bad += part[i].nonfinite;
    mn = fminf(mn, part[i].mn);
    mx = fmaxf(mx, part[i].mx);
  }
  if (moment == 1) {
    state->count += cnt;
    state->nonfinite += bad;
    if (bad != 0 && state->first_nonfinite_case < 0) state->first_nonfinite_case = case_index;
    if ((double)mn < state->min) state->min = (double)mn;
    if ((double)mx > state->max) state->max = (double)mx;
    state->sum = state->sum + sum;
  } else {
    state->sumsq_centred = state->sumsq_centred + sum;
  }
}

template <typename L>
void fp_launch(int moment, int nwg, hipStream_t st, const float *x, const void *seg, int64_t V, int prefix_bits, int digit_shift,
               unsigned digit_mask, const FpPrefixes &pre, int T, double mean, unsigned *slabs, FpPartial *partials) {
  const L *s = (const L *)seg;
  if (moment == 1)
    hipLaunchKernelGGL((fp_sweep_kernel<L, 1>), dim3(nwg), dim3(256), 0, st, x, s, V, prefix_bits, digit_shift, digit_mask, pre, T,
                       mean, slabs, partials);
  else if (moment == 2)
    hipLaunchKernelGGL((fp_sweep_kernel<L, 2>), dim3(nwg), dim3(256), 0, st, x, s, V, prefix_bits, digit_shift, digit_mask, pre, T,
                       mean, slabs, partials);
  else
    hipLaunchKernelGGL((fp_sweep_kernel<L, 0>), dim3(nwg), dim3(256), 0, st, x, s, V, prefix_bits, digit_shift, digit_mask, pre, T,
                       mean, slabs, partials);
}

inline size_t fp_slab_bytes(int nwg, int T) { return align_up((size_t)nwg * T * BINS * sizeof(unsigned), 32); }

}  // namespace

extern "C" size_t dgtta_fingerprint_ws_bytes(int64_t V, int n_prefixes) {
  if (V < 1 || n_prefixes < 1 || n_prefixes > MAXT) return 0;
  const int nwg = fp_workgroups(V);
  return fp_slab_bytes(nwg, n_prefixes) + (size_t)nwg * sizeof(FpPartial);
}

extern "C" int dgtta_fingerprint_sweep(const float *x, const void *seg, int seg_dtype, int64_t V, int moment, double mean,
                                       int64_t case_index, int prefix_bits, int digit_bits, const uint32_t *h_prefixes,
                                       int n_prefixes, uint64_t *counters, DgttaFingerprintState *state, void *ws, size_t ws_bytes,
                                       void *stream) {
  DG_REQUIRE(x && seg && counters && ws, DGTTA_ERR_BADARG, "fingerprint_sweep: null pointer");
  DG_REQUIRE(V >= 1, DGTTA_ERR_BADARG, "fingerprint_sweep: a case has at least one voxel (got %lld)", (long long)V);
  DG_REQUIRE(moment >= 0 && moment <= 2, DGTTA_ERR_BADARG, "fingerprint_sweep: moment %d not in 0..2", moment);
  DG_REQUIRE(moment == 0 || state != nullptr, DGTTA_ERR_BADARG, "fingerprint_sweep: a moment sweep needs the state");
  DG_REQUIRE(moment != 2 || isfinite(mean), DGTTA_ERR_BADARG, "fingerprint_sweep: the centred sweep needs a finite mean");
  DG_REQUIRE(digit_bits >= 1 && (1 << digit_bits) <= BINS && prefix_bits >= 0 && prefix_bits + digit_bits <= 32, DGTTA_ERR_BADARG,
             "fingerprint_sweep: bad digits (prefix of %d bits, digit of %d; a digit has at most 11)", prefix_bits, digit_bits);
  DG_REQUIRE(n_prefixes >= 1 && n_prefixes <= MAXT && (prefix_bits > 0 || n_prefixes == 1), DGTTA_ERR_BADARG,
             "fingerprint_sweep: 1..%d prefixes, one when the prefix is empty (got %d)", MAXT, n_prefixes);
  DG_REQUIRE(prefix_bits == 0 || h_prefixes != nullptr, DGTTA_ERR_BADARG, "fingerprint_sweep: null prefix table");
  DG_REQUIRE(((uintptr_t)ws & 7) == 0, DGTTA_ERR_WORKSPACE, "fingerprint_sweep: workspace must be 8-byte aligned");
  const size_t need = dgtta_fingerprint_ws_bytes(V, n_prefixes);
  DG_REQUIRE(ws_bytes >= need, DGTTA_ERR_WORKSPACE, "fingerprint_sweep: workspace of %zu bytes, %zu needed (dgtta_fingerprint_ws_bytes)",
             ws_bytes, need);
  FpPrefixes pre;
  for (int j = 0; j < MAXT; ++j) pre.p[j] = 0u;
  for (int j = 0; j < n_prefixes && prefix_bits > 0; ++j) {
    DG_REQUIRE(prefix_bits == 32 || (h_prefixes[j] >> prefix_bits) == 0, DGTTA_ERR_BADARG,
               "fingerprint_sweep: prefix %d has more than %d bits", j, prefix_bits);
    for (int k = 0; k < j; ++k)
      DG_REQUIRE(h_prefixes[k] != h_prefixes[j], DGTTA_ERR_BADARG, "fingerprint_sweep: prefixes %d and %d are equal", k, j);
    pre.p[j] = h_prefixes[j];
  }
  hipStream_t st = (hipStream_t)stream;
  const int nwg = fp_workgroups(V);
  unsigned *slabs = (unsigned *)ws;
  FpPartial *partials = (FpPartial *)((char *)ws + fp_slab_bytes(nwg, n_prefixes));
  const int digit_shift = 32 - prefix_bits - digit_bits;
  const unsigned digit_mask = (1u << digit_bits) - 1u;
  if (seg_dtype == DGTTA_SEG_U8)
    fp_launch<uint8_t>(moment, nwg, st, x, seg, V, prefix_bits, digit_shift, digit_mask, pre, n_prefixes, mean, slabs, partials);
  else if (seg_dtype == DGTTA_SEG_I16)
    fp_launch<int16_t>(moment, nwg, st, x, seg, V, prefix_bits, digit_shift, digit_mask, pre, n_prefixes, mean, slabs, partials);
  else if (seg_dtype == DGTTA_SEG_I32)
    fp_launch<int32_t>(moment, nwg, st, x, seg, V, prefix_bits, digit_shift, digit_mask, pre, n_prefixes, mean, slabs, partials);
  else
    DG_REQUIRE(false, DGTTA_ERR_BADARG, "fingerprint_sweep: label type %d (DGTTA_SEG_U8 / I16 / I32)", seg_dtype);
  DG_CHECK_LAUNCH("fp_sweep_kernel");
  const int nbin = n_prefixes * BINS;
  hipLaunchKernelGGL(fp_reduce_hist_kernel, dim3(cdiv(nbin, 256)), dim3(256), 0, st, slabs, nwg, nbin, (unsigned long long *)counters);
  DG_CHECK_LAUNCH("fp_reduce_hist_kernel");
  if (moment != 0) {
    hipLaunchKernelGGL(fp_reduce_moments_kernel, dim3(1), dim3(256), 0, st, partials, nwg, moment, (long long)case_index, state);
    DG_CHECK_LAUNCH("fp_reduce_moments_kernel");
  }
  return DGTTA_OK;
}
