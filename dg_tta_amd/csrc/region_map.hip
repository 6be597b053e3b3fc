// The integer ends of region-based datasets (region_loss.hip's header: R sigmoid outputs, overlapping regions of a label map):
//   dgtta_region_counts   TP / FP / FN per region of the hard prediction z > 0 (sigmoid > 0.5) - nnU-Net's online pseudo-Dice
//                         of a region trainer, the counterpart of dgtta_argmax_dice's counts for the softmax case;
//   dgtta_logits_regions  the label map of accumulated region logits, nnU-Net's convert_probabilities_to_segmentation for
//                         regions: seg = 0; for i = 0 .. R-1 in order: seg[l_i > 0] = regions_class_order[i] - the LAST positive
//                         region in the order wins, a logit of exactly 0 is not in the region.  The ensemble-mean logit is a
//                         positive multiple of the accumulated sum, so the sign of the accumulator decides: no division.
// Both restated from memory of nnunetv2 2.2.1, UNPINNED.  The feature-space form of the label map is window_features.hip's.
// Integer sums only (LDS and global integer atomics): the same counts on every run.
#include "common.h"

namespace {

constexpr int RM_MAXR = 32;
constexpr int RM_MAXL = 1024;

struct RmOrder {
  int c[RM_MAXR];
};

// counts[0][r] = TP, counts[1][r] = FP, counts[2][r] = FN over the voxels whose label is inside the table
__global__ __launch_bounds__(256) void region_counts_kernel(const float *__restrict__ logits, int ldc, int R,
                                                            const int64_t *__restrict__ labels, const uint32_t *__restrict__ table,
                                                            int L, unsigned long long *__restrict__ counts, int64_t rows) {
  __shared__ uint32_t s_tab[RM_MAXL];
  __shared__ unsigned int s_cnt[3][RM_MAXR];
  const int t = threadIdx.x, lane = t & 63;
  for (int i = t; i < L; i += 256) s_tab[i] = table[i];
  if (t < 3 * RM_MAXR) s_cnt[t / RM_MAXR][t % RM_MAXR] = 0;
  __syncthreads();
  const uint32_t rmask = R == 32 ? 0xffffffffu : (1u << R) - 1u;
  for (int64_t v0 = (int64_t)blockIdx.x * 256; v0 < rows; v0 += (int64_t)gridDim.x * 256) {      // (uniform trip count: ballots below)
    const int64_t v = v0 + t;
    uint32_t pm = 0, tm = 0, on = 0;
    if (v < rows) {
      const int64_t yl = labels[v];
      if (yl >= 0 && yl < L) {
        on = rmask;
        tm = s_tab[yl];
        const float *row = logits + v * ldc;
        for (int r = 0; r < R; ++r) pm |= row[r] > 0.f ? 1u << r : 0u;
      }
    }
    const uint32_t tp = pm & tm & on, fp = pm & ~tm & on, fn = ~pm & tm & on;
    for (int r = 0; r < R; ++r) {
      const unsigned int a = __popcll(__ballot((tp >> r) & 1u)), b = __popcll(__ballot((fp >> r) & 1u)),
                         c = __popcll(__ballot((fn >> r) & 1u));
      if (lane == 0) {
        if (a) atomicAdd(&s_cnt[0][r], a);
        if (b) atomicAdd(&s_cnt[1][r], b);
        if (c) atomicAdd(&s_cnt[2][r], c);
      }
    }
  }
  __syncthreads();
  if (t < 3 * R) {
    const int k = t / R, r = t - k * R;
    if (s_cnt[k][r]) atomicAdd(&counts[k * R + r], (unsigned long long)s_cnt[k][r]);
  }
}

template <typename ACC>
__global__ __launch_bounds__(256) void logits_regions_kernel(const ACC *__restrict__ acc, int R, int64_t rows, RmOrder order,
                                                             int64_t *__restrict__ out) {
  __shared__ int s_ord[RM_MAXR];
  if (threadIdx.x < RM_MAXR) {
    int mine = 0;
#pragma unroll
    for (int k = 0; k < RM_MAXR; ++k) mine = (int)threadIdx.x == k ? order.c[k] : mine;      // (no runtime index into the kernel argument)
    s_ord[threadIdx.x] = mine;
  }
  __syncthreads();
  for (int64_t v = (int64_t)blockIdx.x * 256 + threadIdx.x; v < rows; v += (int64_t)gridDim.x * 256) {
    const ACC *row = acc + v * R;
    int lab = 0;
    for (int i = 0; i < R; ++i)
      if (ld_f<ACC>(row + i) > 0.f) lab = s_ord[i];
    out[v] = lab;
  }
}

}  // namespace

extern "C" int dgtta_region_counts(const float *logits, int ldc, int R, const int64_t *labels, const uint32_t *table, int L,
                                   int64_t *counts, int64_t rows, void *stream) {
  DG_REQUIRE(logits && labels && table && counts, DGTTA_ERR_BADARG, "region_counts: null pointer");
  DG_REQUIRE(R >= 1 && R <= RM_MAXR && ldc >= R && L >= 1 && L <= RM_MAXL && rows > 0, DGTTA_ERR_BADARG,
             "region_counts: need 1<=R<=%d, ldc>=R, 1<=L<=%d, rows>0 (R=%d ldc=%d L=%d)", RM_MAXR, RM_MAXL, R, ldc, L);
  // at most 2048 workgroups: a workgroup's 32-bit LDS counters then hold rows up to 2^43
  DG_REQUIRE(rows < (1ll << 43), DGTTA_ERR_UNSUPPORTED, "region_counts: too many rows");
  const int64_t nblk = cdiv64(rows, 256);
  if (hipMemsetAsync(counts, 0, (size_t)3 * R * sizeof(int64_t), (hipStream_t)stream) != hipSuccess) {
    dgtta_set_error("region_counts: cannot clear the counts");
    return DGTTA_ERR_LAUNCH;
  }
  hipLaunchKernelGGL(region_counts_kernel, dim3((unsigned)(nblk < 2048 ? nblk : 2048)), dim3(256), 0, (hipStream_t)stream, logits, ldc, R,
                     labels, table, L, (unsigned long long *)counts, rows);
  DG_CHECK_LAUNCH("region_counts_kernel");
  return DGTTA_OK;
}

extern "C" int dgtta_logits_regions(const void *acc, int acc_dtype, int R, int64_t rows, const int *h_order, int64_t *label_out,
                                    void *stream) {
  DG_REQUIRE(acc && h_order && label_out, DGTTA_ERR_BADARG, "logits_regions: null pointer");
  DG_REQUIRE(R >= 1 && R <= RM_MAXR && rows > 0, DGTTA_ERR_BADARG, "logits_regions: need 1<=R<=%d, rows>0 (R=%d)", RM_MAXR, R);
  DG_REQUIRE(acc_dtype == DGTTA_F32 || acc_dtype == DGTTA_F16, DGTTA_ERR_UNSUPPORTED, "logits_regions: rows are fp32 or fp16");
  RmOrder order{};
  for (int i = 0; i < R; ++i) {
    DG_REQUIRE(h_order[i] > 0, DGTTA_ERR_BADARG, "logits_regions: regions_class_order[%d] = %d is not a positive label", i, h_order[i]);
    order.c[i] = h_order[i];
  }
  const dim3 grid((unsigned)grid_for(rows));
  if (acc_dtype == DGTTA_F32)
    hipLaunchKernelGGL(logits_regions_kernel<float>, grid, dim3(256), 0, (hipStream_t)stream, (const float *)acc, R, rows, order, label_out);
  else
    hipLaunchKernelGGL(logits_regions_kernel<f16_t>, grid, dim3(256), 0, (hipStream_t)stream, (const f16_t *)acc, R, rows, order, label_out);
  DG_CHECK_LAUNCH("logits_regions_kernel");
  return DGTTA_OK;
}
