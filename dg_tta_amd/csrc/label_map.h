// Where the label of a loss voxel lives: the index map the label-reading loss kernels share (dice_ce.hip, region_loss.hip).
#pragma once
#include "common.h"

// where the label of voxel v of sample b lives: dense [B][V], or a strided view of a full-resolution map (h == 0: dense).
// Deep supervision: low-resolution voxel (i, j, k) of [d][h][w] reads the full-resolution map [d sd][h sh][w sw] at
// (i sd + sd / 2, j sh + sh / 2, k sw + sw / 2) - no downsampled label tensor exists (dice_ce.hip's header).
struct DcLabels {
  int h, w, sd, sh, sw;
  int64_t H, W, Vfull;
  __device__ __forceinline__ int64_t at(int b, int64_t v, int64_t V) const {
    if (h == 0) return (int64_t)b * V + v;
    const int64_t i = v / ((int64_t)h * w), rem = v - i * ((int64_t)h * w);
    const int64_t j = rem / w, k = rem - j * w;
    return (int64_t)b * Vfull + ((i * sd + sd / 2) * H + (j * sh + sh / 2)) * W + (k * sw + sw / 2);
  }
};

static const DcLabels DC_DENSE = {0, 0, 1, 1, 1, 0, 0, 0};

static inline bool dc_ds_dims_ok(int d, int h, int w, int sd, int sh, int sw) {
  return d > 0 && h > 0 && w > 0 && sd > 0 && sh > 0 && sw > 0 && (int64_t)d * sd < (1ll << 31) && (int64_t)h * sh < (1ll << 31) &&
         (int64_t)w * sw < (1ll << 31);
}
static inline DcLabels dc_ds_labels(int d, int h, int w, int sd, int sh, int sw) {
  DcLabels lm = {h, w, sd, sh, sw, (int64_t)h * sh, (int64_t)w * sw, (int64_t)d * sd * h * sh * w * sw};
  return lm;
}
