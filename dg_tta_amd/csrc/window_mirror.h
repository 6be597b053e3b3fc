// Mirror masks of nnU-Net's mirroring (training: MirrorTransform, inference: the mirrored passes of a sliding window), shared by
// window_features.hip, window_logits.hip and mirror.hip.  Bit 0 = axis 0 (D), bit 1 = axis 1 (H), bit 2 = axis 2 (W) of a
// [PD][PH][PW] block.  A flip is its own inverse, so the same index map gathers a flipped input and un-flips an output.
#pragma once
#include <cstdint>

constexpr int WM_MASKS = 8;      // masks 0..7

// voxel index of (pd, ph, pw) mirrored along the axes of `mirror`, inside the [PD][PH][PW] block
__device__ __forceinline__ int64_t wm_source(int mirror, int64_t pd, int ph, int pw, int PD, int PH, int PW) {
  const int64_t sd = (mirror & 1) ? PD - 1 - pd : pd;
  const int sh = (mirror & 2) ? PH - 1 - ph : ph;
  const int sw = (mirror & 4) ? PW - 1 - pw : pw;
  return (sd * PH + sh) * PW + sw;
}
