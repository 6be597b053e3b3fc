// What the sliding-window accumulations (window_features.hip, window_logits.hip) share: where a window lies in the volume and how it
// is mirrored - one descriptor that the extern "C" entry points fill once, the host checks in the words they are reported with, and
// the index arithmetic of the kernels, which take the descriptor by value.
#pragma once
#include "common.h"
#include "window_mirror.h"

// A [PD][PH][PW] window at (x0, y0, z0) of the [X][Y][Z] volume; mirror: the mask of the pass that produced it (window_mirror.h)
struct WindowPlace {
  int PD, PH, PW, X, Y, Z, x0, y0, z0, mirror;
};

// `also`: a further condition of the caller's that is reported in the same words (window_accumulate: a positive class count)
static inline int window_place_check(const char *who, const WindowPlace &w, bool also = true) {
  DG_REQUIRE(w.mirror >= 0 && w.mirror < WM_MASKS, DGTTA_ERR_BADARG, "%s: mirror mask %d outside 0..7", who, w.mirror);
  DG_REQUIRE(also && w.PD > 0 && w.PH > 0 && w.PW > 0 && w.x0 >= 0 && w.y0 >= 0 && w.z0 >= 0 && w.x0 + w.PD <= w.X && w.y0 + w.PH <= w.Y &&
                 w.z0 + w.PW <= w.Z,
             DGTTA_ERR_BADARG, "%s: window outside the volume", who);
  return DGTTA_OK;
}

// storage type of a logits-space accumulator
static inline int window_acc_check(const char *who, int acc_dtype, int mirror) {
  DG_REQUIRE(acc_dtype == DGTTA_F32 || acc_dtype == DGTTA_F16, DGTTA_ERR_UNSUPPORTED, "%s: the accumulator is fp32 or fp16 (acc_dtype %d)",
             who, acc_dtype);
  DG_REQUIRE(!mirror || acc_dtype == DGTTA_F32, DGTTA_ERR_UNSUPPORTED, "%s: a mirrored pass needs the fp32 accumulator", who);
  return DGTTA_OK;
}

// voxel p of a [PD][PH][L] block (L = PW: the window; shorter: a segment of its last axis)
struct WindowVoxel {
  int64_t pd;
  int ph, pw;
};
__device__ __forceinline__ WindowVoxel wp_voxel(int64_t p, int PH, int L) {
  return {p / ((int64_t)L * PH), (int)((p / L) % PH), (int)(p % L)};
}
// window voxel (pd, ph, pw): its index in the volume, in the window, and in the window as the pass produced it (MIR: mirrored).
// PD: int where a kernel walks rows (the first product then is a 32-bit one), int64_t where it decodes a linear index
template <typename PD>
__device__ __forceinline__ int64_t wp_volume(const WindowPlace &w, PD pd, int ph, int pw) {
  return ((int64_t)(pd + w.x0) * w.Y + (ph + w.y0)) * w.Z + (pw + w.z0);
}
template <typename PD>
__device__ __forceinline__ int64_t wp_window(const WindowPlace &w, PD pd, int ph, int pw) {
  return ((int64_t)pd * w.PH + ph) * w.PW + pw;
}
template <bool MIR, typename PD>
__device__ __forceinline__ int64_t wp_source(const WindowPlace &w, PD pd, int ph, int pw) {
  return MIR ? wm_source(w.mirror, pd, ph, pw, w.PD, w.PH, w.PW) : wp_window(w, pd, ph, pw);
}
