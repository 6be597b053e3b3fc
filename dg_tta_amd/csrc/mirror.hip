// nnU-Net's mirroring as data movement (restated from memory of nnunetv2 2.2 / batchgenerators, UNPINNED):
//   dgtta_mirror_batch    MirrorTransform of pre-training: image [B][C][D][H][W] fp32 and labels [B][D][H][W] int64, source to
//                         destination, item b flipped along the axes of h_masks[b] (mask 0: copied) - one launch per 16 items;
//   dgtta_window_gather   the network input of sliding-window inference with mirroring: window k of the batch [n][C][PD][PH][PW] is
//                         the block of the resident volume [C][X][Y][Z] at h_origins[k], flipped along the axes of h_masks[k].
// Mask bits as in window_mirror.h.  One thread per destination element: a wave's stores cover one contiguous run and its loads cover
// one contiguous run per window row - the same run, read in reverse order when the last axis is flipped.  The masks and origins are
// HOST arrays copied into the kernel arguments: nothing is uploaded, nothing is allocated, nothing waits for the stream.
#include "gfx950.h"
#include "window_mirror.h"

namespace {

struct MirrorItems {
  int x0[DGTTA_MIRROR_MAX_ITEMS], y0[DGTTA_MIRROR_MAX_ITEMS], z0[DGTTA_MIRROR_MAX_ITEMS], mask[DGTTA_MIRROR_MAX_ITEMS];
};

// blockIdx.y = item; i < C V: image element (c, p), else label element p
__global__ __launch_bounds__(256) void mirror_batch_kernel(const MirrorItems items, const float *__restrict__ img, const int64_t *__restrict__ lab,
                                                           float *__restrict__ img_out, int64_t *__restrict__ lab_out, int C, int D, int H,
                                                           int W, int64_t V) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (C + 1) * V) return;
  const int b = (int)blockIdx.y;
  const int64_t c = i / V, p = i - c * V;
  const int pw = (int)(p % W), ph = (int)((p / W) % H);
  const int64_t pd = p / ((int64_t)W * H);
  const int64_t ps = wm_source(items.mask[b], pd, ph, pw, D, H, W);
  if (c < C) img_out[(b * (int64_t)C + c) * V + p] = img[(b * (int64_t)C + c) * V + ps];
  else lab_out[b * V + p] = lab[b * V + ps];
}

// blockIdx.y = window * C + channel
__global__ __launch_bounds__(256) void window_gather_kernel(const MirrorItems items, const float *__restrict__ vol, float *__restrict__ out, int C,
                                                            int PD, int PH, int PW, int Y, int Z, int64_t VOL, int64_t P) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= P) return;
  const int k = (int)blockIdx.y / C, c = (int)blockIdx.y % C;
  const int m = items.mask[k];
  const int pw = (int)(p % PW), ph = (int)((p / PW) % PH);
  const int pd = (int)(p / ((int64_t)PW * PH));
  const int sd = (m & 1) ? PD - 1 - pd : pd, sh = (m & 2) ? PH - 1 - ph : ph, sw = (m & 4) ? PW - 1 - pw : pw;
  const int64_t v = ((int64_t)(items.x0[k] + sd) * Y + (items.y0[k] + sh)) * Z + (items.z0[k] + sw);
  out[((int64_t)k * C + c) * P + p] = vol[c * VOL + v];
}

}  // namespace

extern "C" int dgtta_mirror_batch(const float *image, const int64_t *labels, float *image_out, int64_t *labels_out, const int *h_masks, int B,
                                  int C, int D, int H, int W, void *stream) {
  DG_REQUIRE(image && labels && image_out && labels_out && h_masks, DGTTA_ERR_BADARG, "mirror_batch: null pointer");
  DG_REQUIRE(image != image_out && labels != labels_out, DGTTA_ERR_BADARG, "mirror_batch: source and destination must differ");
  DG_REQUIRE(B >= 1 && C >= 1 && D > 0 && H > 0 && W > 0, DGTTA_ERR_BADARG, "mirror_batch: bad sizes");
  const int64_t V = (int64_t)D * H * W;
  const int64_t nblk = cdiv64((C + 1) * V, 256);
  DG_REQUIRE(V < (1ll << 31) && nblk < (1ll << 31), DGTTA_ERR_UNSUPPORTED, "mirror_batch: item too large");
  for (int b = 0; b < B; ++b)
    DG_REQUIRE(h_masks[b] >= 0 && h_masks[b] < WM_MASKS, DGTTA_ERR_BADARG, "mirror_batch: mask %d of item %d outside 0..7", h_masks[b], b);
  for (int b0 = 0; b0 < B; b0 += DGTTA_MIRROR_MAX_ITEMS) {
    const int nb = B - b0 < DGTTA_MIRROR_MAX_ITEMS ? B - b0 : DGTTA_MIRROR_MAX_ITEMS;
    MirrorItems items{};
    for (int b = 0; b < nb; ++b) items.mask[b] = h_masks[b0 + b];
    hipLaunchKernelGGL(mirror_batch_kernel, dim3((unsigned)nblk, (unsigned)nb), dim3(256), 0, (hipStream_t)stream, items, image + b0 * C * V,
                       labels + b0 * V, image_out + b0 * C * V, labels_out + b0 * V, C, D, H, W, V);
  }
  DG_CHECK_LAUNCH("mirror_batch_kernel");
  return DGTTA_OK;
}

extern "C" int dgtta_window_gather(const float *volume, float *out, const int *h_origins, const int *h_masks, int n, int C, int PD, int PH,
                                   int PW, int X, int Y, int Z, void *stream) {
  DG_REQUIRE(volume && out && h_origins && h_masks, DGTTA_ERR_BADARG, "window_gather: null pointer");
  DG_REQUIRE(n >= 1 && C >= 1 && C <= 4095 && PD > 0 && PH > 0 && PW > 0 && X > 0 && Y > 0 && Z > 0, DGTTA_ERR_BADARG, "window_gather: bad sizes");
  const int64_t P = (int64_t)PD * PH * PW;
  DG_REQUIRE(cdiv64(P, 256) < (1ll << 31), DGTTA_ERR_UNSUPPORTED, "window_gather: window too large");
  for (int k = 0; k < n; ++k) {
    const int x0 = h_origins[3 * k], y0 = h_origins[3 * k + 1], z0 = h_origins[3 * k + 2];
    DG_REQUIRE(x0 >= 0 && y0 >= 0 && z0 >= 0 && x0 <= X - PD && y0 <= Y - PH && z0 <= Z - PW, DGTTA_ERR_BADARG,
               "window_gather: window %d outside the volume", k);
    DG_REQUIRE(h_masks[k] >= 0 && h_masks[k] < WM_MASKS, DGTTA_ERR_BADARG, "window_gather: mask %d of window %d outside 0..7", h_masks[k], k);
  }
  for (int k0 = 0; k0 < n; k0 += DGTTA_MIRROR_MAX_ITEMS) {
    const int nk = n - k0 < DGTTA_MIRROR_MAX_ITEMS ? n - k0 : DGTTA_MIRROR_MAX_ITEMS;
    MirrorItems items{};
    for (int k = 0; k < nk; ++k) {
      items.x0[k] = h_origins[3 * (k0 + k)], items.y0[k] = h_origins[3 * (k0 + k) + 1], items.z0[k] = h_origins[3 * (k0 + k) + 2];
      items.mask[k] = h_masks[k0 + k];
    }
    hipLaunchKernelGGL(window_gather_kernel, dim3((unsigned)cdiv64(P, 256), (unsigned)(nk * C)), dim3(256), 0, (hipStream_t)stream, items, volume,
                       out + (int64_t)k0 * C * P, C, PD, PH, PW, Y, Z, (int64_t)X * Y * Z, P);
  }
  DG_CHECK_LAUNCH("window_gather_kernel");
  return DGTTA_OK;
}
