/*
 * dgtta.h — C ABI of libdgtta_hip.so: hand-written gfx950 (MI355X / CDNA4) kernels for the
 * DG-TTA test-time-adaptation hot path.
 *
 * The reference (multimodallearning/DG-TTA) is pure Python on stock PyTorch ops and has no FFI of
 * its own; this ABI is the drop-in boundary that sits UNDER the reference's Python operator
 * signatures (dg_tta_amd/ mirrors those).  Each entry point cites the reference code it replaces
 * (paths relative to /root/reference).  INTEGRATION.md shows the ctypes binding a maintainer adds.
 *
 * Conventions
 *  - plain pointers + sizes, no torch types; all pointers are DEVICE pointers unless named h_*.
 *  - every call only ENQUEUES work on `stream` (a hipStream_t passed as void*) and returns;
 *    nothing here allocates, frees or synchronises, so calls may be captured into a hipGraph.
 *  - the caller owns all memory, including workspaces (sizes from the *_ws_bytes queries).
 *  - return value: 0 = OK, <0 = DGTTA_ERR_*; dgtta_last_error() gives a thread-local message.
 *  - volumes are D x H x W (W fastest).  Layouts:
 *        NCDHW  [B][C][D][H][W]          (PyTorch contiguous; the reference's layout)
 *        NDHWC  [B][D][H][W][ldc]        (channels-last; `ldc` >= C elements per voxel, so a
 *                                          tensor may be a channel slice of a wider buffer)
 *  - dtype: 0 = fp32, 1 = bf16, 2 = fp16 (storage of activations and packed weights; accumulation, statistics,
 *    weight gradients and the optimizer state are always fp32).  fp16 gradients need the caller's static loss scale
 *    (dgtta_adamw_step divides it out).
 */
#ifndef DGTTA_H
#define DGTTA_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DGTTA_OK 0
#define DGTTA_ERR_BADARG (-1)
#define DGTTA_ERR_UNSUPPORTED (-2)
#define DGTTA_ERR_WORKSPACE (-3)
#define DGTTA_ERR_LAUNCH (-4)

#define DGTTA_F32 0
#define DGTTA_BF16 1
#define DGTTA_F16 2

#define DGTTA_PAD_ZEROS 0
#define DGTTA_PAD_BORDER 1
#define DGTTA_INTERP_LINEAR 0
#define DGTTA_INTERP_NEAREST 1

int dgtta_version(void);
const char *dgtta_last_error(void);
/* The DGTTA_* diagnostic switches are read from the environment once, at first use; this call takes a
 * fresh snapshot (tests that flip a switch inside one process call it after changing the environment). */
int dgtta_reload_env(void);

/* ---------------------------------------------------------------------------------------------
 * MIND3D descriptor.  Replaces MIND3D.forward + smooth + filter1D (dg_tta/mind.py:142-164, :27-43,
 * :5-24) and mind_hook (:167-168).  img [B,1,D,H,W] fp32; noise [B,12,D,H,W] fp32 = the
 * torch.randn_like draw of mind.py:150 (caller supplies it so RNG semantics stay the caller's).
 * out: 12 channels, either NCDHW fp32 (out_ndhwc=0) or NDHWC with row length out_ldc (>=12;
 * channels 12..out_ldc-1 are written as zero) in out_dtype.  delta (mind.py:98,137: neighbour distance,
 * 1 or 2) and the Gaussian taps of `sigma` (h_taps: HOST array of 3 / 5 / 7 floats evaluated as mind.py:30-37
 * does, i.e. sigma <= 2; the reference itself only ever uses delta = 1, sigma = 1).
 * ws: dgtta_mind3d_ws_bytes(B,D,H,W) bytes.
 * ------------------------------------------------------------------------------------------- */
size_t dgtta_mind3d_ws_bytes(int B, int D, int H, int W);
int dgtta_mind3d_fwd(const float *img, const float *noise, float randn_weighting, int delta, const float *h_taps,
                     int ntaps, void *out, int out_ndhwc, int out_ldc, int out_dtype, void *ws, size_t ws_bytes, int B,
                     int D, int H, int W, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Seeded MIND noise: a counter-based stand-in for the randn draw of mind.py:150 that needs no noise
 * tensor and no generator state.  It is NOT torch.randn's stream.  n[b,c,d,h,w], c in 0..11, is
 *   (x0,x1,x2,x3) = Philox4x32-10(counter = (v, 4*b + c/4, offset_lo, offset_hi), key = (seed_lo, seed_hi))
 *         v = (d*H + h)*W + w  (< 2^31),  b = b0 + the sample's index inside the call (b0 + B <= 2^29)
 *   u_i = ((x_i >> 9) + 0.5) * 2^-23                    exact in fp32, in (0,1)
 *   c%4 == 0: sqrt(-2 ln u0) cos(2 pi u1)   1: sqrt(-2 ln u0) sin(2 pi u1)
 *         2: sqrt(-2 ln u2) cos(2 pi u3)   3: sqrt(-2 ln u2) sin(2 pi u3)
 * Philox4x32-10 as published (Random123): multipliers 0xD2511F53 (on counter word 0) and 0xCD9E8D57 (on
 * word 2), key increments 0x9E3779B9 / 0xBB67AE85, 10 rounds with the key bumped between rounds, round
 * output (hi1^c1^k0, lo1, hi0^c3^k1, lo0); counter 0 / key 0 gives 6627e8d5 e169c58d bc57ac4c 9b00dbd8.
 * A value depends on (seed, offset, b, c, v) only: not on tiling, grouping or launch geometry.
 *
 * noise_fill: writes that field as [B,12,D,H,W] fp32 (the testable face of the definition; also for
 * callers who want the tensor).
 * fwd_seeded: dgtta_mind3d_fwd with the field generated inside the descriptor kernel where the tensor
 * form loads it (voxels of the replicate-padded halo take the noise of the clamped voxel, as there);
 * same checks, workspace and outputs.  fwd_seeded(img, seed, ...) equals fwd(img, noise_fill(seed, ...))
 * up to the last bits of the library's log / sincos between two kernels.
 * ------------------------------------------------------------------------------------------- */
int dgtta_mind3d_noise_fill(float *noise, uint64_t seed, uint64_t offset, int b0, int B, int D, int H, int W,
                            void *stream);
int dgtta_mind3d_fwd_seeded(const float *img, uint64_t seed, uint64_t offset, int b0, float randn_weighting, int delta,
                            const float *h_taps, int ntaps, void *out, int out_ndhwc, int out_ldc, int out_dtype,
                            void *ws, size_t ws_bytes, int B, int D, int H, int W, void *stream);

/* ---------------------------------------------------------------------------------------------
 * GIN random-convolution chain.  Replaces GINGroupConv.forward / GradlessGCReplayNonlinBlock.forward
 * (dg_tta/gin.py:168-230, :59-122) for gin_aug's fixed config (1->2->2->2->1 channels, 4 layers).
 * x,out [B,1,D,H,W] fp32.  alpha [B].  ksz[4] HOST ints in {1,3}.  ker[l] = device pointer to
 * [B*cout_l, cin_l, k,k,k] fp32 exactly as drawn at gin.py:94-97; shift[l] = [B*cout_l] (gin.py:98-103).
 * ws: dgtta_gin_ws_bytes(B,D,H,W).
 * ------------------------------------------------------------------------------------------- */
size_t dgtta_gin_ws_bytes(int B, int D, int H, int W);
int dgtta_gin_chain_fwd(const float *x, const float *alpha, const int *h_ksz, const float *const *h_ker,
                        const float *const *h_shift, float *out, void *ws, size_t ws_bytes, int B, int D, int H,
                        int W, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Affine resampling = F.affine_grid + F.grid_sample(align_corners=False) without materialising
 * the grid.  Replaces the call sites dg_tta/tta/tta.py:523-551 (image, border), :572-575 (logits,
 * zeros) and dg_tta/tta/torch_utils.py:55-73 (get_batch; zeros; linear / nearest).
 * theta [B,3,4] fp32 device (x,y,z order of F.affine_grid).  If tta_grid_algebra != 0 the sampling
 * grid is formed as ((affine_grid(theta) - identity) + identity) in fp32, as tta.py:523-548 does.
 * src [B,C,Ds,Hs,Ws] / dst [B,C,Dd,Hd,Wd], layout NCDHW (ndhwc=0) or NDHWC with row lengths
 * src_ldc/dst_ldc.  fp32 only.  If sub_const_dev != NULL the scalar it points to is subtracted
 * before and added back after sampling (get_batch's "(img - img_min) ... + img_min", torch_utils.py:55-73).
 * bwd: grad_src = d(dst)/d(src)^T grad_dst (linear only; theta gets no gradient, as in the
 * reference where R is a constant).  grad_src is overwritten; it needs no initialisation.
 * ------------------------------------------------------------------------------------------- */
int dgtta_affine_warp3d_fwd(const float *src, const float *theta, float *dst, int B, int C, int Ds, int Hs,
                            int Ws, int Dd, int Hd, int Wd, int ndhwc, int src_ldc, int dst_ldc, int pad_mode,
                            int interp_mode, int tta_grid_algebra, const float *sub_const_dev, void *stream);
int dgtta_affine_warp3d_bwd(const float *grad_dst, const float *theta, float *grad_src, int B, int C, int Ds,
                            int Hs, int Ws, int Dd, int Hd, int Wd, int ndhwc, int src_ldc, int dst_ldc,
                            int pad_mode, int tta_grid_algebra, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Deformable spatial augmentation (spatial_aug_type = "deformable").  Replaces get_rf_field and the
 * inverse-consistent branch of calc_consistent_diffeomorphic_field (dg_tta/tta/augmentation_utils.py:8-43,
 * :46-135) as get_disp_field composes them (:138-153, without the keyword get_rf_field does not take), and
 * the two F.grid_sample calls of calc_branch through the dense grids (dg_tta/tta/tta.py:534-575).  fp32 only.
 *
 * rf_field: draw [P][Dl][Hl][Wl] = the torch.randn draw of P = batch * fields planes (the caller supplies it,
 * so RNG semantics stay the caller's) -> three k^3 box filters (avg_pool3d, stride 1, padding k/2 counted in
 * the divisor; k odd, every low-resolution axis >= k) -> trilinear upsampling to [P][D][H][W]
 * (align_corners=False) -> per plane (x - mean) / (1e-3 + unbiased std).  ws: dgtta_rf_field_ws_bytes.
 *
 * diffeo_fields: field [N][3][D][H][W] -> disp, inverse [N][D][H][W][3] (the permuted layout the reference
 * returns): field * factor / [D,H,W] / 2^time_steps / time_steps, time_steps iterations of
 * d' = d/2 - sample(i, id + d)/2, i' = i/2 - sample(d, id + i)/2 (grid_sample border, align_corners=True,
 * inverse starting at 0), then * 2^time_steps * [D,H,W].  As the reference writes it, channel c is scaled by
 * the c-th of (D, H, W) while it displaces the c-th of (x, y, z).  ws: dgtta_diffeo_fields_ws_bytes.
 *
 * dense_warp3d: dst = F.grid_sample(src, (0 * identity + disp) + identity, align_corners=False), identity =
 * F.affine_grid(eye) evaluated in the kernel; src / dst [B,C,D,H,W] NCDHW or NDHWC as in dgtta_affine_warp3d_*,
 * disp [B][D][H][W][3] (x, y, z).  bwd: grad_src = adjoint w.r.t. src (disp gets no gradient; the fields are
 * built without autograd in the reference).  grad_src is overwritten; it is summed with fp32 atomics, so its
 * last bits depend on the order in which the additions arrive.
 * ------------------------------------------------------------------------------------------- */
size_t dgtta_rf_field_ws_bytes(int P, int Dl, int Hl, int Wl);
int dgtta_rf_field_fwd(const float *draw, float *field, void *ws, size_t ws_bytes, int P, int k, int Dl, int Hl, int Wl,
                       int D, int H, int W, void *stream);
size_t dgtta_diffeo_fields_ws_bytes(int N, int D, int H, int W);
int dgtta_diffeo_fields(const float *field, float factor, float *disp, float *inverse, void *ws, size_t ws_bytes, int N,
                        int D, int H, int W, int time_steps, void *stream);
int dgtta_dense_warp3d_fwd(const float *src, const float *disp, float *dst, int B, int C, int D, int H, int W, int ndhwc,
                           int src_ldc, int dst_ldc, int pad_mode, void *stream);
int dgtta_dense_warp3d_bwd(const float *grad_dst, const float *disp, float *grad_src, int B, int C, int D, int H, int W,
                           int ndhwc, int src_ldc, int dst_ldc, int pad_mode, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Consistency loss.  Replaces dg_tta/tta/tta.py:263-271 + soft_dice_loss (torch_utils.py:90-104):
 * mask=(sum_c a>0)(sum_c b>0); sm=softmax_c * mask; dice_c = mean(2ab)/mean((a+b)^2/2);
 * loss = 1 - mean_{b, c>=start_class} dice.  la, lb: logits NDHWC [B][V][ldc], C classes, fp32.
 * fwd writes dice[B*C], loss[1] and keeps what bwd needs in ws.  bwd writes grad_la/grad_lb
 * (same layout) = grad_scale * (grad_scale_dev ? *grad_scale_dev : 1) * dloss/dlogits (mask treated as
 * a constant, as autograd does; the device scalar lets autograd's upstream gradient stay on the GPU).
 * guard_items: soft_dice_loss's "denominator.sum() == 0 -> dice = 1" guard is evaluated per group of
 * guard_items consecutive batch items (B = one reference call; 1 = every item is its own call, used
 * when several accumulation steps of batch size 1 run as one batch).  Must divide B.
 * ------------------------------------------------------------------------------------------- */
size_t dgtta_softdice_ws_bytes(int B, int C, int64_t V);
int dgtta_softdice_fwd(const float *la, const float *lb, float *dice, float *loss, void *ws, size_t ws_bytes,
                       int B, int C, int64_t V, int ldc, int start_class, int guard_items, void *stream);
int dgtta_softdice_bwd(const float *la, const float *lb, float *grad_la, float *grad_lb, const void *ws,
                       float grad_scale, const float *grad_scale_dev, int B, int C, int64_t V, int ldc,
                       int start_class, void *stream);
/* dgtta_softdice_bwd with the gradient rows in `grad_dtype` (DGTTA_F32: the call above; DGTTA_BF16 / DGTTA_F16: the 16-class
 * form only - C = ldc = 16 - each value rounded once on the way out; what dgtta_seghead_warp_bwd_g16 consumes). */
int dgtta_softdice_bwd_t(const float *la, const float *lb, void *grad_la, void *grad_lb, const void *ws, float grad_scale,
                         const float *grad_scale_dev, int B, int C, int64_t V, int ldc, int start_class, int grad_dtype,
                         void *stream);

/* Stand-alone soft_dice_loss(smp_a, smp_b) -> dice[B][C] of the reference (dg_tta/tta/torch_utils.py:90-104) on
 * probability maps: nom = mean_v(2ab), den = mean_v((a+b)^2)/2, dice = nom/den, all ones when den.sum() == 0.
 * a, b: fp32 [B][C][V] addressed with element strides (stride_b, stride_c, stride_v): NCDHW has stride_v = 1,
 * channels-last stride_c = 1.  bwd: grad_a / grad_b (same strides) = sum_c grad_dice[b][c] * d dice / d a.
 * ws: dgtta_softdice_ws_bytes(B, C, V), kept between fwd and bwd. */
int dgtta_softdice_probs_fwd(const float *a, const float *b, float *dice, void *ws, size_t ws_bytes, int B, int C,
                             int64_t V, int64_t stride_b, int64_t stride_c, int64_t stride_v, void *stream);
int dgtta_softdice_probs_bwd(const float *a, const float *b, const float *grad_dice, float *grad_a, float *grad_b,
                             const void *ws, int B, int C, int64_t V, int64_t stride_b, int64_t stride_c,
                             int64_t stride_v, void *stream);

/* Supervised loss of the PRE-TRAINING side: soft Dice + cross-entropy against an integer label map -
 * nnU-Net's DC_and_CE_loss [3P nnunetv2==2.2.1], the loss of the nnUNetTrainer the reference's trainers inherit
 * (dg_tta/pretraining/nnUNetTrainer_GIN.py:38-59, nnUNetTrainer_MIND.py:37-57, nnUNetTrainer_GIN_MIND.py:38-59):
 *   p = softmax_c(logits);  voxels whose label is outside [0, C) are ignored
 *   loss3[0] = loss3[1] + loss3[2];  loss3[1] = -mean_v log p[v][y_v];  loss3[2] = -mean_{b, c >= (do_bg ? 0 : 1)} dice[b][c]
 *   dice[b][c] = (2 sum_v p y + smooth) / (sum_v p + sum_v y + smooth)          (per sample: batch_dice = False)
 * logits / grad_logits: voxel-major fp32 [B][V][ld], labels int64 [B][V].  bwd: grad_logits = grad_scale * (*grad_scale_dev
 * if given) * d loss3[0] / d logits.  ws: dgtta_dice_ce_ws_bytes(B, C, V), kept between fwd and bwd.  1 <= B <= 8, C <= 128. */
size_t dgtta_dice_ce_ws_bytes(int B, int C, int64_t V);
int dgtta_dice_ce_fwd(const float *logits, int ldc, const int64_t *labels, float *loss3, float *dice, void *ws,
                      size_t ws_bytes, int B, int C, int64_t V, float smooth, int do_bg, void *stream);
int dgtta_dice_ce_bwd(const float *logits, int ldc, const int64_t *labels, const void *ws, float grad_scale,
                      const float *grad_scale_dev, float *grad_logits, int ldg, int B, int C, int64_t V, void *stream);
/* The same loss at a lower resolution (deep supervision): logits / grad_logits fp32 [B][d][h][w][ld], labels_full the
 * FULL-resolution int64 map [B][d sd][h sh][w sw] with integer strides; the label of low-resolution voxel (i, j, k) is
 * labels_full[i sd + sd / 2][j sh + sh / 2][k sw + sw / 2] (integer division) - the voxel an order-0 resize with half-pixel
 * centres and round-half-up picks.  Restated from memory of nnU-Net's DownsampleSegForDSTransform2 [3P nnunetv2==2.2.1, not
 * available here]: UNPINNED.  No downsampled label tensor is materialised.  Same smooth / do_bg / ignore rule / loss3 / dice
 * / ws contract as above with V = d h w; the per-scale weight of the multi-scale loss goes in through grad_scale(_dev).
 * Strides (1, 1, 1) give dgtta_dice_ce_fwd / _bwd bit for bit. */
size_t dgtta_dice_ce_ds_ws_bytes(int B, int C, int d, int h, int w);
int dgtta_dice_ce_ds_fwd(const float *logits, int ldc, const int64_t *labels_full, float *loss3, float *dice, void *ws,
                         size_t ws_bytes, int B, int C, int d, int h, int w, int sd, int sh, int sw, float smooth, int do_bg,
                         void *stream);
int dgtta_dice_ce_ds_bwd(const float *logits, int ldc, const int64_t *labels_full, const void *ws, float grad_scale,
                         const float *grad_scale_dev, float *grad_logits, int ldg, int B, int C, int d, int h, int w, int sd,
                         int sh, int sw, void *stream);
/* The forward functions above with the plans' `batch_dice` switch.  batch_dice = 0: dgtta_dice_ce_fwd / dgtta_dice_ce_ds_fwd bit
 * for bit.  batch_dice = 1 - nnU-Net's MemoryEfficientSoftDiceLoss(batch_dice=True) inside DC_and_CE_loss [3P nnunetv2==2.2.1, not
 * available here], restated from memory, UNPINNED - pools the three sums over the batch before the ratio:
 *   dice_c = (2 sum_b sum_v p y + smooth) / max(sum_b sum_v p + sum_b sum_v y + smooth, 1e-8);  loss3[2] = -mean_{c >= first} dice_c
 * loss3[1] (cross-entropy) is unchanged; every row of dice[B][C] holds dice_c.  The per-sample sums are formed in the order of the
 * per-sample mode and added over b in ascending order in double, without atomics: bit-reproducible.  Same workspace (size and
 * layout) as above; the matching backward is dgtta_dice_ce_bwd / dgtta_dice_ce_ds_bwd, unchanged.  Any other batch_dice:
 * DGTTA_ERR_BADARG. */
int dgtta_dice_ce_batch_fwd(const float *logits, int ldc, const int64_t *labels, float *loss3, float *dice, void *ws,
                            size_t ws_bytes, int B, int C, int64_t V, float smooth, int do_bg, int batch_dice, void *stream);
int dgtta_dice_ce_ds_batch_fwd(const float *logits, int ldc, const int64_t *labels_full, float *loss3, float *dice, void *ws,
                               size_t ws_bytes, int B, int C, int d, int h, int w, int sd, int sh, int sw, float smooth,
                               int do_bg, int batch_dice, void *stream);

/* REGION-BASED datasets - nnU-Net's second label model: a dataset.json whose label values are lists describes R overlapping
 * regions of the label map, the network has R sigmoid outputs and no background channel.  Everything below is restated from
 * memory of nnunetv2 2.2.1 [3P, not available here]: UNPINNED.
 *   table      uint32 [L], L = largest label value + 1 <= 1024: bit r of table[y] is set when label y belongs to region r
 *              (R <= 32); t[b][v][r] = bit r of table[labels[b][v]].  A voxel is VALID when 0 <= label < L; any other voxel is
 *              left out of every sum and receives a zero gradient.  No region target tensor is ever built.
 * Loss: DC_and_BCE_loss with MemoryEfficientSoftDiceLoss(do_bg=True, smooth), weights 1 / 1.  s = sigmoid(logits):
 *   loss3[1] = (1 / (N R)) sum_{valid v, r} [max(z, 0) - t z + log1p(exp(-|z|))]      N = valid voxels of the batch (no valid
 *              voxel: 0, and a zero gradient)
 *   dice[b][r] = (2 sum_v s t + smooth) / max(sum_v s + sum_v t + smooth, 1e-8);  loss3[2] = -mean_{b, r} dice
 *   loss3[0] = loss3[1] + loss3[2]
 * logits / grad_logits voxel-major fp32 [B][V][ld], labels int64 [B][V]; the _ds_ forms take logits [B][d][h][w][ld] and the
 * FULL-resolution label map [B][d sd][h sh][w sw], read at (i sd + sd / 2, j sh + sh / 2, k sw + sw / 2) as dgtta_dice_ce_ds_*
 * do (strides (1, 1, 1): the dense entries bit for bit).  The _batch_ forms take the plans' batch_dice (0: the plain entries bit
 * for bit; 1: the three Dice sums are pooled over b before the ratio, loss3[1] unchanged, every row of dice holds the region's
 * one value; anything else DGTTA_ERR_BADARG).  bwd: grad_logits = grad_scale * (*grad_scale_dev if given) * d loss3[0] /
 * d logits.  ws: dgtta_region_loss_ws_bytes(B, R, V), kept between fwd and bwd.  1 <= B <= 8, 1 <= R <= 32.  Double partial sums
 * in fixed slots, one finalize workgroup, no floating-point atomics: bit-reproducible. */
size_t dgtta_region_loss_ws_bytes(int B, int R, int64_t V);
int dgtta_region_loss_fwd(const float *logits, int ldc, const int64_t *labels, const uint32_t *table, int L, float *loss3,
                          float *dice, void *ws, size_t ws_bytes, int B, int R, int64_t V, float smooth, void *stream);
int dgtta_region_loss_batch_fwd(const float *logits, int ldc, const int64_t *labels, const uint32_t *table, int L, float *loss3,
                                float *dice, void *ws, size_t ws_bytes, int B, int R, int64_t V, float smooth, int batch_dice,
                                void *stream);
int dgtta_region_loss_bwd(const float *logits, int ldc, const int64_t *labels, const uint32_t *table, int L, const void *ws,
                          float grad_scale, const float *grad_scale_dev, float *grad_logits, int ldg, int B, int R, int64_t V,
                          void *stream);
size_t dgtta_region_loss_ds_ws_bytes(int B, int R, int d, int h, int w);
int dgtta_region_loss_ds_fwd(const float *logits, int ldc, const int64_t *labels_full, const uint32_t *table, int L, float *loss3,
                             float *dice, void *ws, size_t ws_bytes, int B, int R, int d, int h, int w, int sd, int sh, int sw,
                             float smooth, void *stream);
int dgtta_region_loss_ds_batch_fwd(const float *logits, int ldc, const int64_t *labels_full, const uint32_t *table, int L,
                                   float *loss3, float *dice, void *ws, size_t ws_bytes, int B, int R, int d, int h, int w, int sd,
                                   int sh, int sw, float smooth, int batch_dice, void *stream);
int dgtta_region_loss_ds_bwd(const float *logits, int ldc, const int64_t *labels_full, const uint32_t *table, int L,
                             const void *ws, float grad_scale, const float *grad_scale_dev, float *grad_logits, int ldg, int B,
                             int R, int d, int h, int w, int sd, int sh, int sw, void *stream);
/* Online pseudo-Dice of a region head: counts int64 [3][R] = TP, FP, FN per region of the prediction logits > 0 (sigmoid > 0.5;
 * a logit of exactly 0 is "not predicted") over the valid voxels of logits fp32 [rows][ldc] / labels int64 [rows].  counts is
 * cleared by the call.  Integer sums only. */
int dgtta_region_counts(const float *logits, int ldc, int R, const int64_t *labels, const uint32_t *table, int L,
                        int64_t *counts, int64_t rows, void *stream);
/* Label map of region logits - convert_probabilities_to_segmentation: label = 0; for i = 0 .. R-1 in order: label = order[i]
 * where the ensemble-mean logit of output i is > 0 (the last positive region in the order wins; exactly 0 is not in the region).
 * The mean is a positive multiple of the accumulated sum, so the accumulator's sign decides.  h_order: HOST array of R positive
 * labels (regions_class_order; anything else DGTTA_ERR_BADARG), label_out int64.
 * dgtta_logits_regions: the logits-space window accumulator acc [rows][R], fp32 or fp16 (acc_dtype).
 * dgtta_feature_head_regions: the feature-space accumulators, arguments as dgtta_feature_head_argmax; accumulator i is
 *   sum_m w[m][i] . facc[m][v] + nsum[v] bsum[i], formed in that function's order on the matrix cores.  R <= 32 and a weight
 *   image of M members that fits the LDS (M <= 35), else DGTTA_ERR_UNSUPPORTED. */
int dgtta_logits_regions(const void *acc, int acc_dtype, int R, int64_t rows, const int *h_order, int64_t *label_out, void *stream);
int dgtta_feature_head_regions(const float *facc, int64_t member_stride, const float *nsum, const float *w, const float *bsum, int M,
                               int Cin, int R, int64_t V, const int *h_order, int64_t *label_out, void *stream);

/* ---------------------------------------------------------------------------------------------
 * AdamW (decoupled weight decay, bias-corrected, no amsgrad) over a list of tensors.  Replaces
 * torch.optim.AdamW(model.parameters(), lr).step() at dg_tta/tta/tta.py:185,278 (betas 0.9/0.999,
 * eps 1e-8, weight_decay 0.01 = PyTorch defaults).  h_* are HOST arrays of ntensors device
 * pointers / element counts; tensors whose h_g[i] is NULL are skipped (grad None in PyTorch).
 * step is the 1-based step count of those tensors.  grad_scale: the static loss scale the gradients carry (fp16
 * storage path: the caller multiplied the loss gradient by it); every gradient is divided by it on load. 1 = none.
 * ------------------------------------------------------------------------------------------- */
int dgtta_adamw_step(float *const *h_p, const float *const *h_g, float *const *h_m, float *const *h_v,
                     const int64_t *h_n, int ntensors, float lr, float beta1, float beta2, float eps,
                     float weight_decay, int step, float grad_scale, const int *skip_if_nonzero, void *stream);
/* Overflow guard of the fp16 storage path (the role torch.cuda.amp.GradScaler's inf check plays for autocast users; the
 * reference itself runs fp32, dg_tta/tta/tta.py:275-279): *flag (device int, zeroed by the caller) becomes 1 when any
 * gradient element is inf / NaN.  dgtta_adamw_step(skip_if_nonzero = flag) then leaves parameters and state untouched;
 * skip_if_nonzero may be NULL. */
int dgtta_grads_nonfinite(const float *const *h_g, const int64_t *h_n, int ntensors, int *flag, void *stream);

/* ---------------------------------------------------------------------------------------------
 * nnU-Net's optimiser step [3P nnunetv2==2.2.1 nnUNetTrainer, from memory: UNPINNED], the one `nnUNetv2_train` runs for
 * the reference's trainers (dg_tta/run.py pretrain): torch.nn.utils.clip_grad_norm_(parameters, 12) followed by
 * torch.optim.SGD(lr, weight_decay=3e-5, momentum=0.99, nesterov=True), dampening 0.  h_* are HOST arrays as above; tensors
 * whose h_g[i] is NULL are skipped and do not enter the norm.
 * dgtta_grad_sumsq: *out (device fp32) = sum over all gradient elements of g*g, of the gradients AS STORED (loss scale
 * included).  Bit-reproducible from run to run: per-workgroup partials (double) in ws, added in a fixed order; no floating-
 * point atomics.  ws: dgtta_grad_sumsq_ws_bytes(sum of the element counts, ntensors) bytes, 8-byte aligned.
 * dgtta_sgd_step, per element (no operation fused):
 *   norm = sqrt(*sumsq) / grad_scale;  coef = min(1, max_norm / (norm + 1e-6))      (coef = 1 when sumsq is NULL)
 *   g' = (g / grad_scale) * coef;  d = g' + weight_decay * p;  buf = first_step ? d : momentum * buf + d
 *   p -= lr * (nesterov ? d + momentum * buf : buf)
 * first_step != 0: the momentum buffers are written, never read (torch creates them as a copy of d on a parameter's first
 * step).  sumsq is read on the device.  skip_if_nonzero as in dgtta_adamw_step: p and buf stay untouched. */
size_t dgtta_grad_sumsq_ws_bytes(int64_t total_elements, int ntensors);
int dgtta_grad_sumsq(const float *const *h_g, const int64_t *h_n, int ntensors, float *out, void *ws, size_t ws_bytes,
                     void *stream);
int dgtta_sgd_step(float *const *h_p, const float *const *h_g, float *const *h_buf, const int64_t *h_n, int ntensors,
                   float lr, float momentum, float weight_decay, int nesterov, int first_step, float grad_scale,
                   const float *sumsq, float max_norm, const int *skip_if_nonzero, void *stream);

/* ---------------------------------------------------------------------------------------------
 * nnUNet PlainConvUNet building blocks (third-party dynamic-network-architectures==0.2, built at
 * dg_tta/pretraining/nnUNetTrainer_GIN_MIND.py:46-53 from plans.json:279-401): Conv3d 3x3x3 (pad 1,
 * stride 1|2, bias) -> InstanceNorm3d(eps, affine) -> LeakyReLU(0.01); ConvTranspose3d k2 s2;
 * 1x1x1 segmentation head.  Activations are NDHWC with explicit row lengths (ld*), so that
 * torch.cat((up, skip), 1) is realised by writing into channel slices of one buffer.
 * Weights: w_t = torch layout [Cout][Cin][3][3][3] fp32 (read-only); the kernels use packed copies
 * produced by dgtta_conv3d_pack_weights.
 * ------------------------------------------------------------------------------------------- */

/* packs torch [Cout][Cin][27] fp32 into one blob `wpack` of 2*27*CinP*CoutP elements (dtype fp32|bf16, zero padded):
 *   wf [27][CinP][CoutP] = w[co][ci][tap]        (first half)
 *   wb [27][CoutP][CinP] = w[co][ci][26-tap]     (second half: taps mirrored, channel roles swapped)
 * forward, data-gradient and MFMA kernels pick the orientation they need from the blob. */
size_t dgtta_conv3d_packed_bytes(int CinP, int CoutP, int dtype);
int dgtta_conv3d_pack_weights(const float *w_t, void *wpack, int Cin, int Cout, int CinP, int CoutP, int dtype,
                              void *stream);

/* y[b][vo][co] = bias[co] + sum_{tap,ci} x[b][s*vo+tap-1][ci] * w[co][ci][tap]      (zero padding)
 * Optionally accumulates per-(b,co) partial sums of y and y^2 for the following InstanceNorm
 * (stats != NULL: dgtta_conv3d_stats_bytes).  impl: 0 = auto, 1 = reference-grade VALU kernel,
 * 2 = MFMA implicit GEMM. */
size_t dgtta_conv3d_stats_bytes(int B, int Cout, int Do, int Ho, int Wo);
int dgtta_conv3d_k3_fwd(const void *x, int ldx, const void *wpack, const float *bias, void *y, int ldy, void *stats,
                        int B, int Cin, int Cout, int CinP, int CoutP, int Di, int Hi, int Wi, int stride,
                        int dtype, int impl, void *stream);
/* dx[b][vi][ci] = sum_{tap,co} dy[b][(vi+1-tap)/s][co] * w[co][ci][tap]   (terms with non-integer
 * or out-of-range index dropped).  accumulate != 0: dx += (skip-connection gradient sum). */
int dgtta_conv3d_k3_dgrad(const void *dy, int lddy, const void *wpack, void *dx, int lddx, int B, int Cin, int Cout,
                          int CinP, int CoutP, int Di, int Hi, int Wi, int stride, int accumulate, int dtype,
                          int impl, void *stream);
/* dw_t[co][ci][tap] (+)= sum_{b,vo} x[b][s*vo+tap-1][ci] * dy[b][vo][co];  db[co] (+)= sum dy.
 * fp32 outputs in torch layout; accumulate != 0 adds to existing gradients (gradient accumulation
 * over tta.py:221's 16 steps and over both branches). */
size_t dgtta_conv3d_wgrad_ws_bytes(int B, int Cin, int Cout, int Do, int Ho, int Wo);
/* Optional larger workspace for dtype = DGTTA_F32 (stride 1, or 2 with even extents): the plain workspace followed by room for
 * three bf16 planes of x (input extent) and three of dy.  Given that much, dgtta_conv3d_k3_wgrad evaluates the fp32 weight gradient as six launches of the 16-bit
 * matrix-core kernels on the exact three-term bf16 splits of its operands (x = x0 + x1 + x2; the six products with i + j <= 2,
 * each exact in the fp32 accumulator) instead of the fp32 MFMA kernel: same result to fp32 rounding, ~1.7x the rate. */
size_t dgtta_conv3d_wgrad_split_ws_bytes(int B, int Cin, int Cout, int Do, int Ho, int Wo, int stride);
int dgtta_conv3d_k3_wgrad(const void *x, int ldx, const void *dy, int lddy, float *dw_t, float *db, void *ws,
                          size_t ws_bytes, int B, int Cin, int Cout, int Di, int Hi, int Wi, int stride,
                          int accumulate, int dtype, int impl, void *stream);
/* Round 6: x as 32-channel BLOCKS.  Block c of the input channels is a dense tensor [B][D][H][W][32] at element offset
 * c * x_block_stride from x (the level-0 concat buffer of the U-Net as planes [up | skip]: the kernels that read ONE half - the
 * stride-2 conv of the skip, the transposed conv's backward - then use whole 128-byte lines).  Stride 1, 64 input channels, 16-bit
 * storage, and only where the D-ring kernels take the launch: dgtta_conv3d_k3_blocked_supported returns 1 exactly when BOTH calls below
 * accept these dimensions; otherwise they return DGTTA_ERR_UNSUPPORTED and launch nothing.  Results equal the interleaved
 * layout's bit for bit (same kernels, same order). */
int dgtta_conv3d_k3_blocked_supported(int B, int Cin, int Cout, int D, int H, int W, int dtype);
int dgtta_conv3d_k3_fwd_blocked(const void *x, long long x_block_stride, const void *wpack, const float *bias, void *y, int ldy,
                                void *stats, int B, int Cin, int Cout, int CinP, int CoutP, int Di, int Hi, int Wi, int dtype,
                                void *stream);
int dgtta_conv3d_k3_wgrad_blocked(const void *x, long long x_block_stride, const void *dy, int lddy, float *dw_t, float *db,
                                  void *ws, size_t ws_bytes, int B, int Cin, int Cout, int Di, int Hi, int Wi, int accumulate,
                                  int dtype, void *stream);

/* InstanceNorm3d(eps, affine, biased variance) + LeakyReLU(slope), per (b,c) over the volume.
 * fwd: stats = partial sums from the conv epilogue, or NULL (then computed here from y).
 *      writes mean_rstd[B][C][2] (saved for backward) and z = lrelu(gamma*(y-mean)*rstd + beta). */
size_t dgtta_instnorm_ws_bytes(int B, int C, int64_t V);
int dgtta_instnorm_lrelu_fwd(const void *y, int ldy, const void *stats, const float *gamma, const float *beta,
                             float *mean_rstd, void *z, int ldz, void *ws, size_t ws_bytes, int B, int C,
                             int64_t V, float eps, float slope, int dtype, void *stream);
/* bwd: given gz = dL/dz and saved y, mean_rstd: writes dy (may alias gz), and dgamma/dbeta (+)=. */
int dgtta_instnorm_lrelu_bwd(const void *gz, int ldgz, const void *y, int ldy, const float *gamma,
                             const float *beta, const float *mean_rstd, void *dy, int lddy, float *dgamma,
                             float *dbeta, void *ws, size_t ws_bytes, int B, int C, int64_t V, float slope,
                             int accumulate, int dtype, void *stream);

/* Data gradient of a stride-1 conv whose INPUT was z = LeakyReLU(InstanceNorm(y_prev)) (the blocks built at
 * dg_tta/pretraining/nnUNetTrainer_GIN_MIND.py:46-53; autograd of tta.py:275), fused with the reduction pass of that
 * previous layer's InstanceNorm backward: besides dx = gz it leaves, in `gstats` (size dgtta_conv3d_stats_bytes(B, Cin,
 * Di, Hi, Wi)), the per-tile sums of g' and g' * y_prev (g' = gz * lrelu'(pre-activation)).  *h_produced (HOST int) = 1 when
 * the statistics were produced (16-bit storage on the row-reuse kernel, whole tiles); 0: plain dgtta_conv3d_k3_dgrad ran.
 * dgtta_instnorm_lrelu_bwd_gstats = dgtta_instnorm_lrelu_bwd without its own pass over y and gz. */
int dgtta_conv3d_k3_dgrad_gstats(const void *dy, int lddy, const void *wpack, void *dx, int lddx, int B, int Cin, int Cout,
                                 int CinP, int CoutP, int Di, int Hi, int Wi, const void *y_prev, int ldy_prev,
                                 const float *mean_rstd_prev, const float *gamma_prev, const float *beta_prev, float slope,
                                 void *gstats, size_t gstats_bytes, int *h_produced, int dtype, int impl, void *stream);
int dgtta_instnorm_lrelu_bwd_gstats(const void *gz, int ldgz, const void *y, int ldy, const float *gamma, const float *beta,
                                    const float *mean_rstd, void *dy, int lddy, float *dgamma, float *dbeta,
                                    const void *gstats, void *ws, size_t ws_bytes, int B, int C, int64_t V, float slope,
                                    int accumulate, int dtype, void *stream);
/* dgtta_instnorm_lrelu_bwd of the block in front of the segmentation head, with gz given as its factors: d16 [B][V][nsel] (dtype),
 * what dgtta_seghead_warp_bwd_g16_d16 left, and the head's fp32 weight w [classes][C] with the selected rows sel (NULL: rows
 * 0..nsel-1).  gz[c] = sum_k w[sel[k]][c] * float(d16[k]) is rebuilt in fp32 in both passes and used unrounded; it is never stored.
 * C = 32, nsel = 16, bf16 / fp16 only (else DGTTA_ERR_UNSUPPORTED and nothing is launched); ws as dgtta_instnorm_lrelu_bwd. */
int dgtta_instnorm_lrelu_bwd_head(const void *d16, const float *w, const int *sel, int nsel, const void *y, int ldy,
                                  const float *gamma, const float *beta, const float *mean_rstd, void *dy, int lddy,
                                  float *dgamma, float *dbeta, void *ws, size_t ws_bytes, int B, int C, int64_t V, float slope,
                                  int accumulate, int dtype, void *stream);

/* ConvTranspose3d(Cin, Cout, kernel 2, stride 2, bias): w_t torch layout [Cin][Cout][2][2][2] fp32.
 * out[b][2v+o][co] = bias[co] + sum_ci x[b][v][ci] * w[ci][co][o]. */
size_t dgtta_convT3d_fwd_ws_bytes(int Cin, int Cout, int dtype);
int dgtta_convT3d_k2s2_fwd(const void *x, int ldx, const float *w_t, const float *bias, void *out, int ldo, void *ws,
                           size_t ws_bytes, int B, int Cin, int Cout, int Di, int Hi, int Wi, int dtype, int impl,
                           void *stream);
size_t dgtta_convT3d_bwd_ws_bytes(int B, int Cin, int Cout, int Di, int Hi, int Wi);
/* (round 5) the same with room for the fp32 weight gradient as six launches of the 16-bit matrix-core kernel on the exact three-term
 * bf16 splits of x and dout (see dgtta_conv3d_wgrad_split_ws_bytes): offered this workspace, dgtta_convT3d_k2s2_bwd takes that path in
 * fp32 storage; with the plain one it runs the fp32 MFMA kernel as before. */
size_t dgtta_convT3d_bwd_split_ws_bytes(int B, int Cin, int Cout, int Di, int Hi, int Wi);
int dgtta_convT3d_k2s2_bwd(const void *x, int ldx, const void *dout, int lddo, const float *w_t, void *dx, int lddx,
                           float *dw_t, float *db, void *ws, size_t ws_bytes, int B, int Cin, int Cout, int Di,
                           int Hi, int Wi, int accumulate, int dtype, int impl, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Anisotropic PlainConvUNet layers: what nnU-Net 2.2.1's planner writes for data whose slice spacing is much coarser than
 * its in-plane spacing (conv_kernel_sizes [kd, 3, 3], pool_op_kernel_sizes with 1 or 2 per axis).  Same conventions as the
 * k3 family above; a layer with a 3x3x3 kernel and an isotropic stride keeps using the k3 entry points.
 * Conv3d(Cin, Cout, kernel (kd, 3, 3), stride (sd, sh, sw), padding (kd / 2, 1, 1), bias) with kd in {1, 3} and strides in
 * {1, 2}; output extent (i + 2 * pad - k) / s + 1 per axis.  Anything else returns DGTTA_ERR_UNSUPPORTED.  x / dy operands:
 * 16-byte aligned rows (ld a multiple of 16 bytes).  Data and weight gradients of a strided axis need an even input extent.
 * ------------------------------------------------------------------------------------------- */
/* packs torch [Cout][Cin][kd][kh][kw] fp32 (kh = kw = 3) into one blob of dgtta_conv3d_kpacked_bytes: the matrix-core images of
 * the forward (N = Cout, K = Cin) and of the data-gradient (N = Cin, K = Cout) orientation, kd * 9 taps each; CinP / CoutP =
 * the channel counts zero padded to multiples of 8 (fp32) or 16 (16-bit). */
size_t dgtta_conv3d_kpacked_bytes(int kd, int CinP, int CoutP, int dtype);
int dgtta_conv3d_kpack_weights(const float *w_t, void *wpack, int kd, int kh, int kw, int Cin, int Cout, int CinP, int CoutP,
                               int dtype, void *stream);
/* y[b][vo][co] = bias[co] + sum_{tap,ci} x[b][s*vo + tap - pad][ci] * w[co][ci][tap]   (per axis, zero padding).
 * stats != NULL: the InstanceNorm partial sums as dgtta_conv3d_k3_fwd leaves them (dgtta_conv3d_stats_bytes of the output);
 * NULL: dgtta_instnorm_lrelu_fwd computes them from y. */
int dgtta_conv3d_fwd(const void *x, int ldx, const void *wpack, const float *bias, void *y, int ldy, void *stats, int B, int Cin,
                     int Cout, int CinP, int CoutP, int Di, int Hi, int Wi, int kd, int sd, int sh, int sw, int dtype, void *stream);
/* dx[b][vi][ci] = sum_{tap,co} dy[b][vo][co] * w[co][ci][tap] over s*vo + tap - pad = vi;  accumulate != 0: dx += (the
 * skip-connection gradient sum).  Di, Hi, Wi: input extent. */
int dgtta_conv3d_dgrad(const void *dy, int lddy, const void *wpack, void *dx, int lddx, int B, int Cin, int Cout, int CinP, int CoutP,
                       int Di, int Hi, int Wi, int kd, int sd, int sh, int sw, int accumulate, int dtype, void *stream);
/* dw_t[co][ci][tap] (+)= sum_{b,vo} x[b][s*vo + tap - pad][ci] * dy[b][vo][co];  db[co] (+)= sum dy (db may be NULL).
 * fp32 torch layout, fixed summation order (deterministic); accumulate != 0 adds to the existing gradients.
 * Di, Hi, Wi: INPUT extent (also for the workspace query). */
size_t dgtta_conv3d_kwgrad_ws_bytes(int B, int Cin, int Cout, int Di, int Hi, int Wi, int kd, int sd, int sh, int sw);
int dgtta_conv3d_wgrad(const void *x, int ldx, const void *dy, int lddy, float *dw_t, float *db, void *ws, size_t ws_bytes, int B,
                       int Cin, int Cout, int Di, int Hi, int Wi, int kd, int sd, int sh, int sw, int accumulate, int dtype,
                       void *stream);
/* ConvTranspose3d(Cin, Cout, kernel = stride = (sd, sh, sw) in {1, 2}^3, not all 1, bias): w_t torch layout
 * [Cin][Cout][sd][sh][sw] fp32.  out[b][s*v + o][co] = bias[co] + sum_ci x[b][v][ci] * w[ci][co][o].
 * bwd: dx (overwritten; NULL: skipped), dw_t / db (+)= as for the k2s2 form (NULL: skipped). */
size_t dgtta_convT3d_s_fwd_ws_bytes(int Cin, int Cout, int sd, int sh, int sw, int dtype);
int dgtta_convT3d_s_fwd(const void *x, int ldx, const float *w_t, const float *bias, void *out, int ldo, void *ws, size_t ws_bytes,
                        int B, int Cin, int Cout, int Di, int Hi, int Wi, int sd, int sh, int sw, int dtype, void *stream);
size_t dgtta_convT3d_s_bwd_ws_bytes(int B, int Cin, int Cout, int Di, int Hi, int Wi, int sd, int sh, int sw);
int dgtta_convT3d_s_bwd(const void *x, int ldx, const void *dout, int lddo, const float *w_t, void *dx, int lddx, float *dw_t,
                        float *db, void *ws, size_t ws_bytes, int B, int Cin, int Cout, int Di, int Hi, int Wi, int sd, int sh,
                        int sw, int accumulate, int dtype, void *stream);

/* 1x1x1 head fused with map_label(input_format="logits") (torch_utils.py:214-221): only the rows
 * sel[0..nsel) of the [Ccls][Cin] weight are evaluated (sel == NULL: all Ccls rows).
 * out fp32: NDHWC [B][V][ldo] (out_ndhwc=1) or NCDHW [B][nsel][V]. */
int dgtta_seghead_fwd(const void *x, int ldx, const float *w, const float *bias, const int *sel, int nsel,
                      float *out, int out_ndhwc, int ldo, int B, int Cin, int64_t V, int dtype, void *stream);
/* dx = dout . W_sel ; dw_sel[nsel][Cin], db_sel[nsel] (+)= (fp32, compact rows; caller scatters). */
size_t dgtta_seghead_bwd_ws_bytes(int B, int Cin, int nsel, int64_t V);
int dgtta_seghead_bwd(const void *x, int ldx, const float *dout, int lddo, const float *w, const int *sel,
                      int nsel, void *dx, int lddx, float *dw_sel, float *db_sel, void *ws, size_t ws_bytes,
                      int B, int Cin, int64_t V, int accumulate, int dtype, void *stream);
/* + accumulate_dx: dx += dout . W_sel instead of dx = (an auxiliary head of deep supervision adds to the gradient rows that the
 * next transposed conv's backward wrote; no temporary, no add pass).  Same workspace.  Heads with Cin a multiple of 32
 * (32..320; 64.. without accumulate_dx), nsel <= 128 and 16-bit storage run on the matrix cores (csrc/seghead_mfma.hip), as
 * does dgtta_seghead_fwd for them; every other shape runs the general kernels. */
int dgtta_seghead_bwd_acc(const void *x, int ldx, const float *dout, int lddo, const float *w, const int *sel,
                          int nsel, void *dx, int lddx, float *dw_sel, float *db_sel, void *ws, size_t ws_bytes,
                          int B, int Cin, int64_t V, int accumulate, int accumulate_dx, int dtype, void *stream);

/* Segmentation head fused with the inverse warp of its logits: the two steps at the end of calc_branch
 * (dg_tta/tta/tta.py:560-575: model() -> map_label(logits) -> grid_sample(..., R_inverse grid, zeros padding)) in one launch
 * each way.  Both are linear and the head is per voxel, so warp(head(z)) = head(warp(z)) + bias * (in-bounds corner weight):
 * the un-warped logits and their gradient are never materialised.  z: NDHWC [B][D][H][W][32] in `dtype` (bf16 / fp16 only);
 * w / bias: the head's fp32 parameters, sel: the nsel (4, 8, 12 or 16) selected class rows; theta [B][3][4] = R_inverse.
 * fwd: out [B][D][H][W][nsel] fp32 = the branch's logits in the common frame.
 * bwd: gout = gradient of that tensor; gz [B][D][H][W][32] (dtype) = gradient of z; dw_sel [nsel][32], db_sel [nsel] fp32
 * (either may be NULL; accumulate != 0 adds).  h_theta: HOST copy of theta - the owner-computes gather has no scatter
 * fallback here, so maps it would decline (singular / strongly minifying) are rejected with DGTTA_ERR_UNSUPPORTED before
 * anything is launched and the caller uses dgtta_seghead_* + dgtta_affine_warp3d_*.  ws: dgtta_seghead_warp_bwd_ws_bytes
 * (0 = shape not offered: B*D*H*W must be a multiple of 128). */
/* 1 when the fused pair applies to this shape / dtype and to every map of the HOST array h_theta [B][3][4], else 0.  The
 * weight gradient of the fused backward needs nsel = 8 or 16: with 4 or 12 selected classes this returns 0 and
 * dgtta_seghead_warp_bwd refuses dw_sel != NULL with DGTTA_ERR_UNSUPPORTED before anything is launched (gz and db_sel alone
 * are computed). */
int dgtta_seghead_warp_supported(const float *h_theta, int B, int Cin, int nsel, int D, int H, int W, int dtype);
size_t dgtta_seghead_warp_bwd_ws_bytes(int B, int Cin, int nsel, int D, int H, int W);
int dgtta_seghead_warp_fwd(const void *z, const float *w, const float *bias, const int *sel, int nsel, const float *theta,
                           float *out, int B, int Cin, int D, int H, int W, int tta_grid_algebra, int dtype, void *stream);
int dgtta_seghead_warp_bwd(const void *z, const float *gout, const float *theta, const float *h_theta, const float *w,
                           const int *sel, int nsel, void *gz, float *dw_sel, float *db_sel, void *ws, size_t ws_bytes, int B,
                           int Cin, int D, int H, int W, int tta_grid_algebra, int accumulate, int dtype, void *stream);
/* The same with gout16 = the gradient of the warped logits in the network's 16-bit storage type `dtype`, rows of nsel values as
 * dgtta_softdice_bwd_t writes them (round 6): the gather reads half the bytes per candidate; acc += float(g16) * weight in the
 * same order, so the result equals dgtta_seghead_warp_bwd on the widened values bit for bit. */
int dgtta_seghead_warp_bwd_g16(const void *z, const void *gout16, const float *theta, const float *h_theta, const float *w,
                               const int *sel, int nsel, void *gz, float *dw_sel, float *db_sel, void *ws, size_t ws_bytes, int B,
                               int Cin, int D, int H, int W, int tta_grid_algebra, int accumulate, int dtype, void *stream);
/* dgtta_seghead_warp_bwd_g16 without the data gradient: d16_out [B][D][H][W][nsel] (dtype, 16-byte aligned, caller-owned) receives
 * the gathered logit gradient, each value rounded once - the operand the weight gradient reads; dw_sel / db_sel are bit for bit
 * those of dgtta_seghead_warp_bwd_g16.  gz = W^T d16 is left to dgtta_instnorm_lrelu_bwd_head, which never stores it. */
int dgtta_seghead_warp_bwd_g16_d16(const void *z, const void *gout16, const float *theta, const float *h_theta, int nsel,
                                   void *d16_out, float *dw_sel, float *db_sel, void *ws, size_t ws_bytes, int B, int Cin, int D,
                                   int H, int W, int tta_grid_algebra, int accumulate, int dtype, void *stream);

/* Layout / dtype converters between the reference's NCDHW fp32 and internal NDHWC. */
int dgtta_ncdhw_to_ndhwc(const float *src, void *dst, int B, int C, int64_t V, int ldc, int dtype, void *stream);
int dgtta_ndhwc_to_ncdhw(const void *src, float *dst, int B, int C, int64_t V, int ldc, int dtype, void *stream);

/* argmax over channels + per-label hard Dice counts; replaces tta.py:321 + dice_coeff
 * (torch_utils.py:107-117).  logits NDHWC fp32 (or NULL: predictions are read from argmax_out);
 * labels int64 [B][V] or NULL; argmax_out int64 [B][V]; counts[3*C] int64 (|pred==l|, |gt==l|,
 * |both|), zeroed by the caller. */
int dgtta_argmax_dice(const float *logits, int ldc, int C, const int64_t *labels, int64_t *argmax_out,
                      int64_t *counts, int B, int64_t V, void *stream);

/* Gaussian-weighted sliding-window accumulation for the post-TTA ensemble inference (nnU-Net's
 * predict_sliding_window_return_logits, reached from dg_tta/tta/nnunet_utils.py:116-125,208-230):
 * acc[(x0..,y0..,z0..)][c] += patch[p][c]*gauss[p]; nsum[..] += gauss[p] (nsum may be NULL).
 * patch [PD][PH][PW][C], acc [X][Y][Z][C], nsum [X][Y][Z], all fp32 voxel-major. */
int dgtta_window_accumulate(const float *patch, const float *gauss, float *acc, float *nsum, int C, int PD, int PH,
                            int PW, int X, int Y, int Z, int x0, int y0, int z0, void *stream);

/* The same with the 1x1x1 segmentation head in front of it: acc += gauss * (W z + bias) for ALL C classes of one window,
 * from the window's feature map z [PD][PH][PW][32] (16-bit storage) - the window's logits (880 MB at 128^3 x 105) are never
 * written.  Logits are evaluated as dgtta_seghead_fwd does (identical values). */
int dgtta_seghead_window_accumulate(const void *z, const float *w, const float *bias, const float *gauss, float *acc,
                                    float *nsum, int Cin, int C, int PD, int PH, int PW, int X, int Y, int Z, int x0, int y0,
                                    int z0, int dtype, void *stream);

/* The accumulator's storage type as a parameter (round 4): acc_dtype DGTTA_F32 or DGTTA_F16.  nnU-Net's predictor keeps
 * `predicted_logits` in torch.half (nnunetv2==2.2.1 predict_sliding_window_return_logits); with DGTTA_F16 the sum is formed
 * in fp32 and rounded to half once per window and voxel - half the HBM traffic of the read-modify-write and half the 52.5 GiB
 * of a 105-class 512^3 volume.  nsum stays fp32.  The functions above are these with DGTTA_F32. */
int dgtta_window_accumulate_t(const float *patch, const float *gauss, void *acc, float *nsum, int C, int PD, int PH, int PW,
                              int X, int Y, int Z, int x0, int y0, int z0, int acc_dtype, void *stream);
int dgtta_seghead_window_accumulate_t(const void *z, const float *w, const float *bias, const float *gauss, void *acc,
                                      float *nsum, int Cin, int C, int PD, int PH, int PW, int X, int Y, int Z, int x0, int y0,
                                      int z0, int dtype, int acc_dtype, void *stream);
/* argmax over the C <= 112 classes of `rows` voxel-major rows stored back to back (fp32 or fp16): the label map of the
 * window accumulator (nnU-Net's convert_predicted_logits_to_segmentation..., argmax over ALL pretrain classes,
 * dg_tta/tta/tta.py:404-413).  First maximum wins (dgtta_argmax_dice routes here when it can). */
int dgtta_argmax_rows(const void *logits, int acc_dtype, int C, int64_t rows, int64_t *argmax_out, void *stream);

/* One-axis spline resampling (order 0 / 1 / 3) with the coordinate rule and boundary handling of
 * skimage.transform.resize(mode='edge', anti_aliasing=False) = scipy.ndimage.zoom(mode='nearest', grid_mode=True), which is
 * what nnU-Net's DefaultPreprocessor resamples with (third-party nnunetv2==2.2.1, reached from preprocess_fromfile,
 * dg_tta/tta/nnunet_utils.py:170-204).  src: double [outer][n][inner], dst: double [outer][m][inner]; applied per axis
 * by the caller (the nD operation is separable).  ws: dgtta_resample_axis_ws_bytes (order 3 only). */
size_t dgtta_resample_axis_ws_bytes(int64_t outer, int n, int64_t inner, int order);
int dgtta_resample_axis(const double *src, double *dst, void *ws, size_t ws_bytes, int64_t outer, int n, int m,
                        int64_t inner, int order, void *stream);

/* Export of a prediction in the case's ORIGINAL geometry: nnU-Net's convert_predicted_logits_to_segmentation_with_correct_shape
 * (third-party nnunetv2==2.2.1), which the reference reaches through predict_from_data_iterator
 * (dg_tta/tta/nnunet_utils.py:208-230) before sitk_io.write_seg (dg_tta/tta/tta.py:404-413).
 * dgtta_logits_chunk_f64: dst[x][y][z][j] = acc[x0+x][y0+y][z0+z][c0+j] / nsum[..] as double (classes c0..c0+cg-1 of the
 * window accumulator, cropped back from the padding to the patch size), the input of the dgtta_resample_axis passes.
 * dgtta_argmax_merge_f64: running argmax over class groups: vals double [V][cg] holds classes c0..; best_val / best_idx
 * are initialised when first != 0.  Ties keep the lower class id (argmax semantics).
 * dgtta_regions_merge_f64: the region end of the same loop (a region head: R sigmoid outputs of overlapping regions, see
 * dgtta_logits_regions).  vals double [V][cg] holds outputs c0..c0+cg-1 of the SUM over members of the window-normalised logits
 * (what the *_chunk_f64 functions return after the dgtta_resample_axis passes).  label int32 [V] starts from 0 when first != 0,
 * otherwise from what it holds; for j = 0..cg-1 in order, label = h_order[c0 + j] where vals[v][j] > 0 (exactly 0, -0.0 and NaN are
 * not in the region; the sign of the sum is the sign of the mean).  Merged in ascending c0 the calls are nnU-Net's
 * convert_probabilities_to_segmentation for regions: the last positive region of regions_class_order wins.  probs_out: NULL, or
 * [R][V] plane-major of prob_dtype (DGTTA_F32 / DGTTA_F16): plane c0 + j receives sigmoid(scale * vals[v][j]), scale = 1 / members,
 * evaluated in double by the branch that never overflows.  h_order is a HOST array of R positive labels, 1 <= R <= 32, c0 >= 0,
 * c0 + cg <= R, V > 0, scale > 0, prob_dtype one of the two when probs_out is set: anything else DGTTA_ERR_BADARG.  Restated from
 * memory of nnunetv2 2.2.1, UNPINNED. */
int dgtta_logits_chunk_f64(const float *acc, const float *nsum, double *dst, int C, int X, int Y, int Z, int x0, int y0,
                           int z0, int xs, int ys, int zs, int c0, int cg, void *stream);
int dgtta_argmax_merge_f64(const double *vals, int64_t V, int cg, int c0, double *best_val, int *best_idx, int first,
                           void *stream);
int dgtta_logits_chunk_f64_t(const void *acc, const float *nsum, double *dst, int C, int X, int Y, int Z, int x0, int y0,
                             int z0, int xs, int ys, int zs, int c0, int cg, int acc_dtype, void *stream);
int dgtta_regions_merge_f64(const double *vals, int64_t V, int cg, int c0, double scale, const int *h_order, int R, int *label,
                            void *probs_out, int prob_dtype, int first, void *stream);

/* Sliding-window accumulation in FEATURE space (round 5).  The segmentation head is a 1x1x1 convolution and the last layer of the
 * network, so sum_w g_w (W z_w + b) = W (sum_w g_w z_w) + b sum_w g_w: the volume accumulator holds the 32 Gaussian-weighted feature
 * channels of the last decoder block (128 B per voxel instead of 420 B for 105 fp32 logits; 16 GiB instead of 52.5 GiB at 512^3) and
 * the head runs once per voxel at the end.  Replaces, for the label map the reference writes (dg_tta/tta/tta.py:404-413), the
 * accumulate / average / argmax chain of nnunetv2==2.2.1 predict_sliding_window_return_logits + predict_logits_from_preprocessed_data
 * (reached from dg_tta/tta/nnunet_utils.py:116-125, 208-230); sums are re-associated in fp32 (labels can differ at float ties).
 * dgtta_feature_window_accumulate: facc[(x0.., y0.., z0..)][k] += gauss[p] * z[p][k], nsum[..] += gauss[p] for one window;
 *   z [PD][PH][PW][Cin = 32] in `dtype` storage (DGTTA_F32 / BF16 / F16), facc [X][Y][Z][32] fp32, nsum [X][Y][Z] fp32 or NULL.
 * dgtta_feature_head_argmax: argmax_out[v] = argmax_c sum_m (w[m][c] . facc[m][v]) + nsum[v] * bsum[c] over V voxels; facc member m
 *   starts at facc + m * member_stride (floats), w [M][C][32], bsum [C] = sum over members of the head biases.  First maximum wins.
 * dgtta_feature_logits_chunk_f64: the export path's class chunk (see dgtta_logits_chunk_f64) evaluated from the features in double:
 *   dst[x][y][z][j] = sum_m (w[m][c0 + j] . facc[m][sv]) / nsum[sv] + bsum[c0 + j]. */
int dgtta_feature_window_accumulate(const void *z, const float *gauss, float *facc, float *nsum, int Cin, int PD, int PH, int PW, int X,
                                    int Y, int Z, int x0, int y0, int z0, int dtype, void *stream);
/* ... with the InstanceNorm + LeakyReLU apply of the block in front of the head folded in: y [PD][PH][PW][32] is that block's raw conv
 * output, mean_rstd [32][2] the window's statistics (dgtta_instnorm_lrelu_fwd with z = NULL leaves them without applying them);
 * z = round_dtype(lrelu(y * rstd * gamma + (beta - mean * rstd * gamma))) is formed in registers - the values the apply pass writes. */
int dgtta_feature_window_accumulate_norm(const void *y, const float *mean_rstd, const float *gamma, const float *beta, float slope,
                                         const float *gauss, float *facc, float *nsum, int Cin, int PD, int PH, int PW, int X, int Y,
                                         int Z, int x0, int y0, int z0, int dtype, void *stream);
/* ... for nsrc = 1..4 windows of one network pass that overlap along the last axis, one SEGMENT of that axis per call: h_srcs[k] (a HOST array of device pointers, like h_mean_rstds and h_zoffs) is window
 * k's features (h_mean_rstds == NULL) or raw conv output (h_mean_rstds[k] = its statistics), h_zoffs[k] the segment's first voxel in window
 * k's coordinates, seg_len its length, (x0, y0, z0) its first voxel in the volume.  Contributions are added in window order in
 * registers - the bits nsrc single-window calls produce - and the accumulator is read and written once. */
int dgtta_feature_window_accumulate_multi(const void *const *h_srcs, const float *const *h_mean_rstds, const int *h_zoffs, int nsrc,
                                          const float *gamma, const float *beta, float slope, const float *gauss, float *facc,
                                          float *nsum, int Cin, int PD, int PH, int PW, int seg_len, int X, int Y, int Z, int x0, int y0,
                                          int z0, int dtype, void *stream);
int dgtta_feature_head_argmax(const float *facc, int64_t member_stride, const float *nsum, const float *w, const float *bsum, int M,
                              int Cin, int C, int64_t V, int64_t *argmax_out, void *stream);
int dgtta_feature_logits_chunk_f64(const float *facc, int64_t member_stride, const float *nsum, const float *w, const float *bsum,
                                   double *dst, int M, int Cin, int C, int X, int Y, int Z, int x0, int y0, int z0, int xs, int ys,
                                   int zs, int c0, int cg, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Softmax end of the ensemble prediction: probabilities, confidence and entropy maps beside the label map.  The reference writes
 * label maps only (dg_tta/tta/tta.py:404-413); the definitions are nnU-Net's `save_probabilities` ones from memory, UNPINNED.
 * For voxel v, members m = 1..M, classes c = 0..C-1:
 *   l_c(v)     = (sum_m w[m][c] . facc[m][v] + n(v) bsum[c]) / (M n(v))     the ensemble-MEAN window-normalised logit
 *   p          = softmax_c(l) over ALL C classes;   label = argmax_c l_c, first maximum wins
 *   confidence = p[label] = 1 / S,   S = sum_c exp(l_c - l_max)
 *   entropy    = -sum_c p_c ln p_c = ln S - (sum_c (l_c - l_max) exp(l_c - l_max)) / S      (nats, in [0, ln C])
 *   probs[k]   = p[sel[k]], k < K: 1 <= K <= 32 DISTINCT classes in any order (h_sel is a HOST array; a duplicate or a class outside
 *                [0, C) is DGTTA_ERR_BADARG).  The K planes sum to at most 1: the rest is mass on classes that were not selected.
 *
 * dgtta_feature_head_softmax: all of it from the feature-space accumulators in one pass on the matrix cores - the inputs of
 *   dgtta_feature_head_argmax and the same accumulation order, so label_out holds the integers that function writes.  label_out
 *   int64 [V], conf_out / entropy_out fp32 [V], probs_out [K][V] (plane-major) of prob_dtype DGTTA_F32 or DGTTA_F16.  C <= 128 and
 *   a weight image (M x 128-class blocks) that fits the LDS, else DGTTA_ERR_UNSUPPORTED: the caller takes the class-group path.
 *
 * dgtta_softmax_merge_f64 / dgtta_softmax_finalize_f64: the same quantities for the class-group export loop (beside
 *   dgtta_argmax_merge_f64, which keeps producing the label).  vals double [V][cg] holds classes c0.. of the SUM over members of the
 *   normalised logits (what the *_chunk_f64 functions return, resampled or not); l = scale * vals with scale = 1 / M.  run_max,
 *   run_sum, run_dot double [V]: the running maximum, sum exp(l - max) and sum (l - max) exp(l - max), rescaled when the maximum
 *   moves; initialised when first != 0.  stash double [K][V] receives l of every selected class that falls in this group (fp64:
 *   8 K V bytes, 17 GB at 512^3 with K = 16) - every selected class must lie in one of the merged groups.  finalize turns the state
 *   into conf_out, entropy_out and probs_out as above.
 * ------------------------------------------------------------------------------------------- */
int dgtta_feature_head_softmax(const float *facc, int64_t member_stride, const float *nsum, const float *w, const float *bsum, int M,
                               int Cin, int C, int64_t V, const int *h_sel, int K, int prob_dtype, int64_t *label_out, float *conf_out,
                               float *entropy_out, void *probs_out, void *stream);
int dgtta_softmax_merge_f64(const double *vals, int64_t V, int cg, int c0, double scale, double *run_max, double *run_sum,
                            double *run_dot, const int *h_sel, int K, double *stash, int first, void *stream);
int dgtta_softmax_finalize_f64(const double *run_max, const double *run_sum, const double *run_dot, const double *stash, int64_t V,
                               int K, int prob_dtype, float *conf_out, float *entropy_out, void *probs_out, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Surface-distance metrics of the folder evaluation (HD95, HD, ASSD, NSD; dg_tta_amd/tta/evaluation.py).  The reference
 * delegates evaluation to nnU-Net (dg_tta/tta/tta.py:447-470) and computes none of them: the definitions are the published
 * ones, UNPINNED.  Label maps are int64 [D][H][W].
 *
 * label_bboxes: boxes int32 [nlab][6] = (lo d, lo h, lo w, hi d, hi h, hi w), the inclusive bounding box of the voxels that
 * carry label l in map a OR in map b; a label in neither gets the empty box (INT_MAX x 3, -1 x 3: lo > hi).  The table is
 * initialised here; values outside [0, nlab) are passed over.  nlab <= 1024.
 *
 * label_surface: surf uint8 [cd][ch][cw] = S(map == label) inside the crop box that starts at (d0, h0, w0): 1 where the
 * voxel carries the label and at least one of its six face neighbours does not.  Outside the VOLUME counts as "does not";
 * the box edge is no edge: neighbours are read from the full map.
 *
 * edt_sq: dist2 float [D][H][W] = squared physical distance from every voxel to the nearest nonzero voxel of `site`
 * (uint8 [D][H][W]); +inf everywhere when there is none.  Exact and separable, three passes of one operator along W, then H,
 * then D, starting from 0 at a site and +inf elsewhere:
 *     out[i] = min_j ( in[j] + (s * (float)(i - j))^2 )           s = the axis' spacing (sw, sh, sd)
 * evaluated in fp32 in exactly this order - the product, its square, the add, the min - with no fused multiply-add.  At unit
 * spacing every value is an integer below 2^24 and the result is exact.  Otherwise, with u = 2^-24 and the spacings taken as
 * the floats they are: a pass rounds the product (which the square counts twice), the square and the sum; the W pass adds to 0
 * or +inf, which is exact, and a term is rounded by the sums of the later passes only, so the W term collects 3 + 2 roundings,
 * the H term 3 + 2, the D term 3 + 1: the relative error against real arithmetic is at most (1 + u)^5 - 1 = 5 u to first
 * order.  Spacings in (0, 1e6].  Every axis at most DGTTA_EDT_MAX_AXIS voxels (above:
 * DGTTA_ERR_UNSUPPORTED).  ws: dgtta_edt_ws_bytes(D, H, W) bytes, 4-byte aligned; site, dist2 and ws must not overlap.
 * ------------------------------------------------------------------------------------------- */
#define DGTTA_EDT_MAX_AXIS 1024
int dgtta_label_bboxes(const int64_t *a, const int64_t *b, int D, int H, int W, int nlab, int *boxes, void *stream);
int dgtta_label_surface(const int64_t *map, int D, int H, int W, int64_t label, int d0, int h0, int w0, int cd, int ch, int cw,
                        uint8_t *surf, void *stream);
size_t dgtta_edt_ws_bytes(int D, int H, int W);
int dgtta_edt_sq(const uint8_t *site, float *dist2, void *ws, size_t ws_bytes, int D, int H, int W, float sd, float sh, float sw,
                 void *stream);

/* ---------------------------------------------------------------------------------------------
 * Connected-component post-processing of a prediction (dg_tta_amd/tta/postprocessing.py): keep the largest component of an
 * organ, drop small islands.  The reference leaves this to the user's postprocess_results_fn; the definitions below are this
 * library's, UNPINNED.  Label maps are int64 [D][H][W]; n = D*H*W must be below 2^31 - 1 (DGTTA_ERR_UNSUPPORTED otherwise):
 * components are named by int32.
 *
 * group: int32 [ntab] on the device, ntab <= DGTTA_CC_MAX_TABLE.  g(i) = group[map[i]], and 0 where map[i] lies outside
 * [0, ntab) or the entry lies outside [0, ntab).  Group 0 is "not looked at".  Two voxels are connected iff they are neighbours
 * under `connectivity` (6 faces, 18 + edges, 26 + corners) and have equal, non-zero g: each label its own group, several
 * labels sharing a group (a region), or all foreground in one group.
 *
 * cc_label: cc int32 [D][H][W] = 0 where g == 0, elsewhere 1 + the smallest linear index (d*H + h)*W + w of the voxel's
 * component: canonical, the same on every run.  ws: dgtta_cc_ws_bytes(D, H, W) bytes, 4-byte aligned; it holds the
 * union-find forest, which is built tile by tile in LDS, united across tile borders with atomicMin (always the larger root
 * under the smaller) and flattened by a launch of its own.
 *
 * cc_sizes: size int32 [n]; size[r] = the number of voxels with cc == r + 1, so 0 wherever r is not a component's first
 * voxel.  Cleared here.
 *
 * cc_filter: out int64 [n].  winner[c] = the largest component of group c, ties to the smaller cc.  A voxel with g != 0
 * keeps its label iff (keep_largest == 0 or its component is winner[g]) and its component has at least min_voxels voxels;
 * otherwise it becomes `background`.  Voxels with g == 0 pass through.  removed int64 [ntab] (8-byte aligned) = the number
 * of voxels removed per group id, cleared here.  cc and size must come from cc_label / cc_sizes with the same map and
 * group table.  ws: at least 8 * ntab bytes, 8-byte aligned (dgtta_cc_ws_bytes is enough; the buffer of cc_label may be
 * reused).  out must not overlap map.
 * ------------------------------------------------------------------------------------------- */
#define DGTTA_CC_MAX_TABLE 1024
size_t dgtta_cc_ws_bytes(int D, int H, int W);
int dgtta_cc_label(const int64_t *map, const int *group, int ntab, int D, int H, int W, int connectivity, int *cc, void *ws,
                   size_t ws_bytes, void *stream);
int dgtta_cc_sizes(const int *cc, int64_t n, int *size, void *stream);
int dgtta_cc_filter(const int64_t *map, const int *group, int ntab, const int *cc, const int *size, int64_t n, int keep_largest,
                    int min_voxels, int64_t background, int64_t *out, int64_t *removed, void *ws, size_t ws_bytes, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Hole filling (csrc/components.hip): the same labelling on the COMPLEMENT of a uint8 membership mask [D][H][W] (non-zero =
 * member).  A voxel outside the mask is enclosed iff its component of the complement under `connectivity` has no voxel on any
 * of the six faces of the volume; an axis of extent 1 or 2 therefore encloses nothing.  With connectivity 6 this is
 * scipy.ndimage.binary_fill_holes (18 / 26: structure = generate_binary_structure(3, 2) / (3, 3)); equal to scipy's by test.
 * n = D*H*W must be below 2^31 - 1.
 *
 * holes_fill: out uint8 [n] = 1 on the mask and its enclosed voxels, else 0; must not overlap mask.  n_filled (8-byte
 * aligned) = the number of enclosed voxels.  box: NULL, or int32 [6] = the inclusive bounding box of out (lo d, h, w, hi d,
 * h, w; lo > hi when out is empty).  Both are cleared here.  ws: dgtta_holes_ws_bytes(D, H, W) bytes, 4-byte aligned (the
 * forest and one flag byte per voxel).  Integer valued: the same on every run.
 *
 * holes_member / holes_apply: one entry of fill_label_holes (tta/postprocessing.py) inside a crop box (d0, h0, w0) +
 * (cd, ch, cw) of an int64 label map, whose faces then count as the volume's.  member: mask uint8 [cd][ch][cw] = 1 where
 * group[map] != 0 (the table rule of cc_label).  apply: IN PLACE, a voxel of the box with filled != 0, mask == 0 and
 * map == background becomes `label`; count (8-byte aligned, cleared here) = the voxels changed.
 *
 * nonzero_mask: mask uint8 [n] = OR over c of (data[c][i] != 0) for float32 data [C][n], with IEEE comparison: NaN counts as
 * non-zero, -0.0 as zero (numpy's `!=`).  The mask of nnU-Net's crop_to_nonzero before its holes are filled.
 * ------------------------------------------------------------------------------------------- */
size_t dgtta_holes_ws_bytes(int D, int H, int W);
int dgtta_holes_fill(const uint8_t *mask, int D, int H, int W, int connectivity, uint8_t *out, int64_t *n_filled, int *box, void *ws,
                     size_t ws_bytes, void *stream);
int dgtta_holes_member(const int64_t *map, int D, int H, int W, const int *group, int ntab, int d0, int h0, int w0, int cd, int ch,
                       int cw, uint8_t *mask, void *stream);
int dgtta_holes_apply(int64_t *map, int D, int H, int W, const uint8_t *mask, const uint8_t *filled, int d0, int h0, int w0, int cd,
                      int ch, int cw, int64_t background, int64_t label, int64_t *count, void *stream);
int dgtta_nonzero_mask(const float *data, int C, int64_t n, uint8_t *mask, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Rotation / scaling augmentation of pre-training (csrc/spatial_aug.hip, dg_tta_amd/pretraining/spatial.py): patches sampled
 * through an affine voxel map the way nnU-Net 2.2 samples them with scipy.ndimage.map_coordinates (restated from memory,
 * UNPINNED).  Volumes are fp32 [D][H][W] with fewer than 2^31 voxels.
 *
 * bspline3_prefilter: dst = scipy.ndimage.spline_filter(src, order=3, mode="mirror") in fp32: along every axis gain 6, pole
 * sqrt(3) - 2, the causal and anticausal recursion with the mirror initialisation (its sum cut after 64 terms, below fp32
 * resolution); an axis of extent 1 is left as it is.  dst may be src.  Three launches; once per case.
 *
 * patch_sample_aug: items is a HOST array of n_items <= DGTTA_PATCH_MAX_ITEMS descriptors, copied into the kernel arguments
 * (nothing is read from it after the call returns).  Output voxel v = (d, h, w) of item b reads the source position
 *     x = map[0..2] . v + map[3],  map[4..6] . v + map[7],  map[8..10] . v + map[11]         (D, H, W order, voxel units)
 * evaluated in double from the fp32 entries, which must be finite.  image float [B][1][PD][PH][PW]:
 * map_coordinates(order, mode="constant", cval=0) - 0 when x leaves [0, n - 1] on any axis, else the (order + 1)^3 taps
 * around x with mirrored tap indices; order 3 reads it.image as B-spline COEFFICIENTS (bspline3_prefilter), order 1 as the raw
 * volume.  labels int64 [B][PD][PH][PW] from it.label (a label map stored as fp32 values): of the 8 trilinear corners of x,
 * those outside the volume carry label 0; the mass of a label is the sum of the weights of the corners that carry it; the
 * result is the largest label > 0 whose mass is >= 0.5, else 0.  order: 1 or 3 (DGTTA_ERR_UNSUPPORTED otherwise).  One launch.
 * ------------------------------------------------------------------------------------------- */
#define DGTTA_PATCH_MAX_ITEMS 16
typedef struct DgttaPatchItem {
  const float *image; /* device: coefficients (order 3) or raw volume (order 1) */
  const float *label; /* device: label map */
  int D, H, W;
  float map[12];      /* row-major 3 x 4 [A | t] */
} DgttaPatchItem;
int dgtta_bspline3_prefilter(const float *src, float *dst, int D, int H, int W, void *stream);
int dgtta_patch_sample_aug(const DgttaPatchItem *items, int n_items, int PD, int PH, int PW, int order, float *image,
                           int64_t *labels, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Intensity augmentation of pre-training (csrc/intensity_aug.hip, dg_tta_amd/pretraining/intensity.py): the kernels under
 * nnU-Net's noise / blur / brightness / contrast / gamma transforms (restated from memory of nnunetv2 2.2 / batchgenerators,
 * UNPINNED).  x is a batch [B][V] of fp32 items, V = D*H*W < 2^31 voxels each.  Every entry point takes a HOST array of
 * n_items <= DGTTA_INTENSITY_MAX_ITEMS descriptors that is copied into the kernel arguments (nothing is uploaded, nothing is
 * read from it after the call returns); `item` is the index of the batch item a descriptor works on.  A batch item that no
 * descriptor names is neither read nor written.  No operation below is fused into an FMA.
 *
 * intensity_stats: stats[item][4] = (min, max, mean, population standard deviation) of the item, as doubles on the device.
 * min / max are the exact fp32 values.  With the pivot p = the item's first voxel, S1 = sum (x - p) and S2 = sum (x - p)^2 are
 * formed in double (x - p and its square of two fp32 values are exact or rounded once in double): one partial per workgroup of
 * 4096 voxels in `ws`, added in a fixed order by one last workgroup;
 *     mean = p + S1 / V,   std = sqrt(max(S2 / V - (S1 / V)^2, 0))
 * so a constant item has std = 0 exactly.  No floating-point atomics: the same bits on every run.
 * ws: dgtta_intensity_stats_ws_bytes(n_items, V) bytes, 8-byte aligned.  Two launches.
 *
 * intensity_map: dst[item] = f(src[item]) voxel by voxel, one launch, mode and parameters per descriptor.  dst may be src.
 * Statistics are read on the device from `stats` (and `stats2`), rows [item][4] as intensity_stats writes them, each value
 * rounded to fp32 ONCE; all per-voxel arithmetic is fp32 in the order written:
 *   DGTTA_IMAP_LINEAR    y = x * a + s * n(v)              (s == 0: y = x * a, the generator is not called)
 *   DGTTA_IMAP_CONTRAST  mean, lo, hi = fp32(stats mean, min, max);  y = min(max((x - mean) * a + mean, lo), hi)
 *   DGTTA_IMAP_GAMMA     negate = 0: lo = fp32(min);  negate = 1: x = -x, lo = -fp32(max);  r = fp32(max - min) (the
 *                        difference taken in double);  y = powf((x - lo) / (r + 1e-7f), a) * r + lo
 *                        (y is NOT negated back: the statistics of the next step are those of the negated item)
 *   DGTTA_IMAP_RESTORE   mn = fp32(stats mean) (negate = 1: -fp32(stats mean)), sd = fp32(stats std), mn2, sd2 = fp32(stats2
 *                        mean, std);  y = (x - mn2) / (sd2 + 1e-8f) * sd + mn;  negate = 1: y = -y
 * 1e-7f / 1e-8f are the fp32 values nearest 1e-7 / 1e-8.  stats is needed by every mode but LINEAR, stats2 by RESTORE.
 * The noise n(v) of voxel v (index inside the item) is counter-based, Philox4x32-10 + Box-Muller exactly as the seeded MIND
 * noise above (csrc/philox.h), one Philox call per four voxels:
 *   (x0,x1,x2,x3) = Philox4x32-10(counter = (v >> 2, noise_b, off_lo, off_hi), key = (seed_lo, seed_hi))
 *   v & 3 == 0: sqrt(-2 ln u0) cos(2 pi u1)   1: sqrt(-2 ln u0) sin(2 pi u1)   2, 3: the same from (u2, u3)
 * It depends on (seed, offset, noise_b, v) only: an item launched alone with the same noise_b draws the same field.  There is
 * no noise tensor and no generator state.
 *
 * gauss_blur3: scipy.ndimage.gaussian_filter(item, sigma, order=0, mode="reflect", truncate=4) for sigma <= 1, separable, the
 * axes in the order D, H, W: out[i] = sum_{k = 0 .. 2 radius} taps[k] * in[reflect(i + k - radius)] added in ascending k in fp32,
 * reflect(j) = j mod 2n, mirrored (2n - 1 - j) when >= n - correct for extents shorter than the radius too.  taps: the caller's
 * 2 radius + 1 <= 9 normalised weights (float64 exp(-x^2 / (2 sigma^2)) / sum, rounded to fp32), radius = int(4 sigma + 0.5)
 * in 1 .. 4.  Three launches: D pass src -> scratch, H pass scratch -> dst, W pass dst -> dst (a whole row is staged in LDS
 * before it is written; W <= 2048).  dst may be src; scratch [B][V] is neither.
 * ------------------------------------------------------------------------------------------- */
#define DGTTA_INTENSITY_MAX_ITEMS 16
#define DGTTA_IMAP_LINEAR 0
#define DGTTA_IMAP_CONTRAST 1
#define DGTTA_IMAP_GAMMA 2
#define DGTTA_IMAP_RESTORE 3
typedef struct DgttaIntensityItem {
  int item;    /* index in the batch */
  int mode;    /* DGTTA_IMAP_* */
  int negate;  /* GAMMA: negate the input; RESTORE: negate the output */
  int noise_b; /* LINEAR: counter word 1 of the noise */
  float a;     /* LINEAR: multiplier; CONTRAST: factor; GAMMA: exponent */
  float s;     /* LINEAR: noise scale */
  uint32_t seed_lo, seed_hi, off_lo, off_hi; /* LINEAR: Philox key and counter words 2, 3 */
} DgttaIntensityItem;
typedef struct DgttaBlurItem {
  int item;   /* index in the batch */
  int radius; /* 1 .. 4 */
  float taps[9];
} DgttaBlurItem;
size_t dgtta_intensity_stats_ws_bytes(int n_items, int64_t V);
int dgtta_intensity_stats(const float *x, int B, int64_t V, const int *h_items, int n_items, double *stats, void *ws,
                          size_t ws_bytes, void *stream);
int dgtta_intensity_map(const float *src, float *dst, int B, int64_t V, const DgttaIntensityItem *h_items, int n_items,
                        const double *stats, const double *stats2, void *stream);
int dgtta_gauss_blur3(const float *src, float *dst, float *scratch, int B, int D, int H, int W, const DgttaBlurItem *h_items,
                      int n_items, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Mirroring for the stock nnUNetTrainer (csrc/mirror.hip, csrc/window_mirror.h): nnU-Net's MirrorTransform in pre-training and the
 * mirrored passes of its sliding-window predictor (nnunetv2 2.2.1 _internal_maybe_mirror_and_predict), both restated from memory,
 * UNPINNED.  A mirror mask selects the flipped axes of a [D][H][W] block: bit 0 = axis 0 (D), bit 1 = axis 1 (H), bit 2 = axis 2
 * (W); masks outside 0..7 are DGTTA_ERR_BADARG.  Masks and origins are HOST arrays copied into the kernel arguments (one launch per
 * DGTTA_MIRROR_MAX_ITEMS items); the library allocates nothing and does not wait for the stream.
 *
 * dgtta_mirror_batch: image_out[b][c][p] = image[b][c][flip(p)], labels_out[b][p] = labels[b][flip(p)] with item b's mask (mask 0:
 *   a copy); image [B][C][D][H][W] fp32, labels [B][D][H][W] int64, source and destination distinct buffers.
 * dgtta_window_gather: out[k][c][p] = volume[c][origin_k + flip_k(p)] for n windows [PD][PH][PW] of the volume [C][X][Y][Z];
 *   h_origins holds n (x0, y0, z0) triples; a window outside the volume is DGTTA_ERR_BADARG.
 * dgtta_*_window_accumulate_mirror*: the window accumulations above for a mirrored pass - the arguments of the unmirrored entry plus
 *   `mirror`: the destination voxel origin + p receives gauss[p] * (source value at flip(p)), nsum receives gauss[p].  The Gaussian is
 *   NOT flipped (at even tile sizes the flipped map is a different array).  mirror = 0 produces the bits of the unmirrored entry.  The
 *   two logits-space forms take fp32 accumulators only (acc_dtype DGTTA_F32, else DGTTA_ERR_UNSUPPORTED): eight passes per window at
 *   Gaussian weight 10 leave no headroom in half.
 * ------------------------------------------------------------------------------------------- */
#define DGTTA_MIRROR_MAX_ITEMS 16
int dgtta_mirror_batch(const float *image, const int64_t *labels, float *image_out, int64_t *labels_out, const int *h_masks, int B,
                       int C, int D, int H, int W, void *stream);
int dgtta_window_gather(const float *volume, float *out, const int *h_origins, const int *h_masks, int n, int C, int PD, int PH, int PW,
                        int X, int Y, int Z, void *stream);
int dgtta_feature_window_accumulate_mirror(const void *z, const float *gauss, float *facc, float *nsum, int Cin, int PD, int PH, int PW,
                                           int X, int Y, int Z, int x0, int y0, int z0, int dtype, int mirror, void *stream);
int dgtta_feature_window_accumulate_norm_mirror(const void *y, const float *mean_rstd, const float *gamma, const float *beta, float slope,
                                                const float *gauss, float *facc, float *nsum, int Cin, int PD, int PH, int PW, int X,
                                                int Y, int Z, int x0, int y0, int z0, int dtype, int mirror, void *stream);
int dgtta_seghead_window_accumulate_mirror_t(const void *z, const float *w, const float *bias, const float *gauss, void *acc,
                                             float *nsum, int Cin, int C, int PD, int PH, int PW, int X, int Y, int Z, int x0, int y0,
                                             int z0, int dtype, int acc_dtype, int mirror, void *stream);
int dgtta_window_accumulate_mirror_t(const float *patch, const float *gauss, void *acc, float *nsum, int C, int PD, int PH, int PW,
                                     int X, int Y, int Z, int x0, int y0, int z0, int acc_dtype, int mirror, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Dataset fingerprint (csrc/fingerprint.hip, dg_tta_amd/planning/fingerprint.py): exact pooled statistics of the foreground
 * voxels (seg > 0) of one image channel over all training cases.  One call per case and sweep; the kernels hold no state: the
 * running histogram `counters` and the running `state` are the caller's device buffers, zeroed / initialised by the caller and
 * carried from case to case.  x: fp32 [V]; seg: [V] labels of type seg_dtype (DGTTA_SEG_*).  Three launches at most, all on
 * `stream`; nothing is allocated and the stream is not waited for.
 *
 * Histogram.  key(v) = bits(v) ^ 0x80000000 for a value with a clear sign bit, ~bits(v) otherwise: unsigned order of the keys =
 * order of the values (-0.0 sorts before +0.0).  With the key's leading prefix_bits bits as its prefix and the next digit_bits
 * (1 .. 11) bits as its digit, counters[t][d] (uint64 [n_prefixes][DGTTA_FP_BINS]) grows by the number of finite foreground
 * values whose prefix is h_prefixes[t] and whose digit is d.  prefix_bits = 0: one histogram of all finite foreground values,
 * h_prefixes is not read, n_prefixes = 1.  The prefixes (HOST array, copied into the kernel arguments) are distinct.  Every
 * workgroup counts in LDS and stores its histogram to a slab of `ws`; a second launch adds the slabs in ascending order.
 * Exact: integer counts only.
 *
 * Moments.  moment = 0: none.  moment = 1: state->count, min, max, sum (double) and nonfinite grow by the case's finite /
 * non-finite foreground values; first_nonfinite_case becomes case_index if the case has a non-finite foreground value and the
 * field is still negative.  moment = 2: sumsq_centred grows by the case's sum of ((double)x - mean)^2.  Non-finite foreground
 * values are counted and left out of everything else (histogram included).  Double sums per thread in index order, a fixed tree
 * across the workgroup, the workgroups' partials added in ascending order, the case's sum added to the state: the same bits on
 * every run for a given order of the cases.  No floating-point atomics.
 * Initial state: count = nonfinite = 0, first_nonfinite_case = -1, min = +inf, max = -inf, sum = sumsq_centred = 0.
 * ws: dgtta_fingerprint_ws_bytes(V, n_prefixes) bytes (0 for arguments out of range), 8-byte aligned.
 * ------------------------------------------------------------------------------------------- */
#define DGTTA_FP_BINS 2048
#define DGTTA_FP_MAX_PREFIXES 6
#define DGTTA_SEG_U8 0
#define DGTTA_SEG_I16 1
#define DGTTA_SEG_I32 2
typedef struct DgttaFingerprintState {
  uint64_t count;               /* finite foreground values */
  uint64_t nonfinite;           /* NaN / inf foreground values */
  int64_t first_nonfinite_case; /* case_index of the first case that had one, else negative */
  double min, max;              /* exact fp32 values */
  double sum;                   /* of the finite foreground values */
  double sumsq_centred;         /* of (x - mean)^2 */
} DgttaFingerprintState;
size_t dgtta_fingerprint_ws_bytes(int64_t V, int n_prefixes);
int dgtta_fingerprint_sweep(const float *x, const void *seg, int seg_dtype, int64_t V, int moment, double mean, int64_t case_index,
                            int prefix_bits, int digit_bits, const uint32_t *h_prefixes, int n_prefixes, uint64_t *counters,
                            DgttaFingerprintState *state, void *ws, size_t ws_bytes, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* DGTTA_H */
