// Supervised loss of REGION-BASED datasets (nnU-Net's second label model): soft Dice + binary cross-entropy of R sigmoid outputs
// against overlapping regions of an integer label map, forward and backward.  A dataset.json whose label values are lists (KiTS:
// kidney_and_masses = [1, 2, 3], masses = [2, 3], tumor = 2) describes R regions; the network has one output per region and no
// background channel, and nnU-Net trains it with DC_and_BCE_loss(MemoryEfficientSoftDiceLoss(do_bg=True, smooth=1e-5), weights
// 1 / 1) [3P nnunetv2==2.2.1, not available here] - restated FROM MEMORY, UNPINNED:
//   s = sigmoid(z);  t[b][v][r] = bit r of table[y_bv]      table: uint32 [L], bit r of entry y set when label y belongs to region r
//   a voxel is valid when 0 <= y < L; anything else is left out of every sum (dice_ce.hip's rule for labels outside [0, C))
//   bce   = (1 / (N R)) sum_{valid v, r} [ max(z, 0) - t z + log1p(exp(-|z|)) ]          N = valid voxels of the whole batch
//   dc_br = (2 sum_v s t + smooth) / max(sum_v s + sum_v t + smooth, 1e-8)               per sample b and region r
//   loss  = bce - mean_{b, r} dc_br
// Batch Dice pools the three sums over b before the ratio and leaves bce alone (dice_ce.hip's header; the finalize kernel alone
// knows the mode).  Gradient, with the quotient rule's alpha = -2 w / D, beta = w (2 I + smooth) / D^2 (0 where D was clamped: the
// clamp's derivative), w = 1 / (B R) or 1 / R:
//   dL/dz = (s - t) / (N R) + s (1 - s) (alpha_br t + beta_br)                           on valid voxels, 0 elsewhere
// A batch without a valid voxel has bce = 0 and a zero gradient.
// No region target tensor exists: nnU-Net materialises [B, R, D, H, W]; here a voxel costs its 8 bytes of label and a table
// lookup in LDS.  The deep-supervision entries (dgtta_region_loss_ds_*) read the FULL-resolution label map through label_map.h's
// index map, as dgtta_dice_ce_ds_* do: no downsampled label map exists either.
// Structure and reproducibility are dice_ce.hip's: voxel-major fp32 rows of pitch ldc staged 128 at a time through LDS, double
// partial sums per workgroup in fixed slots {sum s t, sum s, sum t}[R], sum bce, valid voxels; ONE finalize workgroup adds the
// slots in order (and over b in ascending order for batch Dice); no floating-point atomics: the same bits on every run.
// sigmoid and s (1 - s) are formed from e = exp(-|z|) <= 1 (s = 1 / (1 + e) or e / (1 + e), s (1 - s) = e / (1 + e)^2): nothing
// overflows for any finite z, and at |z| = 80 both are normal fp32 numbers.
#include "common.h"
#include "label_map.h"

namespace {

constexpr int RL_MAXR = 32;                // regions: the bits of a table entry
constexpr int RL_MAXL = 1024;              // label values the table holds
constexpr int RL_TILE = 128;               // voxels per tile (dice_ce.hip: rows staged through LDS as one contiguous run)
constexpr int RL_THREADS = 256;
constexpr int RL_PARTS = 8;                // the tile's region sums: RL_PARTS threads per region, 16 voxels each, added in order

__host__ __device__ inline int rl_pitch(int R) { return R | 1; }
inline int rl_blocks(int64_t V) {
  const int64_t b = (V + RL_TILE - 1) / RL_TILE;
  return (int)(b < 1024 ? b : 1024);
}
inline size_t rl_partial_doubles(int B, int R, int64_t V) { return (size_t)B * rl_blocks(V) * (3 * R + 2); }

// rows [nv][ld] in memory <-> tile [nv][R | 1] in LDS (odd pitch: a lane per voxel walks its row conflict free)
__device__ __forceinline__ void rl_tile_load(float *tile, const float *src, int nv, int R, int ld, int LDP) {
  if (ld == R) {
    // eight loads in flight per thread before the first LDS store
    const int n = nv * R;
    for (int e0 = threadIdx.x; e0 < n; e0 += RL_THREADS * 8) {
      float tmp[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int e = e0 + RL_THREADS * u;
        tmp[u] = e < n ? src[e] : 0.f;
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int e = e0 + RL_THREADS * u;
        if (e < n) {
          const int v = e / R;
          tile[v * LDP + (e - v * R)] = tmp[u];
        }
      }
    }
  } else {
    for (int e = threadIdx.x; e < nv * R; e += RL_THREADS) {
      const int v = e / R, r = e - v * R;
      tile[v * LDP + r] = src[(int64_t)v * ld + r];
    }
  }
}
__device__ __forceinline__ void rl_tile_store(const float *tile, float *dst, int nv, int R, int ld, int LDP) {
  for (int e = threadIdx.x; e < nv * R; e += RL_THREADS) {
    const int v = e / R, r = e - v * R;
    dst[(int64_t)v * ld + r] = tile[v * LDP + r];
  }
}

// e = exp(-|z|) -> sigmoid(z) and sigmoid'(z), overflow free (file header)
__device__ __forceinline__ void rl_sigmoid(float z, float &e, float &s, float &ds) {
  e = expf(-fabsf(z));
  const float inv = 1.0f / (1.0f + e);
  s = z >= 0.f ? inv : e * inv;
  ds = e * inv * inv;
}

// partial[(b * nblk + blk) * (3R + 2) + {r, R + r, 2R + r, 3R, 3R + 1}] = {sum s t, sum s, sum t, sum bce terms, valid voxels}
__global__ __launch_bounds__(RL_THREADS) void region_loss_fwd_kernel(const float *__restrict__ logits, int ldc,
                                                                    const int64_t *__restrict__ labels,
                                                                    const uint32_t *__restrict__ table, int L,
                                                                    double *__restrict__ partial, int R, int64_t V, DcLabels lm) {
  extern __shared__ float rl_tile[];               // [RL_TILE][R | 1]
  __shared__ uint32_t s_tab[RL_MAXL];
  __shared__ uint32_t s_bits[RL_TILE];             // a voxel's region memberships (0: background, or not valid - its row is 0 then)
  __shared__ float s_part[3][RL_PARTS][RL_MAXR];
  __shared__ float s_red[16];
  const int LDP = rl_pitch(R);
  const int b = blockIdx.y, t = threadIdx.x;
  for (int i = t; i < L; i += RL_THREADS) s_tab[i] = table[i];
  const float *lb = logits + (int64_t)b * V * ldc;
  double aI = 0.0, aP = 0.0, aY = 0.0, bce = 0.0, nv_tot = 0.0;
  const int pr = t % R, pp = t / R;                // region and part of the tile's region sums (t < RL_PARTS R)
  const int64_t ntile = (V + RL_TILE - 1) / RL_TILE;
  for (int64_t tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
    const int64_t v0 = tile * RL_TILE;
    const int nv = V - v0 < RL_TILE ? (int)(V - v0) : RL_TILE;
    rl_tile_load(rl_tile, lb + v0 * ldc, nv, R, ldc, LDP);
    __syncthreads();                                 // (the first one also publishes s_tab)
    float term = 0.f, ok = 0.f;
    if (t < RL_TILE) {
      float *row = rl_tile + t * LDP;
      uint32_t bits = 0;
      bool valid = false;
      if (t < nv) {
        const int64_t yl = labels[lm.at(b, v0 + t, V)];
        if (yl >= 0 && yl < L) valid = true, bits = s_tab[yl];
      }
      if (valid) {
        for (int r = 0; r < R; ++r) {
          const float z = row[r];
          float e, s, ds;
          rl_sigmoid(z, e, s, ds);
          term += fmaxf(z, 0.f) - ((bits >> r) & 1u ? z : 0.f) + log1pf(e);
          row[r] = s;
        }
        ok = 1.f;
      } else {
        for (int r = 0; r < R; ++r) row[r] = 0.f;
      }
      s_bits[t] = bits;
    }
    const float tb = block_sum(term, s_red);          // (also the barrier that publishes the sigmoids)
    const float tnv = block_sum(ok, s_red);
    if (t == 0) bce += (double)tb, nv_tot += (double)tnv;
    if (pp < RL_PARTS) {
      float sI = 0.f, sP = 0.f, sY = 0.f;
      for (int q = pp * (RL_TILE / RL_PARTS); q < (pp + 1) * (RL_TILE / RL_PARTS); ++q) {
        const float s = rl_tile[q * LDP + pr];
        const float hit = (s_bits[q] >> pr) & 1u ? 1.f : 0.f;
        sI += s * hit;
        sP += s;
        sY += hit;
      }
      s_part[0][pp][pr] = sI;
      s_part[1][pp][pr] = sP;
      s_part[2][pp][pr] = sY;
    }
    __syncthreads();
    if (t < R) {
      float sI = s_part[0][0][t], sP = s_part[1][0][t], sY = s_part[2][0][t];
      for (int p = 1; p < RL_PARTS; ++p) sI += s_part[0][p][t], sP += s_part[1][p][t], sY += s_part[2][p][t];
      aI += (double)sI;
      aP += (double)sP;
      aY += (double)sY;
    }
    // (the next tile's stores into rl_tile / s_bits / s_part come after its own barrier and this tile's reads before the
    // block_sum barriers of the next tile: s_part is rewritten only after two further barriers)
  }
  double *out = partial + ((int64_t)b * gridDim.x + blockIdx.x) * (3 * R + 2);
  if (t < R) {
    out[t] = aI;
    out[R + t] = aP;
    out[2 * R + t] = aY;
  }
  if (t == 0) {
    out[3 * R] = bce;
    out[3 * R + 1] = nv_tot;
  }
}

// one workgroup: loss[0] = total, loss[1] = bce, loss[2] = -mean dice; dice[B][R]; coef[(b * R + r) * 2 + {0, 1}] = {alpha, beta}
// with dL/ds[v][r] = alpha * t + beta, coef[2 B R] = 1 / (N R).  batch_dice: the sums of a region are pooled over b first; every
// row of dice and every b of coef then holds the region's one value.
__global__ __launch_bounds__(1024) void region_loss_finalize_kernel(const double *__restrict__ partial, int nblk, int B, int R,
                                                                   float smooth, int batch_dice, float *__restrict__ loss,
                                                                   float *__restrict__ dice, float *__restrict__ coef) {
  __shared__ double s_dc[8 * RL_MAXR];
  __shared__ double s_sum[3][8 * RL_MAXR];             // batch mode: the per-sample {I, P, Y} of every (b, r)
  __shared__ double s_bce, s_nv;
  const int n = B * R, W = 3 * R + 2;
  const double w = 1.0 / (double)((batch_dice ? 1 : B) * R);
  // four lanes per (b, r): lane p adds the partial slots p, p + 4, ..., the quad combines in lane order - a fixed summation order
  const int p4 = threadIdx.x & 3;
  {
    const int i = threadIdx.x >> 2;                    // n <= 256 = blockDim.x / 4
    const bool on = i < n;
    const int b = on ? i / R : 0, r = on ? i - b * R : 0;
    double I = 0.0, P = 0.0, Y = 0.0;
    if (on)
      for (int q = p4; q < nblk; q += 4) {
        const double *s = partial + ((int64_t)b * nblk + q) * W;
        I += s[r];
        P += s[R + r];
        Y += s[2 * R + r];
      }
#pragma unroll
    for (int m = 1; m <= 2; m <<= 1) {
      I += __shfl_xor(I, m, 64);
      P += __shfl_xor(P, m, 64);
      Y += __shfl_xor(Y, m, 64);
    }
    if (on && p4 == 0 && batch_dice) {
      s_sum[0][i] = I;
      s_sum[1][i] = P;
      s_sum[2][i] = Y;
    } else if (on && p4 == 0) {
      const double N = 2.0 * I + (double)smooth;
      double D = P + Y + (double)smooth;
      const bool clamped = D < 1e-8;
      if (clamped) D = 1e-8;
      const double dc = N / D;
      s_dc[i] = dc;
      dice[i] = (float)dc;
      coef[2 * i] = (float)(-2.0 * w / D);
      coef[2 * i + 1] = clamped ? 0.f : (float)(w * N / (D * D));
    }
  }
  if (threadIdx.x < 64) {      // bce sum and valid-voxel count: one wave, slots dealt to its lanes, fixed tree
    double bce = 0.0, nv = 0.0;
    for (int q = threadIdx.x; q < B * nblk; q += 64) {
      const double *s = partial + (int64_t)q * W;
      bce += s[3 * R];
      nv += s[3 * R + 1];
    }
    bce = wave_sum_d(bce);
    nv = wave_sum_d(nv);
    if (threadIdx.x == 0) s_bce = bce, s_nv = nv;
  }
  __syncthreads();
  if (batch_dice) {
    if (threadIdx.x < R) {       // a lane per region: the samples' sums in ascending b
      const int r = threadIdx.x;
      double I = s_sum[0][r], P = s_sum[1][r], Y = s_sum[2][r];
      for (int b = 1; b < B; ++b) {
        I += s_sum[0][b * R + r];
        P += s_sum[1][b * R + r];
        Y += s_sum[2][b * R + r];
      }
      const double N = 2.0 * I + (double)smooth;
      double D = P + Y + (double)smooth;
      const bool clamped = D < 1e-8;
      if (clamped) D = 1e-8;
      const double dc = N / D;
      s_dc[r] = dc;
      const float alpha = (float)(-2.0 * w / D), beta = clamped ? 0.f : (float)(w * N / (D * D));
      for (int b = 0; b < B; ++b) {
        dice[b * R + r] = (float)dc;
        coef[2 * (b * R + r)] = alpha;
        coef[2 * (b * R + r) + 1] = beta;
      }
    }
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    double acc = 0.0;
    for (int b = 0; b < (batch_dice ? 1 : B); ++b)
      for (int r = 0; r < R; ++r) acc += s_dc[b * R + r];
    const double nr = (s_nv > 0.0 ? s_nv : 1.0) * (double)R;
    const double bm = s_bce / nr, dl = -acc * w;
    loss[0] = (float)(bm + dl);
    loss[1] = (float)bm;
    loss[2] = (float)dl;
    coef[2 * n] = (float)(1.0 / nr);
  }
}

__global__ __launch_bounds__(RL_THREADS) void region_loss_bwd_kernel(const float *__restrict__ logits, int ldc,
                                                                    const int64_t *__restrict__ labels,
                                                                    const uint32_t *__restrict__ table, int L,
                                                                    const float *__restrict__ coef, float scale,
                                                                    const float *__restrict__ scale_dev, float *__restrict__ grad,
                                                                    int ldg, int B, int R, int64_t V, DcLabels lm) {
  extern __shared__ float rl_tile[];               // [RL_TILE][R | 1]: logits in, gradient out
  __shared__ uint32_t s_tab[RL_MAXL];
  __shared__ float s_coef[2 * RL_MAXR];
  const int LDP = rl_pitch(R);
  const int b = blockIdx.y, t = threadIdx.x;
  for (int i = t; i < L; i += RL_THREADS) s_tab[i] = table[i];
  for (int i = t; i < 2 * R; i += RL_THREADS) s_coef[i] = coef[(int64_t)b * 2 * R + i];
  const float inv_nr = coef[(int64_t)B * 2 * R];
  const float sc = scale * (scale_dev ? scale_dev[0] : 1.0f);
  const int64_t ntile = (V + RL_TILE - 1) / RL_TILE;
  for (int64_t tile = blockIdx.x; tile < ntile; tile += gridDim.x) {
    const int64_t v0 = tile * RL_TILE;
    const int nv = V - v0 < RL_TILE ? (int)(V - v0) : RL_TILE;
    __syncthreads();                                 // previous tile stored (and s_tab, s_coef published)
    rl_tile_load(rl_tile, logits + ((int64_t)b * V + v0) * ldc, nv, R, ldc, LDP);
    __syncthreads();
    if (t < nv) {
      float *row = rl_tile + t * LDP;
      const int64_t yl = labels[lm.at(b, v0 + t, V)];
      if (yl < 0 || yl >= L) {
        for (int r = 0; r < R; ++r) row[r] = 0.f;
      } else {
        const uint32_t bits = s_tab[yl];
        for (int r = 0; r < R; ++r) {
          float e, s, ds;
          rl_sigmoid(row[r], e, s, ds);
          const float hit = (bits >> r) & 1u ? 1.f : 0.f;
          row[r] = sc * ((s - hit) * inv_nr + ds * (s_coef[2 * r] * hit + s_coef[2 * r + 1]));
        }
      }
    }
    __syncthreads();
    rl_tile_store(rl_tile, grad + ((int64_t)b * V + v0) * ldg, nv, R, ldg, LDP);
  }
}

}  // namespace

static bool rl_dims_ok(int B, int R, int64_t V) { return B > 0 && B <= 8 && R >= 1 && R <= RL_MAXR && V > 0; }

// ws: [partials: B * nblk * (3R + 2) double][coef: 2 B R + 1 float], kept between fwd and bwd
extern "C" size_t dgtta_region_loss_ws_bytes(int B, int R, int64_t V) {
  if (!rl_dims_ok(B, R, V)) return 0;
  return align_up(rl_partial_doubles(B, R, V) * sizeof(double), 256) + align_up(((size_t)2 * B * R + 1) * sizeof(float), 256);
}

static int region_loss_fwd(const float *logits, int ldc, const int64_t *labels, const uint32_t *table, int L, float *loss3,
                           float *dice, void *ws, size_t ws_bytes, int B, int R, int64_t V, float smooth, int batch_dice,
                           void *stream, const DcLabels &lm) {
  DG_REQUIRE(logits && labels && table && loss3 && dice && ws, DGTTA_ERR_BADARG, "region_loss_fwd: null pointer");
  DG_REQUIRE(batch_dice == 0 || batch_dice == 1, DGTTA_ERR_BADARG, "region_loss_fwd: batch_dice is 0 or 1, not %d", batch_dice);
  DG_REQUIRE(rl_dims_ok(B, R, V) && ldc >= R && L >= 1 && L <= RL_MAXL, DGTTA_ERR_BADARG,
             "region_loss_fwd: need 1<=B<=8, 1<=R<=%d, ldc>=R, 1<=L<=%d (B=%d R=%d ldc=%d L=%d)", RL_MAXR, RL_MAXL, B, R, ldc, L);
  DG_REQUIRE(ws_bytes >= dgtta_region_loss_ws_bytes(B, R, V), DGTTA_ERR_WORKSPACE, "region_loss_fwd: workspace too small");
  hipStream_t st = (hipStream_t)stream;
  const int nblk = rl_blocks(V);
  double *partial = (double *)ws;
  float *coef = (float *)((char *)ws + align_up(rl_partial_doubles(B, R, V) * sizeof(double), 256));
  const size_t lds = (size_t)RL_TILE * rl_pitch(R) * sizeof(float);      // <= 16.5 KiB: below the default dynamic limit
  hipLaunchKernelGGL(region_loss_fwd_kernel, dim3(nblk, B), dim3(RL_THREADS), lds, st, logits, ldc, labels, table, L, partial, R, V, lm);
  DG_CHECK_LAUNCH("region_loss_fwd_kernel");
  hipLaunchKernelGGL(region_loss_finalize_kernel, dim3(1), dim3(1024), 0, st, partial, nblk, B, R, smooth, batch_dice, loss3, dice, coef);
  DG_CHECK_LAUNCH("region_loss_finalize_kernel");
  return DGTTA_OK;
}

static int region_loss_bwd(const float *logits, int ldc, const int64_t *labels, const uint32_t *table, int L, const void *ws,
                           float grad_scale, const float *grad_scale_dev, float *grad_logits, int ldg, int B, int R, int64_t V,
                           void *stream, const DcLabels &lm) {
  DG_REQUIRE(logits && labels && table && ws && grad_logits, DGTTA_ERR_BADARG, "region_loss_bwd: null pointer");
  DG_REQUIRE(rl_dims_ok(B, R, V) && ldc >= R && ldg >= R && L >= 1 && L <= RL_MAXL, DGTTA_ERR_BADARG,
             "region_loss_bwd: bad dims (B=%d R=%d ldc=%d ldg=%d L=%d)", B, R, ldc, ldg, L);
  const float *coef = (const float *)((const char *)ws + align_up(rl_partial_doubles(B, R, V) * sizeof(double), 256));
  int64_t gx = (V + RL_TILE - 1) / RL_TILE;
  if (gx > 2048) gx = 2048;
  const size_t lds = (size_t)RL_TILE * rl_pitch(R) * sizeof(float);
  hipLaunchKernelGGL(region_loss_bwd_kernel, dim3((unsigned)gx, B), dim3(RL_THREADS), lds, (hipStream_t)stream, logits, ldc, labels,
                     table, L, coef, grad_scale, grad_scale_dev, grad_logits, ldg, B, R, V, lm);
  DG_CHECK_LAUNCH("region_loss_bwd_kernel");
  return DGTTA_OK;
}

extern "C" int dgtta_region_loss_fwd(const float *logits, int ldc, const int64_t *labels, const uint32_t *table, int L,
                                     float *loss3, float *dice, void *ws, size_t ws_bytes, int B, int R, int64_t V, float smooth,
                                     void *stream) {
  return region_loss_fwd(logits, ldc, labels, table, L, loss3, dice, ws, ws_bytes, B, R, V, smooth, 0, stream, DC_DENSE);
}

extern "C" int dgtta_region_loss_batch_fwd(const float *logits, int ldc, const int64_t *labels, const uint32_t *table, int L,
                                           float *loss3, float *dice, void *ws, size_t ws_bytes, int B, int R, int64_t V,
                                           float smooth, int batch_dice, void *stream) {
  return region_loss_fwd(logits, ldc, labels, table, L, loss3, dice, ws, ws_bytes, B, R, V, smooth, batch_dice, stream, DC_DENSE);
}

extern "C" int dgtta_region_loss_bwd(const float *logits, int ldc, const int64_t *labels, const uint32_t *table, int L,
                                     const void *ws, float grad_scale, const float *grad_scale_dev, float *grad_logits, int ldg,
                                     int B, int R, int64_t V, void *stream) {
  return region_loss_bwd(logits, ldc, labels, table, L, ws, grad_scale, grad_scale_dev, grad_logits, ldg, B, R, V, stream, DC_DENSE);
}

// ---- the same loss on logits [B][d][h][w][ld] against the full-resolution label map [B][d sd][h sh][w sw]
extern "C" size_t dgtta_region_loss_ds_ws_bytes(int B, int R, int d, int h, int w) {
  if (d <= 0 || h <= 0 || w <= 0) return 0;
  return dgtta_region_loss_ws_bytes(B, R, (int64_t)d * h * w);
}

extern "C" int dgtta_region_loss_ds_fwd(const float *logits, int ldc, const int64_t *labels_full, const uint32_t *table, int L,
                                        float *loss3, float *dice, void *ws, size_t ws_bytes, int B, int R, int d, int h, int w,
                                        int sd, int sh, int sw, float smooth, void *stream) {
  DG_REQUIRE(dc_ds_dims_ok(d, h, w, sd, sh, sw), DGTTA_ERR_BADARG, "region_loss_ds_fwd: bad dims %dx%dx%d strides %d,%d,%d", d, h, w,
             sd, sh, sw);
  return region_loss_fwd(logits, ldc, labels_full, table, L, loss3, dice, ws, ws_bytes, B, R, (int64_t)d * h * w, smooth, 0, stream,
                         dc_ds_labels(d, h, w, sd, sh, sw));
}

extern "C" int dgtta_region_loss_ds_batch_fwd(const float *logits, int ldc, const int64_t *labels_full, const uint32_t *table,
                                              int L, float *loss3, float *dice, void *ws, size_t ws_bytes, int B, int R, int d,
                                              int h, int w, int sd, int sh, int sw, float smooth, int batch_dice, void *stream) {
  DG_REQUIRE(dc_ds_dims_ok(d, h, w, sd, sh, sw), DGTTA_ERR_BADARG, "region_loss_ds_batch_fwd: bad dims %dx%dx%d strides %d,%d,%d", d,
             h, w, sd, sh, sw);
  return region_loss_fwd(logits, ldc, labels_full, table, L, loss3, dice, ws, ws_bytes, B, R, (int64_t)d * h * w, smooth, batch_dice,
                         stream, dc_ds_labels(d, h, w, sd, sh, sw));
}

extern "C" int dgtta_region_loss_ds_bwd(const float *logits, int ldc, const int64_t *labels_full, const uint32_t *table, int L,
                                        const void *ws, float grad_scale, const float *grad_scale_dev, float *grad_logits, int ldg,
                                        int B, int R, int d, int h, int w, int sd, int sh, int sw, void *stream) {
  DG_REQUIRE(dc_ds_dims_ok(d, h, w, sd, sh, sw), DGTTA_ERR_BADARG, "region_loss_ds_bwd: bad dims %dx%dx%d strides %d,%d,%d", d, h, w,
             sd, sh, sw);
  return region_loss_bwd(logits, ldc, labels_full, table, L, ws, grad_scale, grad_scale_dev, grad_logits, ldg, B, R,
                         (int64_t)d * h * w, stream, dc_ds_labels(d, h, w, sd, sh, sw));
}
