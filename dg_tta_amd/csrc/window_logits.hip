// Sliding-window inference in LOGIT space: the Gaussian-weighted accumulation of a window's logits into the volume, plain
// (window_accumulate_kernel, at the end of the file) and fused with the segmentation head (head_accumulate*_kernel).
// window_features.hip is the same stage in FEATURE space (the head runs once per voxel at the end, fused with the argmax).
// Every kernel takes the window's place in the volume as one WindowPlace (window_api.h: the descriptor, its host checks and the
// index helpers, shared with window_features.hip); the head kernels are launched through head_accumulate_launch<T, ACC, MIR, FMA>.
//
// Segmentation head fused with the Gaussian window accumulation (round 3, BASELINE config 3): a window's logits over ALL
// classes ([3P] nnU-Net predict_sliding_window_return_logits via dg_tta/tta/nnunet_utils.py:116-125) are 880 MB at
// 128^3 x 105 fp32 - written by the head and read back by window_accumulate_kernel.  Here a workgroup takes 64 consecutive
// voxels of a window row, evaluates all classes from the 64-byte feature rows (same FMA chain over the 32 channels and bias
// add as head_fwd_lds_kernel: identical logits), scales them by the voxel's Gaussian weight into an LDS tile and adds the
// tile to the accumulator as one contiguous run (the window row is contiguous in the volume along its last axis).
// Round 4: the run's accumulator values (27 per thread) are requested BEFORE the logits are evaluated and held in
// registers - the round-3 kernel read them one dependent load at a time after the barrier (a workgroup then spends ~27
// memory round trips per tile: 0.79 ms per window where the HBM traffic of 1.9 GB asks for 0.35 ms).  ACC: storage type of
// the accumulator - float, or f16_t (what nnU-Net's predictor keeps, 2.2.1 `predicted_logits` dtype torch.half); the sum is
// formed in fp32 either way and rounded once per window on the way back.
#include "gfx950.h"
#include "window_api.h"

namespace {

constexpr int HA_CIN = 32, HA_MAXC = 112;      // input channels of the head, most classes
constexpr int HA_RUN = (64 * HA_MAXC + 255) / 256;      // accumulator values per thread and tile (fp32 storage)
constexpr int HA_RUN2 = (64 * HA_MAXC / 2 + 1 + 255) / 256;   // 32-bit words per thread and tile (fp16 storage)

// One tile's run of the accumulator (n values from ap) held in registers between the early loads and the late stores.
// fp32 storage: thread t owns values t, t + 256, ...  fp16 storage: the run is addressed as 32-bit words from the aligned
// address at or below ap (a run starts on an odd half when its voxel offset x 105 classes is odd); a word that straddles
// the run's first or last half is accessed as that one half only - the other half belongs to the neighbouring run, which
// another workgroup may be updating.
template <typename ACC>
struct AccRun;
template <>
struct AccRun<float> {
  float r[HA_RUN];
  __device__ __forceinline__ void load(const float *ap, int n) {
#pragma unroll
    for (int j = 0; j < HA_RUN; ++j) {
      const int i = (int)threadIdx.x + 256 * j;
      r[j] = i < n ? ap[i] : 0.f;
    }
  }
  __device__ __forceinline__ void add_store(float *ap, int n, const float *tile, int t = (int)threadIdx.x) {      // t: thread index
#pragma unroll
    for (int j = 0; j < HA_RUN; ++j) {
      const int i = t + 256 * j;
      if (i < n) ap[i] = r[j] + tile[i];
    }
  }
};
template <>
struct AccRun<f16_t> {
  unsigned r[HA_RUN2];
  __device__ __forceinline__ void load(const f16_t *ap, int n) {
    const int h0 = (int)(((uintptr_t)ap >> 1) & 1);
    const unsigned short *hp = reinterpret_cast<const unsigned short *>(ap);
#pragma unroll
    for (int j = 0; j < HA_RUN2; ++j) {
      const int e0 = 2 * ((int)threadIdx.x + 256 * j) - h0;        // first half of the word, relative to ap
      const bool v0 = e0 >= 0 && e0 < n, v1 = e0 + 1 < n;
      unsigned v = 0;
      if (v0 && v1) v = *reinterpret_cast<const unsigned *>(hp + e0);
      else if (v0) v = hp[e0];
      else if (v1) v = (unsigned)hp[e0 + 1] << 16;
      r[j] = v;
    }
  }
  __device__ __forceinline__ void add_store(f16_t *ap, int n, const float *tile, int t = (int)threadIdx.x) {
    const int h0 = (int)(((uintptr_t)ap >> 1) & 1);
    unsigned short *hp = reinterpret_cast<unsigned short *>(ap);
#pragma unroll
    for (int j = 0; j < HA_RUN2; ++j) {
      const int e0 = 2 * (t + 256 * j) - h0;
      const bool v0 = e0 >= 0 && e0 < n, v1 = e0 + 1 < n;
      const unsigned short lo = v0 ? f32_to_f16(f16_to_f32((unsigned short)(r[j] & 0xffffu)) + tile[e0]) : (unsigned short)0;
      const unsigned short hi = v1 ? f32_to_f16(f16_to_f32((unsigned short)(r[j] >> 16)) + tile[e0 + 1]) : (unsigned short)0;
      if (v0 && v1) *reinterpret_cast<unsigned *>(hp + e0) = (unsigned)lo | ((unsigned)hi << 16);
      else if (v0) hp[e0] = lo;
      else if (v1) hp[e0 + 1] = hi;
    }
  }
};

// MIR (both head kernels): a mirrored pass of nnU-Net's test-time mirroring - the feature row of a destination voxel is read at the
// mirrored voxel of the window (wm_source); the destination, its Gaussian weight and everything after the load are the unmirrored ones.
template <typename T, typename ACC, bool MIR>
__global__ __launch_bounds__(256) void head_accumulate_fma_kernel(const T *__restrict__ z, const float *__restrict__ w,
                                                              const float *__restrict__ bias, const float *__restrict__ gauss,
                                                              ACC *__restrict__ acc, float *__restrict__ nsum, int C, WindowPlace wp) {
  extern __shared__ float hsm[];
  float *tile = hsm;                        // [64][C]
  // the head's weights are the same for every lane of a wave (a wave = 64 voxels x one class at a time): they are read
  // through the scalar cache (13 KB at 105 classes; constant address space + a wave-uniform class index) and enter the
  // FMAs as scalar operands.  Round 3 staged them in LDS: a 16-byte broadcast read still moves 1 KB per wave, and 216 of
  // them per tile and wave kept the LDS pipe busier than HBM (0.42 of the 0.79 ms per window)
  typedef const __attribute__((address_space(4))) float *cptr_t;
  const cptr_t wc = (cptr_t)w, bc = (cptr_t)bias;
  const int PH = wp.PH, PW = wp.PW;
  const int runs = (PW + 63) >> 6, nblk = wp.PD * PH * runs;
  const int vox = threadIdx.x & 63;
  const int grp = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));       // 4 class groups per voxel
  for (int blk = blockIdx.x; blk < nblk; blk += gridDim.x) {
    const int row = blk / runs, pw0 = (blk % runs) * 64;
    const int pd = row / PH, ph = row % PH;
    const int nv = PW - pw0 < 64 ? PW - pw0 : 64;
    const int64_t p = wp_window(wp, pd, ph, pw0 + vox);           // voxel inside the window
    const int64_t vg = wp_volume(wp, pd, ph, pw0);
    ACC *ap = acc + vg * C;
    const int n = nv * C;
    AccRun<ACC> run;
    run.load(ap, n);
    float ns = 0.f, gs = 0.f;
    if (nsum && (int)threadIdx.x < nv) {
      ns = nsum[vg + threadIdx.x];
      gs = gauss[wp_window(wp, pd, ph, pw0 + (int)threadIdx.x)];
    }
    __syncthreads();                                              // previous tile consumed
    if (vox < nv) {
      float xr[HA_CIN];
      const int64_t ps = wp_source<MIR>(wp, pd, ph, pw0 + vox);
      const uint4 *zr = reinterpret_cast<const uint4 *>(z + ps * HA_CIN);
#pragma unroll
      for (int g = 0; g < 4; ++g) unpack16<T>(zr[g], xr + 8 * g);
      const float gq = gauss[p];
      for (int k = grp; k < C; k += 4) {
        float a = 0.f;
#pragma unroll
        for (int ci = 0; ci < HA_CIN; ++ci) a = __builtin_fmaf(xr[ci], wc[k * HA_CIN + ci], a);
        tile[vox * C + k] = (a + bc[k]) * gq;
      }
    }
    __syncthreads();
    // the stores' indices are rebuilt from a laundered thread id: shared with the loads above, the compiler keeps the run's 28
    // offsets and lane masks live across the FMA chain (26 registers more) and waits for each store before the next
    int ts = (int)threadIdx.x;
    asm volatile("" : "+v"(ts));
    run.add_store(ap, n, tile, ts);
    if (nsum && (int)threadIdx.x < nv) nsum[vg + threadIdx.x] = ns + gs;
  }
}

// The same on the matrix cores (round 4, the default; DGTTA_HA_MFMA=0 selects the FMA chain above).  Timed alone on one
// 128^3 x 105 window the FMA chain needs 0.31 ms for the logits and the accumulator traffic 0.35 ms (fp32) / 0.20 ms (fp16):
// the vector ALU, not HBM, sets the pace.  Here a wave takes 16 voxels: their feature rows are the B operand of
// v_mfma_f32_16x16x32 as they lie in memory (lane = voxel x 8-channel chunk, one 16-byte load), the head's weights are the A
// operand, held in registers for the life of the workgroup, and D[class][voxel] leaves 4 consecutive classes of one voxel in
// each lane.  The weights stay fp32-exact: every fp32 weight is split into three 16-bit terms (hi + mid + lo; 3 x 8 bits of
// bf16 significand = the 24 of fp32, exact; fp16 terms carry 3 x 11 bits but stop at 2^-24 in magnitude), 16-bit activations
// times 16-bit terms are exact in the fp32 accumulator, so the logits differ from the FMA chain by the order of the 32-term
// sum only (tests: <= a few 1e-7 of the row's magnitude, same labels outside float ties).
static_assert(HA_MAXC <= 8 * 16, "a wave takes class groups wv and wv + 4: at most 8 groups of 16 classes");
template <typename T, typename ACC, bool MIR>
__global__ __launch_bounds__(256) void head_accumulate_kernel(const T *__restrict__ z, const float *__restrict__ w,
                                                              const float *__restrict__ bias, const float *__restrict__ gauss,
                                                              ACC *__restrict__ acc, float *__restrict__ nsum, int C, WindowPlace wp) {
  extern __shared__ float hsm[];
  float *tile = hsm;                        // [64][C]
  const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const int ln = lane & 15, lq = lane >> 4;
  // wave wv evaluates class groups wv and wv + 4 for all 64 voxels of a tile (a wave per voxel group would hold all 7
  // groups x 3 terms = 84 registers of weights and run at 2 waves per SIMD; here it is 24, at 4 waves per SIMD - the
  // accumulator loads in flight are what keeps HBM busy).  A operand: lane = (class ln of the group, channels 8 lq .. + 7)
  uint4 wa[2][3];
  float bq[2][4];
#pragma unroll
  for (int j = 0; j < 2; ++j) {
    const int cg = wv + 4 * j;
    const int m = cg * 16 + ln;
    unsigned short t[3][8];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
      const float x = m < C ? w[m * HA_CIN + lq * 8 + i] : 0.f;
      const unsigned short h = f32_to_16<T>(x);
      const float r1 = x - from16<T>(h);
      const unsigned short mid = f32_to_16<T>(r1);
      const float r2 = r1 - from16<T>(mid);
      t[0][i] = h;
      t[1][i] = mid;
      t[2][i] = f32_to_16<T>(r2);
    }
#pragma unroll
    for (int q = 0; q < 3; ++q)
      wa[j][q] = make_uint4((unsigned)t[q][0] | ((unsigned)t[q][1] << 16), (unsigned)t[q][2] | ((unsigned)t[q][3] << 16),
                            (unsigned)t[q][4] | ((unsigned)t[q][5] << 16), (unsigned)t[q][6] | ((unsigned)t[q][7] << 16));
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int k = cg * 16 + lq * 4 + r;
      bq[j][r] = k < C ? bias[k] : 0.f;
    }
  }
  const int PH = wp.PH, PW = wp.PW;
  const int runs = (PW + 63) >> 6, nblk = wp.PD * PH * runs;
  // Software pipeline over the workgroup's tiles: the accumulator run and the feature rows of tile t + 1 are requested
  // before tile t is evaluated, so that every workgroup keeps loads in flight while its waves are in the MFMA / LDS phase
  // (loads return in order: a wave that asked for its 27 accumulator values first and its feature rows second cannot start
  // on the logits before the whole run has arrived - without the pipeline the phases of a workgroup run strictly one after
  // the other, and the fp32 accumulator, whose 27 registers per thread cost a wave of occupancy, ran at 2.6-3.2 TB/s)
  struct TilePos {
    int nv, n;
    int64_t prow, vg;
    int pd, ph, pw0;      // (read by the mirrored source index only)
  };
  auto tile_pos = [&](int blk) {
    const int row = blk / runs, pw0 = (blk % runs) * 64;
    const int pd = row / PH, ph = row % PH;
    TilePos t;
    t.nv = PW - pw0 < 64 ? PW - pw0 : 64;
    t.n = t.nv * C;
    t.prow = wp_window(wp, pd, ph, pw0);                          // first voxel of the run inside the window
    t.vg = wp_volume(wp, pd, ph, pw0);                            // ... and inside the volume
    t.pd = pd, t.ph = ph, t.pw0 = pw0;
    return t;
  };
  AccRun<ACC> run, run_n;
  uint4 zb[4], zb_n[4];                                           // B operand: lane = (voxel 16 vgp + ln, channels 8 lq .. + 7)
  float gq[4], gq_n[4];
  float ns = 0.f, gs = 0.f, ns_n = 0.f, gs_n = 0.f;
  auto fetch = [&](const TilePos &t, AccRun<ACC> &rn, uint4 *zz, float *gg, float &nss, float &gss) {
    rn.load(acc + t.vg * C, t.n);
    nss = 0.f;
    gss = 0.f;
    if (nsum && (int)threadIdx.x < t.nv) {
      nss = nsum[t.vg + threadIdx.x];
      gss = gauss[t.prow + threadIdx.x];
    }
#pragma unroll
    for (int vgp = 0; vgp < 4; ++vgp) {
      const int vox = vgp * 16 + ln;
      zz[vgp] = make_uint4(0u, 0u, 0u, 0u);
      gg[vgp] = 0.f;
      if (vox < t.nv) {
        const int64_t ps = MIR ? wp_source<true>(wp, t.pd, t.ph, t.pw0 + vox) : t.prow + vox;
        zz[vgp] = *reinterpret_cast<const uint4 *>(z + ps * HA_CIN + lq * 8);
        gg[vgp] = gauss[t.prow + vox];
      }
    }
  };
  int blk = blockIdx.x;
  if (blk < nblk) fetch(tile_pos(blk), run, zb, gq, ns, gs);
  for (; blk < nblk; blk += gridDim.x) {
    const TilePos t = tile_pos(blk);
    const bool more = blk + (int)gridDim.x < nblk;
    if (more) fetch(tile_pos(blk + gridDim.x), run_n, zb_n, gq_n, ns_n, gs_n);
    __syncthreads();                                              // previous tile consumed
#pragma unroll
    for (int j = 0; j < 2; ++j) {
      const int cg = wv + 4 * j;
      if (cg * 16 < C) {                                        // wave-uniform
#pragma unroll
        for (int vgp = 0; vgp < 4; ++vgp) {
          f32x4_t d = {0.f, 0.f, 0.f, 0.f};
          mfma16<T>(wa[j][2], zb[vgp], d);
          mfma16<T>(wa[j][1], zb[vgp], d);
          mfma16<T>(wa[j][0], zb[vgp], d);
          const int vox = vgp * 16 + ln;
          if (vox < t.nv) {
#pragma unroll
            for (int r = 0; r < 4; ++r) {
              const int k = cg * 16 + lq * 4 + r;
              if (k < C) tile[vox * C + k] = (d[r] + bq[j][r]) * gq[vgp];
            }
          }
        }
      }
    }
    __syncthreads();
    run.add_store(acc + t.vg * C, t.n, tile);
    if (nsum && (int)threadIdx.x < t.nv) nsum[t.vg + threadIdx.x] = ns + gs;
    if (more) {
      run = run_n;
#pragma unroll
      for (int vgp = 0; vgp < 4; ++vgp) {
        zb[vgp] = zb_n[vgp];
        gq[vgp] = gq_n[vgp];
      }
      ns = ns_n;
      gs = gs_n;
    }
  }
}

}  // namespace

// One launch of a head kernel as the entry points hand it down; the templates below pick the instantiation from the storage
// types, the mirror mask and DGTTA_HA_MFMA
struct HeadCall {
  const void *z;
  const float *w, *bias, *gauss;
  void *acc;
  float *nsum;
  int C;
  WindowPlace wp;
  int acc_dtype;
  bool fma;
  dim3 grid;
  size_t lds;
  hipStream_t st;
};

template <typename T, typename ACC, bool MIR, bool FMA>
static hipError_t head_accumulate_launch(const HeadCall &c) {
  static DynLdsOnce once;      // one per instantiation: one per kernel
  const auto kernel = FMA ? head_accumulate_fma_kernel<T, ACC, MIR> : head_accumulate_kernel<T, ACC, MIR>;
  const hipError_t e = ensure_dyn_lds(once, (const void *)kernel, (int)c.lds);
  if (e == hipSuccess)
    hipLaunchKernelGGL(kernel, c.grid, dim3(256), c.lds, c.st, (const T *)c.z, c.w, c.bias, c.gauss, (ACC *)c.acc, c.nsum, c.C, c.wp);
  return e;
}
template <typename T, typename ACC, bool MIR>
static hipError_t head_accumulate_launch_k(const HeadCall &c) {
  return c.fma ? head_accumulate_launch<T, ACC, MIR, true>(c) : head_accumulate_launch<T, ACC, MIR, false>(c);
}
template <typename T>
static hipError_t head_accumulate_launch_t(const HeadCall &c) {
  if (c.acc_dtype == DGTTA_F16) return head_accumulate_launch_k<T, f16_t, false>(c);      // (never mirrored: window_acc_check)
  return c.wp.mirror ? head_accumulate_launch_k<T, float, true>(c) : head_accumulate_launch_k<T, float, false>(c);
}

static int seghead_window_accumulate_impl(const char *who, const void *z, const float *w, const float *bias, const float *gauss, void *acc,
                                          float *nsum, int Cin, int C, const WindowPlace &wp, int dtype, int acc_dtype, void *stream) {
  DG_REQUIRE(z && w && bias && gauss && acc, DGTTA_ERR_BADARG, "%s: null pointer", who);
  DG_REQUIRE(Cin == HA_CIN && C > 0 && C <= HA_MAXC && (dtype == DGTTA_BF16 || dtype == DGTTA_F16), DGTTA_ERR_UNSUPPORTED,
             "%s: built for 32 input channels, up to %d classes, 16-bit storage", who, HA_MAXC);
  if (const int rc = window_acc_check(who, acc_dtype, wp.mirror)) return rc;
  if (const int rc = window_place_check(who, wp)) return rc;
  DG_REQUIRE(((uintptr_t)z & 15) == 0, DGTTA_ERR_BADARG, "%s: unaligned feature map", who);
  const int64_t nblk = (int64_t)wp.PD * wp.PH * cdiv(wp.PW, 64);
  DG_REQUIRE(nblk < (1ll << 31), DGTTA_ERR_UNSUPPORTED, "%s: too many rows", who);
  const HeadCall c = {z, w, bias, gauss, acc, nsum, C, wp, acc_dtype, dgtta_switches().ha_mfma == '0',
                      dim3((unsigned)(nblk < 2048 ? nblk : 2048)), (size_t)64 * C * sizeof(float), (hipStream_t)stream};
  DG_REQUIRE((dtype == DGTTA_BF16 ? head_accumulate_launch_t<bf16_t>(c) : head_accumulate_launch_t<f16_t>(c)) == hipSuccess,
             DGTTA_ERR_LAUNCH, "%s: cannot raise the dynamic LDS limit", who);
  DG_CHECK_LAUNCH("head_accumulate_kernel");
  return DGTTA_OK;
}

extern "C" int dgtta_seghead_window_accumulate_t(const void *z, const float *w, const float *bias, const float *gauss, void *acc,
                                                 float *nsum, int Cin, int C, int PD, int PH, int PW, int X, int Y, int Z, int x0,
                                                 int y0, int z0, int dtype, int acc_dtype, void *stream) {
  return seghead_window_accumulate_impl("seghead_window_accumulate", z, w, bias, gauss, acc, nsum, Cin, C,
                                        {PD, PH, PW, X, Y, Z, x0, y0, z0, 0}, dtype, acc_dtype, stream);
}

// The logits-space forms of a mirrored pass: fp32 accumulators only (eight passes per window at Gaussian weight 10 leave no headroom
// in half).
extern "C" int dgtta_seghead_window_accumulate_mirror_t(const void *z, const float *w, const float *bias, const float *gauss, void *acc,
                                                        float *nsum, int Cin, int C, int PD, int PH, int PW, int X, int Y, int Z, int x0,
                                                        int y0, int z0, int dtype, int acc_dtype, int mirror, void *stream) {
  DG_REQUIRE(acc_dtype == DGTTA_F32, DGTTA_ERR_UNSUPPORTED, "seghead_window_accumulate_mirror: the accumulator is fp32 (acc_dtype %d)",
             acc_dtype);
  return seghead_window_accumulate_impl("seghead_window_accumulate_mirror", z, w, bias, gauss, acc, nsum, Cin, C,
                                        {PD, PH, PW, X, Y, Z, x0, y0, z0, mirror}, dtype, acc_dtype, stream);
}

extern "C" int dgtta_seghead_window_accumulate(const void *z, const float *w, const float *bias, const float *gauss, float *acc,
                                               float *nsum, int Cin, int C, int PD, int PH, int PW, int X, int Y, int Z, int x0,
                                               int y0, int z0, int dtype, void *stream) {
  return dgtta_seghead_window_accumulate_t(z, w, bias, gauss, acc, nsum, Cin, C, PD, PH, PW, X, Y, Z, x0, y0, z0, dtype, DGTTA_F32,
                                           stream);
}

// ---------------------------------------------------------------------------------------------------------------------
// Gaussian-weighted sliding-window accumulation (post-TTA ensemble inference; nnU-Net's
// predict_sliding_window_return_logits [3P nnunetv2==2.2.1], reached from dg_tta/tta/nnunet_utils.py:116-125,208-230):
//   acc[v0 + p][c] += patch[p][c] * gauss[p];   nsum[v0 + p] += gauss[p]        (voxel-major fp32 accumulators)
// One lane per (patch voxel, channel): rows of C floats are contiguous, windows overlap only between launches.
namespace {
template <typename ACC, bool MIR>
__global__ void window_accumulate_kernel(const float *__restrict__ patch, const float *__restrict__ gauss,
                                         ACC *__restrict__ acc, float *__restrict__ nsum, int C, WindowPlace wp, int64_t total) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int c = (int)(i % C);
    const int64_t p = i / C;
    const WindowVoxel s = wp_voxel(p, wp.PH, wp.PW);
    const int64_t v = wp_volume(wp, s.pd, s.ph, s.pw);
    const float g = gauss[p];
    const int64_t is = MIR ? wp_source<true>(wp, s.pd, s.ph, s.pw) * C + c : i;      // the mirrored voxel's row of C logits
    st_f<ACC>(acc + v * C + c, ld_f<ACC>(acc + v * C + c) + patch[is] * g);
    if (c == 0 && nsum) nsum[v] += g;
  }
}
}  // namespace

static int window_accumulate_impl(const char *who, const float *patch, const float *gauss, void *acc, float *nsum, int C, const WindowPlace &wp,
                                  int acc_dtype, void *stream) {
  DG_REQUIRE(patch && gauss && acc, DGTTA_ERR_BADARG, "%s: null pointer", who);
  if (const int rc = window_place_check(who, wp, C > 0)) return rc;
  if (const int rc = window_acc_check(who, acc_dtype, wp.mirror)) return rc;
  const int64_t total = (int64_t)wp.PD * wp.PH * wp.PW * C;
  const auto launch = [&](auto kernel, auto *a) {
    hipLaunchKernelGGL(kernel, dim3(grid_for(total)), dim3(256), 0, (hipStream_t)stream, patch, gauss, a, nsum, C, wp, total);
  };
  if (acc_dtype == DGTTA_F16) launch(window_accumulate_kernel<f16_t, false>, (f16_t *)acc);
  else if (wp.mirror) launch(window_accumulate_kernel<float, true>, (float *)acc);
  else launch(window_accumulate_kernel<float, false>, (float *)acc);
  DG_CHECK_LAUNCH("window_accumulate_kernel");
  return DGTTA_OK;
}

extern "C" int dgtta_window_accumulate_t(const float *patch, const float *gauss, void *acc, float *nsum, int C, int PD, int PH,
                                         int PW, int X, int Y, int Z, int x0, int y0, int z0, int acc_dtype, void *stream) {
  return window_accumulate_impl("window_accumulate", patch, gauss, acc, nsum, C, {PD, PH, PW, X, Y, Z, x0, y0, z0, 0}, acc_dtype, stream);
}

extern "C" int dgtta_window_accumulate_mirror_t(const float *patch, const float *gauss, void *acc, float *nsum, int C, int PD, int PH,
                                                int PW, int X, int Y, int Z, int x0, int y0, int z0, int acc_dtype, int mirror,
                                                void *stream) {
  DG_REQUIRE(acc_dtype == DGTTA_F32, DGTTA_ERR_UNSUPPORTED, "window_accumulate_mirror: the accumulator is fp32 (acc_dtype %d)", acc_dtype);
  return window_accumulate_impl("window_accumulate_mirror", patch, gauss, acc, nsum, C, {PD, PH, PW, X, Y, Z, x0, y0, z0, mirror}, acc_dtype,
                                stream);
}

extern "C" int dgtta_window_accumulate(const float *patch, const float *gauss, float *acc, float *nsum, int C, int PD, int PH,
                                       int PW, int X, int Y, int Z, int x0, int y0, int z0, void *stream) {
  return dgtta_window_accumulate_t(patch, gauss, acc, nsum, C, PD, PH, PW, X, Y, Z, x0, y0, z0, DGTTA_F32, stream);
}
