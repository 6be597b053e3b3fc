// Shared declarations of the weight-gradient translation units (conv_wgrad.hip: host dispatch; conv_wgrad_ring.hip,
// conv_wgrad_rows.hip, conv_wgrad_flat.hip, conv_wgrad_s2.hip, convt_wgrad.hip, conv_wgrad_reduce.hip, head_wgrad.hip: kernels and
// their launchers): the kernels' by-value descriptors, the launch and output descriptors of the host chain (WgradLaunch, WgradOut)
// and the launchers that take them (each declared here, once; the defining file includes this header), the class tables
// (wgrad_single_class, wgrad_parity_classes) and the weight-gradient device helpers that more than one kernel file uses (the MFMA
// wrappers and tr_operand: gfx950.h).
// All kernels leave fp32 partial slabs [27 taps][32 ci][32 co], one per workgroup and channel-block pair; wgrad_reduce_launch
// sums them in a fixed order.
#pragma once
#include "conv_common.h"
#include <functional>
#include <type_traits>

namespace dgconv {
// Up to 8 independent classes per launch (blockIdx.z): operand offsets + tap mask per class, one slab set per class.
struct WgradClasses {
  int n;
  unsigned mask[8];
  long long xoff[8], yoff[8];
};
struct RealTaps {
  Taps t[8];
};
// tiles of tW x tH voxels of the dy lattice, D split into nsd ranges of DR slices; units = columns of the volume
struct WgradPlan {
  int tW, tH, nsd, DR, cibs, cobs;
  int64_t units;
};

// One weight-gradient launch as the host chain hands it down: the operands and their views (yv: the lattice the plan tiles),
// batch and channel counts, the storage type, the slab region and the stream.  Every launcher writes its slabs at ws.  Riders:
//   xkh != 0: x holds its 32-channel blocks as dense planes xkh elements apart - only conv3_wgrad_ring_launch reads that layout;
//   split_leg: one of the six launches of an fp32 weight gradient - wgrad_launch_classes keeps those off the flat kernel;
//   dry: no launch, conv3_wgrad_ring_launch only answers whether it would take the call (conv3_wgrad_blocked_ok).
struct WgradLaunch {
  const void *x;
  View xv;
  const void *dy;
  View yv;
  int B, Cin, Cout, dtype;
  void *ws;
  size_t ws_bytes;
  hipStream_t st;
  long long xkh = 0;
  bool split_leg = false;
  bool dry = false;
};
// where the slab reduction writes: dw[co * s_co + ci * s_ci + real_tap * s_tap] (+)=
struct WgradOut {
  float *dw;
  long long s_co, s_ci, s_tap;
  int accumulate;
};
// one fp32 operand of a split weight gradient: rows [B * D * H * W][ld] with C channels used
struct SplitOperand {
  const float *p;
  int ld, C, B, D, H, W;
};
}  // namespace dgconv

// slab region of a launch of plan p with ncls classes
static inline size_t wgrad_slab_bytes(const WgradPlan &p, int ncls) {
  return (size_t)ncls * p.units * p.cibs * p.cobs * 27 * 1024 * sizeof(float);
}
// do the one-pass 16-bit kernels (conv_wgrad_s2.hip, convT_wgrad_tr_kernel) take this launch under their single-class plan p?
static inline bool wgrad_onepass_ok(const WgradLaunch &L, const WgradPlan &p) {
  return L.Cout % 8 == 0 && L.xv.sw % 8 == 0 && L.yv.sw % 8 == 0 && !((uintptr_t)L.x & 15) && !((uintptr_t)L.dy & 15) &&
         L.xv.sw >= (L.Cin + 7) / 8 * 8 && L.ws_bytes >= wgrad_slab_bytes(p, 1) && p.units < (1ll << 31) && p.cibs * p.cobs <= 65535;
}

// ---------------------------------------------------------------------------------------------------- conv_wgrad.hip
// plan of a launch with ncls classes over tiles of tileW x tileH voxels (32 x 4: the stride-1 kernels; WT2::TWO x WT2::TH: the
// one-pass stride-2 and transposed-conv kernels)
WgradPlan wgrad_plan(int B, int Cin, int Cout, int D, int H, int W, int ncls, int tileW, int tileH);
size_t wgrad_classes_bytes(int B, int Cin, int Cout, int D, int H, int W, int ncls);
// class launch of the stride-1 kernels (the first that takes it: flat, ring, tr8, tr; fp32 or DGTTA_WGRAD_TR=0: mfma) + slab reduction
int wgrad_launch_classes(const WgradLaunch &L, const WgradOut &out, const WgradClasses &wc, const RealTaps &reals);
// fp32 operands as three bf16 planes each (exact three-term splits): plane size, and the driver of the six 16-bit launches.  It
// carves the planes out of ws behind slab_bytes, fills them and calls leg(x plane, its ld, dy plane, its ld, accumulate) for the
// products (0,0) (0,1) (1,0) (0,2) (1,1) (2,0), accumulating from the second on.  DGTTA_ERR_UNSUPPORTED, nothing written: the
// split does not apply (Cout % 8, DGTTA_WGRAD_F32_SPLIT=0, workspace without the planes) or the first leg refused
size_t wgrad_split_plane_bytes(int B, int C, int D, int H, int W);
typedef std::function<int(const bf16_t *x, int ldx, const bf16_t *dy, int lddy, int accumulate)> WgradSplitLeg;
int wgrad_f32_split(const SplitOperand &x, const SplitOperand &dy, void *ws, size_t ws_bytes, size_t slab_bytes, int accumulate,
                    hipStream_t st, const WgradSplitLeg &leg);

// ---------------------------------------------------------------------------------------------------- conv_wgrad_ring.hip
// persistent ring sweep of plain 16-bit launches; returns its slab count per channel-block pair (0: not taken, nothing launched)
int conv3_wgrad_ring_launch(const WgradLaunch &L, int *rc);

// ---------------------------------------------------------------------------------------------------- conv_wgrad_rows.hip
// stride-1 kernels; one slab per workgroup at slabs[(class, pair, blockIdx.x)] (tr / tr8: 16-bit storage only)
int conv3_wgrad_mfma_launch(const WgradLaunch &L, const WgradPlan &p, const WgradClasses &wc);
int conv3_wgrad_tr_launch(const WgradLaunch &L, const WgradPlan &p, const WgradClasses &wc, bool plain, int upw, int64_t nslab);
int conv3_wgrad_tr8_launch(const WgradLaunch &L, const WgradPlan &p, int upw, int64_t nslab);

// ---------------------------------------------------------------------------------------------------- conv_wgrad_flat.hip
// planes of W <= 16; returns the number of slabs per channel-block pair (0: shape not taken)
int64_t wgrad_flat_launch(const WgradLaunch &L, int *rc);

// ---------------------------------------------------------------------------------------------------- conv_wgrad_s2.hip
// one-pass stride-2 kernels (L.xv: x at full resolution); two_blocks: the 8-wave kernel that shares the x tile between two
// output-channel blocks
int conv3_wgrad_s2_launch(const WgradLaunch &L, const WgradPlan &p, bool two_blocks);

// ---------------------------------------------------------------------------------------------------- conv_wgrad_reduce.hip
// out (+)= sum over the nslab slabs (at L.ws) of every pair, fixed order; ncls slab sets with the tap tables reals.t[0 .. ncls).  The
// one table of a single-class launch is offered to the dense-layout kernel
int wgrad_reduce_launch(const WgradLaunch &L, const WgradOut &out, const WgradPlan &p, int ncls, int64_t nslab, const RealTaps &reals);

namespace {

// one class over the whole operands (offsets 0) with the virtual taps of tapmask; *reals: its real-tap table
inline WgradClasses wgrad_single_class(unsigned tapmask, const Taps &real, RealTaps *reals) {
  WgradClasses wc{};
  wc.n = 1;
  wc.mask[0] = tapmask;
  reals->t[0] = real;
  return wc;
}

// Weight gradient of a [kd, 3, 3] conv with strides (sd, sh, sw) in {1, 2}^3 as stride-1 problems over dy's lattice (the counterpart
// of dgrad_parity_classes, conv_common.h):  dW[co][ci][t] = sum_{b,vo} dy[vo][co] x[s vo + t - pad][ci] per axis.  A strided axis
// splits x into its two parity lattices: parity p at virtual offset u (-1, 0, +1) carries the real tap t = s u + p + pad where
// 0 <= t < k (stride 1: t = u + pad; kd = 3, stride 2: parity 0 carries tap 1, parity 1 taps 0 and 2).  One class per parity
// combination that carries a tap (1 to 8, parities flattened in D, H, W order), its mask exactly the virtual taps with a real tap
// (*reals) - each real tap belongs to one class.  *xv: the lattices' common view (steps s, extent of dy, batch stride of the dense
// volume); strided axes need even input extents.
inline WgradClasses wgrad_parity_classes(const ConvProblem &P, int ldx, RealTaps *reals, View *xv) {
  const int ks[3] = {P.kd, 3, 3}, ss[3] = {P.sd, P.sh, P.sw};
  WgradClasses wc{};
  *xv = dense_view(1, P.Di, P.Hi, P.Wi, ldx);
  for (int c = 0; c < P.noff(); ++c) {
    const Parity par = class_parity(c, P.sd, P.sh, P.sw);
    unsigned mask = 0;
    Taps rt;
    for (int t = 0; t < 27; ++t) {
      const int u[3] = {t / 9 - 1, (t / 3) % 3 - 1, t % 3 - 1};
      int real[3];
      bool ok = true;
      for (int a = 0; a < 3; ++a) {
        real[a] = ss[a] * u[a] + par.p[a] + ks[a] / 2;
        ok = ok && real[a] >= 0 && real[a] < ks[a];
      }
      rt.wt[t] = ok ? (signed char)(real[0] * 9 + real[1] * 3 + real[2]) : (signed char)-1;
      if (ok) mask |= 1u << t;
    }
    if (!mask) continue;            // kd = 1 along a strided D: the odd planes carry no tap
    wc.xoff[wc.n] = par.p[0] * xv->sd + par.p[1] * xv->sh + par.p[2] * xv->sw;
    wc.mask[wc.n] = mask;
    reals->t[wc.n] = rt;
    ++wc.n;
  }
  xv->sd *= P.sd, xv->sh *= P.sh, xv->sw *= P.sw;
  xv->D = P.Do(), xv->H = P.Ho(), xv->W = P.Wo();
  return wc;
}

// Workgroups are dispatched round robin over the 8 XCDs (each with its own L2), units are columns of the volume whose x
// tiles overlap their H neighbours' by the halo rows: give every XCD a CONTIGUOUS range of units, so that the halo is
// fetched from HBM by one L2 instead of two (DGTTA_WGRAD_XCD=0: units in dispatch order)
__device__ __forceinline__ int xcd_unit(int xcd_map) {
  const int i = blockIdx.x, n = gridDim.x;
  if (!xcd_map || (n & 7)) return i;
  return (i & 7) * (n >> 3) + (i >> 3);
}

template <typename T>
struct WG {
  static constexpr int EPV = Elem<T>::EPV;
  static constexpr int GC = 32 / EPV;            // channel groups (of EPV channels) per 32-channel tile
  static constexpr int NCH_Y = 32 / EPV;         // voxel runs per dy row
  static constexpr int NCH_X = 32 / EPV + 1;     // voxel runs per x row; run c covers wx = EPV*c - 1 .. EPV*c + EPV - 2
  static constexpr int TH = 4, XR = TH + 2;
  static constexpr int XSLOT = XR * NCH_X * 32;  // uint4 per x slice
  static constexpr int YSLOT = TH * NCH_Y * 32;
  static constexpr int NUX = XR * NCH_X * GC, NUY = TH * NCH_Y * GC, NU = NUX + NUY;
  static constexpr int ROUNDS = (NU + 255) / 256;
  static constexpr size_t LDS_BYTES = (size_t)(4 * XSLOT + 2 * YSLOT) * 16;
  static constexpr int NSTEP = 32 / (4 * EPV);   // MFMA k-steps per voxel row (bf16 1, fp32 2)
  // LDS slot (in uint4) of channel c (0..31) of voxel run `run` in row `row`.  Within a channel group the EPV slots are
  // XOR-swizzled so that the 8 lanes of a ds_write_b128 group (which differ in channel group / run parity and all write
  // the same in-group channel j) hit 8 different 16-byte bank slots; readers apply the same map (still one distinct
  // slot per lane of a 16-lane read group).
  __device__ static __forceinline__ int slot(int row, int run, int nruns, int c) {
    const int cg = c / EPV, j = c % EPV;
    const int sw = (EPV == 8) ? ((cg | ((run & 1) << 2)) & 7) : ((cg >> 1) & 3);
    return (row * nruns + run) * 32 + cg * EPV + (j ^ sw);
  }
};

template <typename T>
__device__ __forceinline__ void transpose_unit(const uint4 *in, uint4 *out);
template <>
__device__ __forceinline__ void transpose_unit<float>(const uint4 *in, uint4 *out) {   // 4 voxels x 4 channels
  out[0] = make_uint4(in[0].x, in[1].x, in[2].x, in[3].x);
  out[1] = make_uint4(in[0].y, in[1].y, in[2].y, in[3].y);
  out[2] = make_uint4(in[0].z, in[1].z, in[2].z, in[3].z);
  out[3] = make_uint4(in[0].w, in[1].w, in[2].w, in[3].w);
}
__device__ __forceinline__ unsigned pack_lo(unsigned a, unsigned b) { return (a & 0xffffu) | (b << 16); }
__device__ __forceinline__ unsigned pack_hi(unsigned a, unsigned b) { return (a >> 16) | (b & 0xffff0000u); }
template <>
__device__ __forceinline__ void transpose_unit<bf16_t>(const uint4 *in, uint4 *out) {  // 8 voxels x 8 channels
#define TR_PAIR(c, fld)                                                                                      \
  out[c] = make_uint4(pack_lo(in[0].fld, in[1].fld), pack_lo(in[2].fld, in[3].fld), pack_lo(in[4].fld, in[5].fld), \
                      pack_lo(in[6].fld, in[7].fld));                                                        \
  out[c + 1] = make_uint4(pack_hi(in[0].fld, in[1].fld), pack_hi(in[2].fld, in[3].fld),                       \
                          pack_hi(in[4].fld, in[5].fld), pack_hi(in[6].fld, in[7].fld));
  TR_PAIR(0, x) TR_PAIR(2, y) TR_PAIR(4, z) TR_PAIR(6, w)
#undef TR_PAIR
}

template <>
__device__ __forceinline__ void transpose_unit<f16_t>(const uint4 *in, uint4 *out) { transpose_unit<bf16_t>(in, out); }

// A operand for tap column kw from the aligned run `c` and the next run's first dwords (e0, e1)
template <typename T>
__device__ __forceinline__ uint4 shift_run(const uint4 &c, unsigned e0, unsigned e1, int kw);
template <>
__device__ __forceinline__ uint4 shift_run<bf16_t>(const uint4 &c, unsigned e0, unsigned, int kw) {
  if (kw == 0) return c;
  if (kw == 2) return make_uint4(c.y, c.z, c.w, e0);
  return make_uint4((c.x >> 16) | (c.y << 16), (c.y >> 16) | (c.z << 16), (c.z >> 16) | (c.w << 16),
                    (c.w >> 16) | (e0 << 16));
}
template <>
__device__ __forceinline__ uint4 shift_run<f16_t>(const uint4 &c, unsigned e0, unsigned e1, int kw) {
  return shift_run<bf16_t>(c, e0, e1, kw);          // pure 16-bit lane moves
}
template <>
__device__ __forceinline__ uint4 shift_run<float>(const uint4 &c, unsigned e0, unsigned e1, int kw) {
  if (kw == 0) return c;
  if (kw == 1) return make_uint4(c.y, c.z, c.w, e0);
  return make_uint4(c.z, c.w, e0, e1);
}

// LDS geometry of the kernels with hardware-transposed operand reads (conv3_wgrad_tr_kernel and its 8-wave variant): tiles of
// 4 rows x 32 voxels, slices voxel-major [row][voxel][32 channels = 64 B], a ring of 4 x slices (halo of 1) and 2 dy slices
struct WT {
  static constexpr int TH = 4, XR = TH + 2;
  static constexpr int XW = 36;                         // voxels per x row in LDS (34 used)
  static constexpr int X_ROW_B = XW * 64, X_SLICE_B = XR * X_ROW_B;
  static constexpr int Y_ROW_B = 32 * 64, Y_SLICE_B = TH * Y_ROW_B;
  static constexpr int LDS_BYTES = 4 * X_SLICE_B + 2 * Y_SLICE_B;
  static constexpr int NPX = XR * 3, NPY = TH * 2, NP = NPX + NPY;      // DMA pieces per slice
};

// tile geometry of the one-pass stride-2 kernels (conv_wgrad_s2.hip); the transposed-conv kernel tiles its input lattice alike
struct WT2 {
  static constexpr int TH = 2, TWO = 16;                // output rows / voxels per tile
  static constexpr int XR = 2 * TH + 1, XW = 36;        // x rows per slice, voxels per x row in LDS (33 used)
  static constexpr int X_ROW_B = XW * 64, X_SLICE_B = XR * X_ROW_B;
  static constexpr int Y_ROW_B = TWO * 64, Y_SLICE_B = TH * Y_ROW_B;
  static constexpr int NXS = 5;                         // x ring slots
  static constexpr int LDS_BYTES = NXS * X_SLICE_B + 2 * Y_SLICE_B;
  static constexpr int NPX1 = XR * 3;                   // DMA pieces per x slice (16 + 16 + 1 voxels per row)
};

}  // namespace
