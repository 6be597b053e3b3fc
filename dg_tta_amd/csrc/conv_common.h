// Shared declarations of the MFMA convolution translation units (conv_mfma.hip, conv_rows.hip, conv_ring.hip, conv_s2.hip,
// convt_gemm.hip, conv_aniso.hip and, through conv_wgrad_common.h, the weight-gradient units):
// operand descriptors and views, the launch descriptor of the forward / data-gradient dispatch chains (ConvLaunch) and the
// launchers that take it, the views of a volume and its sub-lattices (dense_view, lattice_view) with the one decode of a class
// index into parities (class_parity), the class tables (single_class, dgrad_parity_classes), tile geometry and the weight image
// index.  Pointer-level functions and the problem descriptor they take (ConvProblem, which the entry points fill and the
// pointer-level functions turn into a ConvLaunch) are declared in conv_api.h; what only the weight-gradient units share - their
// launch descriptor (WgradLaunch), launchers and class tables - in conv_wgrad_common.h; the device primitives that are not about convolutions
// (vector types, MFMA wrappers, LDS-DMA) live in gfx950.h.
#pragma once
#include "conv_api.h"
#include "gfx950.h"
#include <stdlib.h>

// operand descriptors shared by the launchers of all three translation units (external linkage)
namespace dgconv {
// Strided view of a channels-last volume: element strides (channel stride 1) + logical extent.  Lets the same kernel
// run on parity sub-lattices (stride-2 data gradient, 2x2x2 transposed conv) without copies.
struct View {
  long long sb, sd, sh, sw;
  int D, H, W;
};
// weight tap used by each of the 27 virtual taps (-1: tap not present)
struct Taps {
  signed char wt[27];
};

// A launch can run up to 8 independent "classes" (blockIdx.z) that share shapes but differ in operand offsets and tap
// tables: the 8 parity sub-lattices of a stride-2 data gradient, or the 8 output offsets of a 2x2x2 transposed conv.
struct ConvClasses {
  int n;
  int acc[8];
  long long xoff[8], yoff[8];   // element offsets of the operands of class c
  Taps taps[8];
  // K concatenation (pointwise variant): input channel c lives in segment c / kseg at element offset segoff[c / kseg]
  // (the 8 parity sub-lattices of a transposed conv's output gradient); kseg == 0: plain channels
  int kseg;
  long long segoff[8];
};

// One forward / data-gradient launch as the dispatch chain hands it down: operands and their views, channel counts (Cin / CinP
// are the GEMM's K, Cout / CoutP its N), the InstanceNorm partial sums to leave (or null), the tap count of the weight image
// and the stream.  The three riders concern the ring / row-reuse launchers only:
//   gst: InstanceNorm-backward context of dgtta_conv3d_k3_dgrad_gstats;
//   xkh != 0: x holds its two 32-channel K halves as dense planes xkh elements apart - only the ring kernel reads that layout
//             (Src::kh of the pointer-level functions);
//   dry: no launch, DGTTA_OK iff the ring kernel would take this call (ConvProblem::dry, dgtta_conv3d_k3_blocked_supported).
struct ConvLaunch {
  const void *x;
  View xv;
  const void *w;
  const float *bias;
  void *y;
  View yv;
  int B, Cin, Cout, CinP, CoutP;
  double *stats;
  int ntaps_src;
  hipStream_t st;
  RowsGstCtx *gst = nullptr;
  long long xkh = 0;
  bool dry = false;
};

}  // namespace dgconv
using namespace dgconv;

// Launchers of the specialised kernels that the dispatchers of conv_mfma.hip try first; they return DGTTA_ERR_UNSUPPORTED for a
// launch they do not take.
// conv_rows.hip: row-reuse kernel
int conv3_rows_launch(const ConvLaunch &L, const Taps &taps, int is_f16);
// conv_ring.hip: D-ring kernel
int conv3_ring_launch(const ConvLaunch &L, const Taps &taps, int64_t stats_cap_slots, int is_f16);
// conv_s2.hip: register-operand kernel of the two large stride-2 encoder transitions (L.w: the forward weight image)
int conv3_s2_regs(const ConvLaunch &L, int64_t cap_slots, int dtype);

namespace {

template <typename T>
struct Elem;
template <>
struct Elem<float> {
  static constexpr int EPV = 4;  // elements per 16 bytes
};
template <>
struct Elem<bf16_t> {
  static constexpr int EPV = 8;
};
template <>
struct Elem<f16_t> {
  static constexpr int EPV = 8;
};

// Tile geometry.  MBW: voxels of an M-block along W (32/16/8); an M-block spans RPM = 32/MBW rows of H.
// MBH x MBD M-blocks per workgroup (MPW = MBH*MBD/4 per wave).  S = stride; S == 0 selects the POINTWISE variant
// (stride 1, centre tap only, no halo) used by the 2x2x2 transposed-conv compositions.
template <int MBW, int MBH, int MBD, int S>
struct Geo {
  static constexpr int SE = (S == 0) ? 1 : S;        // effective stride
  static constexpr int HALO = (S == 0) ? 0 : 1;
  static constexpr int NTAP = (S == 0) ? 1 : 27;     // taps staged in LDS
  static constexpr int RPM = 32 / MBW;
  static constexpr int TW = MBW, TH = RPM * MBH, TD = MBD;
  static constexpr int MB = MBH * MBD, MPW = MB / 4;
  // input halo extents
  static constexpr int ID = (TD - 1) * SE + 1 + 2 * HALO, IH = (TH - 1) * SE + 1 + 2 * HALO,
                       IW = (TW - 1) * SE + 1 + 2 * HALO;
  // LDS row of W: for S=2 the row is split into even / odd columns, each IWH long
  static constexpr int IWH = (S != 2) ? IW : (IW + 1) / 2;
  static constexpr int ROW = (S != 2) ? IW : 2 * IWH;
  static constexpr int NV = ID * IH * ROW;
  __host__ __device__ static constexpr int lds_col(int wx) { return (S != 2) ? wx : (wx & 1) * IWH + (wx >> 1); }
};

template <typename T, int MBW, int MBH, int MBD, int S, int NB, int KSPC>
struct ConvCfg {
  typedef Geo<MBW, MBH, MBD, S> G;
  static constexpr int EPV = Elem<T>::EPV;
  static constexpr int NG = 2 * KSPC;        // 16-byte channel groups per K-chunk
  static constexpr int CK = NG * EPV;        // channels per K-chunk
  static constexpr int NC = 32 * NB;
  static constexpr size_t A_BYTES = (size_t)NG * G::NV * 16;
  static constexpr size_t B_BYTES = (size_t)G::NTAP * NG * NC * 16;
  static constexpr size_t LDS_BYTES = A_BYTES + B_BYTES;
};

__device__ const uint4 g_zero16 = {0u, 0u, 0u, 0u};

inline View dense_view(int B, int D, int H, int W, int ld) {
  (void)B;
  View v;
  v.sw = ld;
  v.sh = (long long)W * ld;
  v.sd = (long long)H * W * ld;
  v.sb = (long long)D * H * W * ld;
  v.D = D;
  v.H = H;
  v.W = W;
  return v;
}
// Parities of class (or output offset) c of a layer with strides (sd, sh, sw) in {1, 2}^3: the classes number the parity
// combinations of the strided axes, flattened in D, H, W order (torch's flattening of a kernel = stride); an axis of stride 1 has
// parity 0.  The one place that knows this numbering.
struct Parity { int p[3]; };      // D, H, W
inline Parity class_parity(int c, int sd, int sh, int sw) {
  return {{sd == 2 ? (c / (sh * sw)) % 2 : 0, sh == 2 ? (c / sw) % 2 : 0, sw == 2 ? c % 2 : 0}};
}
// sub-lattice of class c of the dense volume `full` (its sb is kept) with per-axis steps (sd, sh, sw): elements s * v + parity
inline View lattice_view(const View &full, int sd, int sh, int sw, int c, long long *offset) {
  const Parity par = class_parity(c, sd, sh, sw);
  View v = full;
  *offset = par.p[0] * full.sd + par.p[1] * full.sh + par.p[2] * full.sw;
  v.sd *= sd, v.sh *= sh, v.sw *= sw;
  v.D = (full.D - par.p[0] + sd - 1) / sd;
  v.H = (full.H - par.p[1] + sh - 1) / sh;
  v.W = (full.W - par.p[2] + sw - 1) / sw;
  return v;
}

inline int epv_of(int dtype) { return dtype == DGTTA_F32 ? 4 : 8; }      // Elem<T>::EPV of a runtime dtype
// an operand the MFMA kernels can read: 16-byte aligned rows of whole 16-byte groups (EPV elements), K padded to a k-step
inline bool operand_ok(int EPV, const void *p, long long ld_elems, int Cin, int CinP) {
  return ld_elems % EPV == 0 && ((uintptr_t)p & 15) == 0 && CinP % (2 * EPV) == 0 &&
         ld_elems >= (Cin + EPV - 1) / EPV * EPV;
}

inline Taps identity_taps(int mirror) {
  Taps t;
  for (int i = 0; i < 27; ++i) t.wt[i] = (signed char)(mirror ? 26 - i : i);
  return t;
}

// one class over the whole operands (offsets 0, plain channels)
inline ConvClasses single_class(const Taps &taps, int accumulate) {
  ConvClasses cs{};
  cs.n = 1;
  cs.acc[0] = accumulate;
  cs.taps[0] = taps;
  return cs;
}

// Data gradient of a [kd, 3, 3] conv with strides (sd, sh, sw) in {1, 2}^3 as stride-1 gathers of dy: one class per parity p
// of the strided axes (class index = parities flattened in D, H, W order), writing the sub-lattice s * j + p of dx (*yv: its
// view - with even strided extents one shape serves all classes).  Per axis the virtual tap v (0..k-1) reads dy[j + v - k/2]
// and carries weight tap t = p + k/2 - s * (v - k/2) where 0 <= t < k.
inline ConvClasses dgrad_parity_classes(const ConvProblem &P, int lddx, int accumulate, View *yv) {
  ConvClasses cs{};
  cs.n = P.noff();
  const int ks[3] = {P.kd, 3, 3}, ss[3] = {P.sd, P.sh, P.sw};
  const View full = dense_view(P.B, P.Di, P.Hi, P.Wi, lddx);
  for (int c = 0; c < cs.n; ++c) {
    const Parity par = class_parity(c, P.sd, P.sh, P.sw);
    *yv = lattice_view(full, P.sd, P.sh, P.sw, c, &cs.yoff[c]);
    cs.acc[c] = accumulate;
    for (int t = 0; t < 27; ++t) cs.taps[c].wt[t] = -1;
    for (int v = 0; v < P.ntaps(); ++v) {
      const int vv[3] = {v / 9, (v / 3) % 3, v % 3};
      int real[3];
      bool ok = true;
      for (int a = 0; a < 3; ++a) {
        const int pad = ks[a] / 2;
        real[a] = par.p[a] + pad - ss[a] * (vv[a] - pad);
        ok = ok && real[a] >= 0 && real[a] < ks[a];
      }
      if (ok) cs.taps[c].wt[v] = (signed char)(real[0] * 9 + real[1] * 3 + real[2]);
    }
  }
  return cs;
}

// index of element (n, k, tap) in the LDS-image-ordered weight array [N/32][K/(2*EPV)][ntaps][2][32][EPV]
__host__ __device__ inline int64_t conv_weight_image_index(int n, int k, int tap, int KP, int ntaps, int EPV) {
  const int64_t chunk2 = k / (2 * EPV);
  const int g = (k / EPV) % 2, e = k % EPV;
  return ((((((int64_t)(n / 32)) * (KP / (2 * EPV)) + chunk2) * ntaps + tap) * 2 + g) * 32 + n % 32) * EPV + e;
}
}  // namespace

