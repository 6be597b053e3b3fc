// Shared declarations of the MFMA convolution translation units (conv_mfma.hip, conv_rows.hip, conv_ring.hip, conv_s2.hip,
// convt_gemm.hip, conv_aniso.hip, conv_wgrad_ring.hip and, through conv_wgrad_common.h, the other weight-gradient units):
// operand descriptors and views, the launchers that take them, tile geometry and the weight image index.  Pointer-level
// functions are declared in conv_api.h, what only the weight-gradient units share in conv_wgrad_common.h; the device
// primitives that are not about convolutions (vector types, MFMA wrappers, LDS-DMA) live in gfx950.h.
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

}  // namespace dgconv
using namespace dgconv;

// Launchers of the specialised kernels that the dispatchers of conv_mfma.hip / conv_wgrad.hip try first; the conv ones return
// DGTTA_ERR_UNSUPPORTED for a launch they do not take, conv3_wgrad_ring_launch its slab count (0: nothing launched).
// conv_rows.hip: row-reuse kernel
int conv3_rows_launch(const void *x, const View &xv, const void *w, const Taps &taps, const float *bias, void *y, const View &yv,
                      int B, int Cin, int Cout, int CinP, int CoutP, double *stats, int ntaps_src, int is_f16, hipStream_t st,
                      RowsGstCtx *gst);
// conv_ring.hip: D-ring kernel
int conv3_ring_launch(const void *x, const View &xv, const void *w, const Taps &taps, const float *bias, void *y, const View &yv,
                      int B, int Cin, int Cout, int CinP, int CoutP, double *stats, int64_t stats_cap_slots, int ntaps_src,
                      int is_f16, hipStream_t st, RowsGstCtx *gst, long long xkh = 0, bool dry = false);
// conv_s2.hip: register-operand kernel of the two large stride-2 encoder transitions
int conv3_s2_regs(const void *x, const View &xv, const void *wimg, const float *bias, void *y, const View &yv, int B, int Cin,
                  int Cout, int CinP, int CoutP, double *stats, int64_t cap_slots, int dtype, hipStream_t st);
// conv_wgrad_ring.hip: ring sweep of the weight gradient
int conv3_wgrad_ring_launch(const void *x, const View &xv, const void *dy, const View &yv, float *slabs, size_t ws_bytes, int B,
                            int Cin, int Cout, int is_f16, hipStream_t st, int *rc, long long xkh = 0, bool dry = false);

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
// sub-lattice of a dense volume with per-axis steps (sd,sh,sw) at offsets (pd,ph,pw): elements s*v+p
View lattice_view(int D, int H, int W, int ld, int sd, int sh, int sw, int pd, int ph, int pw, long long *offset) {
  View v = dense_view(1, D, H, W, ld);
  *offset = ((long long)pd * H * W + (long long)ph * W + pw) * ld;
  v.sd *= sd;
  v.sh *= sh;
  v.sw *= sw;
  v.D = (D - pd + sd - 1) / sd;
  v.H = (H - ph + sh - 1) / sh;
  v.W = (W - pw + sw - 1) / sw;
  return v;
}
// sub-lattice of parity (pd,ph,pw) of a dense volume: elements 2v+p
View parity_view(int D, int H, int W, int ld, int pd, int ph, int pw, long long *offset) {
  return lattice_view(D, H, W, ld, 2, 2, 2, pd, ph, pw, offset);
}

template <typename T>
bool operand_ok(const void *p, long long ld_elems, int Cin, int CinP) {
  constexpr int EPV = Elem<T>::EPV;
  return ld_elems % EPV == 0 && ((uintptr_t)p & 15) == 0 && CinP % (2 * EPV) == 0 &&
         ld_elems >= (Cin + EPV - 1) / EPV * EPV;
}

inline Taps identity_taps(int mirror) {
  Taps t;
  for (int i = 0; i < 27; ++i) t.wt[i] = (signed char)(mirror ? 26 - i : i);
  return t;
}

// index of element (n, k, tap) in the LDS-image-ordered weight array [N/32][K/(2*EPV)][ntaps][2][32][EPV]
__host__ __device__ inline int64_t conv_weight_image_index(int n, int k, int tap, int KP, int ntaps, int EPV) {
  const int64_t chunk2 = k / (2 * EPV);
  const int g = (k / EPV) % 2, e = k % EPV;
  return ((((((int64_t)(n / 32)) * (KP / (2 * EPV)) + chunk2) * ntaps + tap) * 2 + g) * 32 + n % 32) * EPV + e;
}
}  // namespace

