// General-shape VALU convolution kernels ("impl 1", reference grade): correct for every Cin/Cout/stride/ld, used
//  (a) as the on-GPU cross-check for the MFMA implicit-GEMM kernels (conv_mfma.hip) at sizes where the CPU oracle
//      is too slow, and (b) for layer shapes the MFMA kernels do not cover (conv_dispatch.hip falls back to them).
// Semantics follow torch.nn.{Conv3d, ConvTranspose3d} as used by nnUNet's PlainConvUNet
// (dynamic-network-architectures==0.2; built at dg_tta/pretraining/nnUNetTrainer_GIN_MIND.py:46-53).
#include "conv_api.h"

namespace {

// ============================================================================ weight packing
template <typename T>
__global__ void pack_weights_kernel(const float *__restrict__ w, T *__restrict__ wf, T *__restrict__ wb, int Cin,
                                    int Cout, int CinP, int CoutP) {
  const int64_t nf = (int64_t)27 * CinP * CoutP;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nf; i += (int64_t)gridDim.x * blockDim.x) {
    {  // wf[tap][ci][co]
      int co = (int)(i % CoutP), ci = (int)((i / CoutP) % CinP), tap = (int)(i / ((int64_t)CoutP * CinP));
      float v = (co < Cout && ci < Cin) ? w[((int64_t)co * Cin + ci) * 27 + tap] : 0.f;
      if (wf) st_f<T>(wf + i, v);
    }
    {  // wb[tap'][co][ci] = w[co][ci][26-tap']
      int ci = (int)(i % CinP), co = (int)((i / CinP) % CoutP), tap = (int)(i / ((int64_t)CoutP * CinP));
      float v = (co < Cout && ci < Cin) ? w[((int64_t)co * Cin + ci) * 27 + (26 - tap)] : 0.f;
      if (wb) st_f<T>(wb + i, v);
    }
  }
}

// ============================================================================ conv 3x3x3 forward (reference grade)
// one thread per (voxel, co); lanes run over co so the x value is a broadcast and wf[tap][ci][co] is coalesced.
template <typename T>
__global__ void conv3_fwd_ref_kernel(const T *__restrict__ x, int ldx, const T *__restrict__ wf,
                                     const float *__restrict__ bias, T *__restrict__ y, int ldy, int Cin, int Cout,
                                     int CinP, int CoutP, int Di, int Hi, int Wi, int Do, int Ho, int Wo, int s,
                                     int64_t total) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int co = (int)(i % Cout);
    const int64_t vox = i / Cout;
    const int wo = (int)(vox % Wo), ho = (int)((vox / Wo) % Ho);
    const int d_o = (int)((vox / ((int64_t)Wo * Ho)) % Do), b = (int)(vox / ((int64_t)Wo * Ho * Do));
    float acc = 0.f;
    for (int kd = 0; kd < 3; ++kd) {
      const int di = d_o * s + kd - 1;
      if ((unsigned)di >= (unsigned)Di) continue;
      for (int kh = 0; kh < 3; ++kh) {
        const int hi = ho * s + kh - 1;
        if ((unsigned)hi >= (unsigned)Hi) continue;
        for (int kw = 0; kw < 3; ++kw) {
          const int wi = wo * s + kw - 1;
          if ((unsigned)wi >= (unsigned)Wi) continue;
          const T *xp = x + ((((int64_t)b * Di + di) * Hi + hi) * Wi + wi) * ldx;
          const T *wp = wf + ((int64_t)(kd * 9 + kh * 3 + kw) * CinP) * CoutP + co;
          for (int ci = 0; ci < Cin; ++ci) acc = __builtin_fmaf(ld_f<T>(xp + ci), ld_f<T>(wp + (int64_t)ci * CoutP), acc);
        }
      }
    }
    st_f<T>(y + vox * ldy + co, acc + (bias ? bias[co] : 0.f));
  }
}

// data gradient, any stride: thread per (input voxel, ci); wb[26-tap][co][ci] is coalesced over ci.
template <typename T>
__global__ void conv3_dgrad_ref_kernel(const T *__restrict__ dy, int lddy, const T *__restrict__ wb, T *__restrict__ dx,
                                       int lddx, int Cin, int Cout, int CinP, int CoutP, int Di, int Hi, int Wi, int Do,
                                       int Ho, int Wo, int s, int accumulate, int64_t total) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int ci = (int)(i % Cin);
    const int64_t vox = i / Cin;
    const int wi = (int)(vox % Wi), hi = (int)((vox / Wi) % Hi);
    const int di = (int)((vox / ((int64_t)Wi * Hi)) % Di), b = (int)(vox / ((int64_t)Wi * Hi * Di));
    float acc = 0.f;
    for (int kd = 0; kd < 3; ++kd) {
      int td = di + 1 - kd;
      if (td < 0 || td % s) continue;
      td /= s;
      if (td >= Do) continue;
      for (int kh = 0; kh < 3; ++kh) {
        int th = hi + 1 - kh;
        if (th < 0 || th % s) continue;
        th /= s;
        if (th >= Ho) continue;
        for (int kw = 0; kw < 3; ++kw) {
          int tw = wi + 1 - kw;
          if (tw < 0 || tw % s) continue;
          tw /= s;
          if (tw >= Wo) continue;
          const T *gp = dy + ((((int64_t)b * Do + td) * Ho + th) * Wo + tw) * lddy;
          const T *wp = wb + ((int64_t)(26 - (kd * 9 + kh * 3 + kw)) * CoutP) * CinP + ci;
          for (int co = 0; co < Cout; ++co) acc = __builtin_fmaf(ld_f<T>(gp + co), ld_f<T>(wp + (int64_t)co * CinP), acc);
        }
      }
    }
    T *o = dx + vox * lddx + ci;
    st_f<T>(o, accumulate ? ld_f<T>(o) + acc : acc);
  }
}

// weight gradient partials: grid (pairs/256, 27, nsplit); thread = one (ci,co) pair, loops over a voxel slice.
// partial layout [split][co][ci][tap] (torch order) so the final reduction is a plain sum over splits.
template <typename T>
__global__ void conv3_wgrad_ref_kernel(const T *__restrict__ x, int ldx, const T *__restrict__ dy, int lddy,
                                       float *__restrict__ part, int Cin, int Cout, int B, int Di, int Hi, int Wi,
                                       int Do, int Ho, int Wo, int s) {
  const int pair = blockIdx.x * blockDim.x + threadIdx.x;
  if (pair >= Cin * Cout) return;
  const int co = pair % Cout, ci = pair / Cout;
  const int tap = blockIdx.y, kd = tap / 9, kh = (tap / 3) % 3, kw = tap % 3;
  const int64_t nvox = (int64_t)B * Do * Ho * Wo;
  const int64_t per = cdiv64(nvox, gridDim.z);
  const int64_t v0 = (int64_t)blockIdx.z * per, v1 = (v0 + per < nvox) ? v0 + per : nvox;
  float acc = 0.f;
  for (int64_t vox = v0; vox < v1; ++vox) {
    const int wo = (int)(vox % Wo), ho = (int)((vox / Wo) % Ho);
    const int d_o = (int)((vox / ((int64_t)Wo * Ho)) % Do), b = (int)(vox / ((int64_t)Wo * Ho * Do));
    const int di = d_o * s + kd - 1, hi = ho * s + kh - 1, wi = wo * s + kw - 1;
    if ((unsigned)di >= (unsigned)Di || (unsigned)hi >= (unsigned)Hi || (unsigned)wi >= (unsigned)Wi) continue;
    const float xv = ld_f<T>(x + ((((int64_t)b * Di + di) * Hi + hi) * Wi + wi) * ldx + ci);
    acc = __builtin_fmaf(xv, ld_f<T>(dy + vox * lddy + co), acc);
  }
  part[(((int64_t)blockIdx.z * Cout + co) * Cin + ci) * 27 + tap] = acc;
}

__global__ void reduce_splits_kernel(const float *__restrict__ part, float *__restrict__ out, int64_t n, int nsplit,
                                     int accumulate) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    float s = 0.f;
    for (int k = 0; k < nsplit; ++k) s += part[(int64_t)k * n + i];
    out[i] = accumulate ? out[i] + s : s;
  }
}

// ============================================================================ ConvTranspose3d k2 s2
template <typename T>
__global__ void convT_fwd_ref_kernel(const T *__restrict__ x, int ldx, const float *__restrict__ w,
                                     const float *__restrict__ bias, T *__restrict__ out, int ldo, int Cin, int Cout,
                                     int Di, int Hi, int Wi, int64_t total) {
  const int Do = 2 * Di, Ho = 2 * Hi, Wo = 2 * Wi;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int co = (int)(i % Cout);
    const int64_t vox = i / Cout;
    const int wo = (int)(vox % Wo), ho = (int)((vox / Wo) % Ho);
    const int d_o = (int)((vox / ((int64_t)Wo * Ho)) % Do), b = (int)(vox / ((int64_t)Wo * Ho * Do));
    const int o = ((d_o & 1) * 2 + (ho & 1)) * 2 + (wo & 1);
    const T *xp = x + ((((int64_t)b * Di + (d_o >> 1)) * Hi + (ho >> 1)) * Wi + (wo >> 1)) * ldx;
    float acc = 0.f;
    for (int ci = 0; ci < Cin; ++ci) acc = __builtin_fmaf(ld_f<T>(xp + ci), w[((int64_t)ci * Cout + co) * 8 + o], acc);
    st_f<T>(out + vox * ldo + co, acc + (bias ? bias[co] : 0.f));
  }
}

template <typename T>
__global__ void convT_dgrad_ref_kernel(const T *__restrict__ dout, int lddo, const float *__restrict__ w,
                                       T *__restrict__ dx, int lddx, int Cin, int Cout, int Di, int Hi, int Wi,
                                       int64_t total) {
  const int Ho = 2 * Hi, Wo = 2 * Wi, Do = 2 * Di;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total; i += (int64_t)gridDim.x * blockDim.x) {
    const int ci = (int)(i % Cin);
    const int64_t vox = i / Cin;
    const int wi = (int)(vox % Wi), hi = (int)((vox / Wi) % Hi);
    const int di = (int)((vox / ((int64_t)Wi * Hi)) % Di), b = (int)(vox / ((int64_t)Wi * Hi * Di));
    float acc = 0.f;
    for (int o = 0; o < 8; ++o) {
      const T *gp =
          dout + ((((int64_t)b * Do + 2 * di + (o >> 2)) * Ho + 2 * hi + ((o >> 1) & 1)) * Wo + 2 * wi + (o & 1)) * lddo;
      for (int co = 0; co < Cout; ++co) acc = __builtin_fmaf(ld_f<T>(gp + co), w[((int64_t)ci * Cout + co) * 8 + o], acc);
    }
    st_f<T>(dx + vox * lddx + ci, acc);
  }
}

// partial[split][ci][co][o]; grid (pairs/256, 8, nsplit)
template <typename T>
__global__ void convT_wgrad_ref_kernel(const T *__restrict__ x, int ldx, const T *__restrict__ dout, int lddo,
                                       float *__restrict__ part, int Cin, int Cout, int B, int Di, int Hi, int Wi) {
  const int pair = blockIdx.x * blockDim.x + threadIdx.x;
  if (pair >= Cin * Cout) return;
  const int co = pair % Cout, ci = pair / Cout, o = blockIdx.y;
  const int Ho = 2 * Hi, Wo = 2 * Wi, Do = 2 * Di;
  const int64_t nvox = (int64_t)B * Di * Hi * Wi;
  const int64_t per = cdiv64(nvox, gridDim.z);
  const int64_t v0 = (int64_t)blockIdx.z * per, v1 = (v0 + per < nvox) ? v0 + per : nvox;
  float acc = 0.f;
  for (int64_t vox = v0; vox < v1; ++vox) {
    const int wi = (int)(vox % Wi), hi = (int)((vox / Wi) % Hi);
    const int di = (int)((vox / ((int64_t)Wi * Hi)) % Di), b = (int)(vox / ((int64_t)Wi * Hi * Di));
    const T *gp =
        dout + ((((int64_t)b * Do + 2 * di + (o >> 2)) * Ho + 2 * hi + ((o >> 1) & 1)) * Wo + 2 * wi + (o & 1)) * lddo;
    acc = __builtin_fmaf(ld_f<T>(x + vox * ldx + ci), ld_f<T>(gp + co), acc);
  }
  part[(((int64_t)blockIdx.z * Cin + ci) * Cout + co) * 8 + o] = acc;
}

}  // namespace

// ============================================================================ host launchers (conv_api.h)
int conv3_pack_weights_ref(const ConvProblem &P, const float *w_t, void *wf, void *wb) {
  const int64_t n = (int64_t)27 * P.CinP * P.CoutP;
  DISPATCH_T(P.dtype, hipLaunchKernelGGL((pack_weights_kernel<T>), dim3(gs_blocks(n)), dim3(256), 0, P.st,
                                         w_t, (T *)wf, (T *)wb, P.Cin, P.Cout, P.CinP, P.CoutP));
  DG_CHECK_LAUNCH("pack_weights_kernel");
  return DGTTA_OK;
}

int conv3_fwd_ref(const ConvProblem &P, Src x, const void *wf, const float *bias, Dst y) {
  const int64_t total = P.B * P.out_vox() * P.Cout;
  DISPATCH_T(P.dtype, hipLaunchKernelGGL((conv3_fwd_ref_kernel<T>), dim3(gs_blocks(total, 1 << 20)), dim3(256), 0, P.st,
                                         (const T *)x.p, x.ld, (const T *)wf, bias, (T *)y.p, y.ld, P.Cin, P.Cout, P.CinP, P.CoutP, P.Di,
                                         P.Hi, P.Wi, P.Do(), P.Ho(), P.Wo(), P.sd, total));
  DG_CHECK_LAUNCH("conv3_fwd_ref_kernel");
  return DGTTA_OK;
}

int conv3_dgrad_ref(const ConvProblem &P, Src dy, const void *wb, Dst dx, int accumulate) {
  const int64_t total = P.B * P.in_vox() * P.Cin;
  DISPATCH_T(P.dtype, hipLaunchKernelGGL((conv3_dgrad_ref_kernel<T>), dim3(gs_blocks(total, 1 << 20)), dim3(256), 0, P.st,
                                         (const T *)dy.p, dy.ld, (const T *)wb, (T *)dx.p, dx.ld, P.Cin, P.Cout, P.CinP, P.CoutP, P.Di, P.Hi,
                                         P.Wi, P.Do(), P.Ho(), P.Wo(), P.sd, accumulate, total));
  DG_CHECK_LAUNCH("conv3_dgrad_ref_kernel");
  return DGTTA_OK;
}

int reduce_splits(const float *part, float *out, int64_t n, int nsplit, int accumulate, hipStream_t st) {
  hipLaunchKernelGGL(reduce_splits_kernel, dim3(gs_blocks(n)), dim3(256), 0, st, part, out, n, nsplit, accumulate);
  DG_CHECK_LAUNCH("reduce_splits_kernel");
  return DGTTA_OK;
}

int conv3_wgrad_ref(const ConvProblem &P, Src x, Src dy, float *part, int nsplit, float *dw_t, int accumulate) {
  DISPATCH_T(P.dtype, hipLaunchKernelGGL((conv3_wgrad_ref_kernel<T>), dim3(cdiv(P.Cin * P.Cout, 256), 27, nsplit), dim3(256),
                                         0, P.st, (const T *)x.p, x.ld, (const T *)dy.p, dy.ld, part, P.Cin, P.Cout, P.B, P.Di, P.Hi, P.Wi,
                                         P.Do(), P.Ho(), P.Wo(), P.sd));
  DG_CHECK_LAUNCH("conv3_wgrad_ref_kernel");
  return reduce_splits(part, dw_t, (int64_t)P.Cout * P.Cin * 27, nsplit, accumulate, P.st);
}

int convT_fwd_ref(const ConvProblem &P, Src x, const float *w_t, const float *bias, Dst out) {
  const int64_t total = P.B * P.in_vox() * 8 * P.Cout;
  DISPATCH_T(P.dtype, hipLaunchKernelGGL((convT_fwd_ref_kernel<T>), dim3(gs_blocks(total, 1 << 20)), dim3(256), 0, P.st,
                                         (const T *)x.p, x.ld, w_t, bias, (T *)out.p, out.ld, P.Cin, P.Cout, P.Di, P.Hi, P.Wi, total));
  DG_CHECK_LAUNCH("convT_fwd_ref_kernel");
  return DGTTA_OK;
}

int convT_dgrad_ref(const ConvProblem &P, Src dout, const float *w_t, Dst dx) {
  const int64_t total = P.B * P.in_vox() * P.Cin;
  DISPATCH_T(P.dtype, hipLaunchKernelGGL((convT_dgrad_ref_kernel<T>), dim3(gs_blocks(total, 1 << 20)), dim3(256), 0, P.st,
                                         (const T *)dout.p, dout.ld, w_t, (T *)dx.p, dx.ld, P.Cin, P.Cout, P.Di, P.Hi, P.Wi, total));
  DG_CHECK_LAUNCH("convT_dgrad_ref_kernel");
  return DGTTA_OK;
}

int convT_wgrad_ref(const ConvProblem &P, Src x, Src dout, float *part, int nsplit, float *dw_t, int accumulate) {
  DISPATCH_T(P.dtype, hipLaunchKernelGGL((convT_wgrad_ref_kernel<T>), dim3(cdiv(P.Cin * P.Cout, 256), 8, nsplit), dim3(256),
                                         0, P.st, (const T *)x.p, x.ld, (const T *)dout.p, dout.ld, part, P.Cin, P.Cout, P.B, P.Di, P.Hi, P.Wi));
  DG_CHECK_LAUNCH("convT_wgrad_ref_kernel");
  return reduce_splits(part, dw_t, (int64_t)P.Cin * P.Cout * 8, nsplit, accumulate, P.st);
}
