// InstanceNorm3d + LeakyReLU element arithmetic, stated once for every kernel that applies it: the kernels of instnorm.hip, the
// norm-on-load of window_features.hip and the backward-statistics epilogues (GST) of conv_rows.hip and conv_ring.hip.
// The library is built with -ffp-contract=off: the parenthesisation here IS the result, bit for bit.  Device only.
#pragma once
#include "common.h"

// (One value per helper, returned by value, and the operands in the order the kernels load them: an output parameter bound to a
// kernel's local keeps that local in memory until the helper is inlined, a helper that takes all operands of two steps moves the
// loads of the second in front of the first - either way the kernels come out scheduled differently.)

// forward constants of one (sample, channel): z = lrelu(y * alpha + beta'), alpha = rstd * gamma, beta' = beta - mean * alpha
// (ATen's batch_norm transform form)
__device__ __forceinline__ float in_alpha(float rs, float gamma) { return rs * gamma; }
__device__ __forceinline__ float in_beta(float beta, float mu, float al) { return beta - mu * al; }
__device__ __forceinline__ float in_fwd(float y, float al, float bt, float slope) { return lrelu(y * al + bt, slope); }

// backward: xhat, and da = gz * lrelu'(a) of one element, a = xhat * gamma + beta
__device__ __forceinline__ float in_xhat(float y, float mu, float rs) { return (y - mu) * rs; }
__device__ __forceinline__ float in_act(float xhat, float ga, float be) { return xhat * ga + be; }
__device__ __forceinline__ float in_da(float a, float gz, float slope) { return a > 0.f ? gz : gz * slope; }
// dy = gamma * rstd * (da - c1 - xhat * c2), c1 = mean(da), c2 = mean(da * xhat)
__device__ __forceinline__ float in_dy(float da, float xhat, float ga, float rs, float c1, float c2) {
  return (ga * rs) * ((da - c1) - xhat * c2);
}

// da of two channels at once (V2 = a vector of two floats: v_pk_fma_f32 / v_pk_mul_f32), from the forward constants: a = fma(gA, y,
// gB), q = gz * lrelu'(a).  The GST epilogues sum q and q * y: sum q xhat = rstd (sum q y - mean sum q).
template <typename V2>
__device__ __forceinline__ V2 in_da2(V2 g2, V2 y2, V2 gA, V2 gB, float slope) {
  const V2 a2 = __builtin_elementwise_fma(gA, y2, gB);
  const V2 gsl = g2 * slope;
  return V2{a2[0] > 0.f ? g2[0] : gsl[0], a2[1] > 0.f ? g2[1] : gsl[1]};
}
