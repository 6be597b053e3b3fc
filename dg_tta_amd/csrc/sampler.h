// Pieces every linear sampler of the library shares (warp.hip: affine maps; deform.hip: dense displacement fields): the
// normalised identity coordinate as at::affine_grid builds it and the eight trilinear corners in ATen's order.
#pragma once
#include "common.h"

namespace {

// normalised base coordinate j of n, as at::affine_grid builds it: linspace(-1,1,n) * (n-1) / n
__device__ __forceinline__ float base_coord(int j, int n) {
  if (n <= 1) return 0.f;
  const float step = 2.0f / (float)(n - 1);
  float v = (j < n / 2) ? (-1.0f + step * (float)j) : (1.0f - step * (float)(n - 1 - j));
  return (v * (float)(n - 1)) / (float)n;
}

struct Sample {
  float ix, iy, iz;
};

struct Corners {
  int x0, y0, z0;
  float w[8];  // order tnw,tne,tsw,tse,bnw,bne,bsw,bse (t: z0, n: y0, w: x0) as ATen's grid_sampler_3d
};

__device__ __forceinline__ Corners corners(const Sample &s) {
  Corners c;
  const float fx = floorf(s.ix), fy = floorf(s.iy), fz = floorf(s.iz);
  c.x0 = (int)fx;
  c.y0 = (int)fy;
  c.z0 = (int)fz;
  const float ex = (fx + 1.0f) - s.ix, ey = (fy + 1.0f) - s.iy, ez = (fz + 1.0f) - s.iz;  // weights of the low side
  const float ux = s.ix - fx, uy = s.iy - fy, uz = s.iz - fz;                                // weights of the high side
  c.w[0] = ex * ey * ez;
  c.w[1] = ux * ey * ez;
  c.w[2] = ex * uy * ez;
  c.w[3] = ux * uy * ez;
  c.w[4] = ex * ey * uz;
  c.w[5] = ux * ey * uz;
  c.w[6] = ex * uy * uz;
  c.w[7] = ux * uy * uz;
  return c;
}

}  // namespace
