// Counter-based MIND noise: Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11; the
// constants and known answers are Random123's public ones) + Box-Muller.  The definition (include/dgtta.h carries it too):
//   (x0,x1,x2,x3) = Philox4x32-10(counter = (v, 4 b + c/4, offset_lo, offset_hi), key = (seed_lo, seed_hi))
//   u_i = ((x_i >> 9) + 0.5) 2^-23                       exact in fp32, in (0,1)
//   c%4 = 0: sqrt(-2 ln u0) cos(2 pi u1)   1: sqrt(-2 ln u0) sin(2 pi u1)   2, 3: the same from (u2, u3)
// for channel c of voxel v = (d H + h) W + w of GLOBAL sample b.  Nothing else enters a value, so the fill kernel and the
// fused descriptor kernel (both in mind3d.hip, both through mind_noise below) agree whatever their tiling.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

struct PhiloxKey {      // kernel argument of the seeded kernels
  uint32_t seed_lo, seed_hi, off_lo, off_hi;
  int b0;               // global index of the call's first sample
};

static inline PhiloxKey make_philox_key(uint64_t seed, uint64_t offset, int b0) {
  return PhiloxKey{(uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)offset, (uint32_t)(offset >> 32), b0};
}

__device__ __forceinline__ void philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1,
                                              uint32_t x[4]) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  x[0] = c0; x[1] = c1; x[2] = c2; x[3] = c3;
}

// Two normals from two words.  The angle is handed to sincospif as 2 u (exact in fp32): its argument reduction is exact, so
// the 2.4e-7 rounding of an fp32 "2 pi u" does not enter; logf / sqrtf / sincospif are the full-precision library routines.
__device__ __forceinline__ void philox_normal_pair(uint32_t xa, uint32_t xb, float &n0, float &n1) {
  const float ua = ((float)(xa >> 9) + 0.5f) * 0x1p-23f, ub = ((float)(xb >> 9) + 0.5f) * 0x1p-23f;
  const float r = sqrtf(-2.0f * logf(ua));
  float s, c;
  sincospif(2.0f * ub, &s, &c);
  n0 = r * c;
  n1 = r * s;
}

// The one generator: channels c0 .. c0+N-1 of voxel v of global sample b; N = 4 (c0 a multiple of 4: a whole Philox call) or
// N = 2 (c0 even: one half of a call's output).
template <int N>
__device__ __forceinline__ void mind_noise(const PhiloxKey &k, int b, int c0, uint32_t v, float n[N]) {
  static_assert(N == 4 || N == 2, "a whole Philox call or one of its halves");
  uint32_t x[4];
  philox4x32_10(v, 4u * (uint32_t)b + (uint32_t)(c0 >> 2), k.off_lo, k.off_hi, k.seed_lo, k.seed_hi, x);
  if constexpr (N == 4) {
    philox_normal_pair(x[0], x[1], n[0], n[1]);
    philox_normal_pair(x[2], x[3], n[2], n[3]);
  } else {
    const bool hi = (c0 & 2) != 0;
    philox_normal_pair(hi ? x[2] : x[0], hi ? x[3] : x[1], n[0], n[1]);
  }
}
