// Device primitives of gfx950 (CDNA4) that more than one kernel file uses, each defined here once: the vector types of the MFMA
// operands, the MFMA wrappers selected by the storage type, 16-byte non-temporal accesses, and the LDS-DMA helpers with the
// waits and the barrier that go with them.  Nothing here is about convolutions: conv_common.h includes this header for the
// conv units, the other units (gin.hip, instnorm.hip, warp.hip, window_features.hip, window_logits.hip) include it directly.
#pragma once
#include "common.h"

namespace {

typedef __attribute__((ext_vector_type(2))) float f32x2_t;
typedef __attribute__((ext_vector_type(4))) float f32x4_t;
typedef __attribute__((ext_vector_type(16))) float f32x16_t;
typedef __attribute__((ext_vector_type(4))) unsigned u32x4_t;
typedef __attribute__((ext_vector_type(2))) __bf16 bf16x2_t;
typedef __attribute__((ext_vector_type(2))) _Float16 f16x2_t;
typedef __attribute__((ext_vector_type(8))) __bf16 bf16x8_t;
typedef __attribute__((ext_vector_type(8))) _Float16 f16x8_t;
typedef __attribute__((ext_vector_type(4))) short s16x4_t;                  // result of ds_read_b64_tr_b16
typedef __attribute__((ext_vector_type(8))) short s16x8_t;                  // two of them
typedef __attribute__((address_space(3))) s16x4_t lds_s16x4_t;
typedef __attribute__((address_space(3))) void lds_void_t;

// ---------------------------------------------------------------- MFMA, selected by the storage type
// 32x32 step on 16 bytes per lane: 32x32x16 for the 16-bit types, four 32x32x2 for fp32
template <typename T>
__device__ __forceinline__ void mfma_step(const uint4 &a, const uint4 &b, f32x16_t &acc);
template <>
__device__ __forceinline__ void mfma_step<bf16_t>(const uint4 &a, const uint4 &b, f32x16_t &acc) {
  acc = __builtin_amdgcn_mfma_f32_32x32x16_bf16(__builtin_bit_cast(bf16x8_t, a), __builtin_bit_cast(bf16x8_t, b), acc, 0,
                                                0, 0);
}
template <>
__device__ __forceinline__ void mfma_step<f16_t>(const uint4 &a, const uint4 &b, f32x16_t &acc) {
  acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8_t, a), __builtin_bit_cast(f16x8_t, b), acc, 0, 0, 0);
}
template <>
__device__ __forceinline__ void mfma_step<float>(const uint4 &a, const uint4 &b, f32x16_t &acc) {
  // lane half h holds channels 4h..4h+3 of the 8-channel k-step; instruction j contracts the pair {j, 4+j}
  acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.x), __uint_as_float(b.x), acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.y), __uint_as_float(b.y), acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.z), __uint_as_float(b.z), acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x2f32(__uint_as_float(a.w), __uint_as_float(b.w), acc, 0, 0, 0);
}

// 16x16 step on 16 bytes per lane: 16x16x32 for the 16-bit types, four 16x16x4 for fp32
template <typename T>
__device__ __forceinline__ void mfma16(const uint4 &a, const uint4 &b, f32x4_t &acc);
template <>
__device__ __forceinline__ void mfma16<bf16_t>(const uint4 &a, const uint4 &b, f32x4_t &acc) {
  acc = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, a), __builtin_bit_cast(bf16x8_t, b), acc, 0,
                                                0, 0);
}
template <>
__device__ __forceinline__ void mfma16<f16_t>(const uint4 &a, const uint4 &b, f32x4_t &acc) {
  acc = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8_t, a), __builtin_bit_cast(f16x8_t, b), acc, 0, 0, 0);
}
template <>
__device__ __forceinline__ void mfma16<float>(const uint4 &a, const uint4 &b, f32x4_t &acc) {
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a.x), __uint_as_float(b.x), acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a.y), __uint_as_float(b.y), acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a.z), __uint_as_float(b.z), acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_16x16x4f32(__uint_as_float(a.w), __uint_as_float(b.w), acc, 0, 0, 0);
}

// 32x32x16 and 16x16x32 steps on transposed-read operands (kept as bf16x8 bit patterns; the storage type picks the instruction)
template <typename T16>
__device__ __forceinline__ f32x16_t mfma32_tr(const bf16x8_t &a, const bf16x8_t &b, const f32x16_t &acc);
template <>
__device__ __forceinline__ f32x16_t mfma32_tr<bf16_t>(const bf16x8_t &a, const bf16x8_t &b, const f32x16_t &acc) {
  return __builtin_amdgcn_mfma_f32_32x32x16_bf16(a, b, acc, 0, 0, 0);
}
template <>
__device__ __forceinline__ f32x16_t mfma32_tr<f16_t>(const bf16x8_t &a, const bf16x8_t &b, const f32x16_t &acc) {
  return __builtin_amdgcn_mfma_f32_32x32x16_f16(__builtin_bit_cast(f16x8_t, a), __builtin_bit_cast(f16x8_t, b), acc, 0, 0, 0);
}
template <typename T16>
__device__ __forceinline__ f32x4_t mfma16_tr(const bf16x8_t &a, const bf16x8_t &b, const f32x4_t &acc);
template <>
__device__ __forceinline__ f32x4_t mfma16_tr<bf16_t>(const bf16x8_t &a, const bf16x8_t &b, const f32x4_t &acc) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, acc, 0, 0, 0);
}
template <>
__device__ __forceinline__ f32x4_t mfma16_tr<f16_t>(const bf16x8_t &a, const bf16x8_t &b, const f32x4_t &acc) {
  return __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8_t, a), __builtin_bit_cast(f16x8_t, b), acc, 0, 0, 0);
}

// two 4-voxel transposed LDS reads (rows of 64 B) = 8 consecutive voxels (k) of this lane's channel
__device__ __forceinline__ bf16x8_t tr_operand(const unsigned char *p) {
  const s16x4_t lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_t *)p);
  const s16x4_t hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_s16x4_t *)(p + 4 * 64));
  const s16x8_t v = {lo[0], lo[1], lo[2], lo[3], hi[0], hi[1], hi[2], hi[3]};
  return __builtin_bit_cast(bf16x8_t, v);
}

// ---------------------------------------------------------------- 16- and 8-byte non-temporal accesses (data streamed once)
// (st16_nt takes its value by value: through a reference the kernels of conv_s2.hip and instnorm.hip come out scheduled
// differently)
__device__ __forceinline__ uint4 ld16_nt(const void *p) {
  const u32x4_t v = __builtin_nontemporal_load(reinterpret_cast<const u32x4_t *>(p));
  return make_uint4(v[0], v[1], v[2], v[3]);
}
__device__ __forceinline__ uint2 ld8_nt(const void *p) {
  typedef __attribute__((ext_vector_type(2))) unsigned u32x2_t;
  const u32x2_t v = __builtin_nontemporal_load(reinterpret_cast<const u32x2_t *>(p));
  return make_uint2(v[0], v[1]);
}
__device__ __forceinline__ void st16_nt(void *p, uint4 val) {
  const u32x4_t nv = {val.x, val.y, val.z, val.w};
  __builtin_nontemporal_store(nv, reinterpret_cast<u32x4_t *>(p));
}

// ---------------------------------------------------------------- LDS-DMA
// LDS-DMA of 16 bytes per lane: lane i's bytes land at lds_addr + 16*i (lds_addr wave-uniform).  Issued from inline asm
// on purpose: the compiler then keeps no s_waitcnt bookkeeping for it (with the builtin it drains vmcnt(0) before the
// next ds_read, i.e. before the MFMA phase the copy is meant to overlap); the kernel waits with dma_wait_all() before
// the barrier that publishes the buffer.  M0 is compiler-reserved, so it is saved and restored in the same statement.
__device__ __forceinline__ void dma16_to_lds(const void *gsrc, unsigned lds_addr) {
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %2\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, off\n\ts_mov_b32 m0, %0"
               : "=&s"(keep)
               : "v"(gsrc), "s"(lds_addr)
               : "memory");
}
// The same through a buffer descriptor: a lane whose offset is outside the descriptor's range delivers zeros.
__device__ __forceinline__ void dma16_buf_to_lds(u32x4_t rsrc, unsigned voff, unsigned soff, unsigned lds_addr) {
  unsigned keep;
  asm volatile("s_mov_b32 %0, m0\n\ts_mov_b32 m0, %4\n\ts_nop 0\n\tbuffer_load_dwordx4 %1, %2, %3 offen lds\n\ts_mov_b32 m0, %0"
               : "=&s"(keep)
               : "v"(voff), "s"(rsrc), "s"(soff), "s"(lds_addr)
               : "memory");
}
// descriptor of `bytes` bytes at `base` for raw buffer operations (wave-uniform)
__device__ __forceinline__ u32x4_t make_rsrc(const void *base, unsigned bytes) {
  const unsigned long long a = (unsigned long long)base;
  u32x4_t r;
  r[0] = __builtin_amdgcn_readfirstlane((unsigned)a);
  r[1] = __builtin_amdgcn_readfirstlane((unsigned)(a >> 32) & 0xffffu);      // stride 0
  r[2] = __builtin_amdgcn_readfirstlane(bytes);
  r[3] = 0x00020000u;                                                         // raw 32-bit data format (gfx9 family)
  return r;
}
// an offset beyond every descriptor built with make_rsrc (the launchers that use it check < 2^31 bytes): such a lane reads
// zeros and its store is dropped
constexpr unsigned RSRC_OOB = 0x80000000u;

__device__ __forceinline__ void dma_wait_all() { asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); }
// Waits until at most n vector-memory operations are in flight, n a run-time value (s_waitcnt takes an immediate: a switch).
// MAXN: the largest n that gets a case of its own; any other n waits for everything, which is always safe.
template <int MAXN>
__device__ __forceinline__ void vm_wait_all_but(int n) {
  static_assert(MAXN <= 40, "add cases");
#define DG_VMCNT(k)                                          \
  case k:                                                    \
    if (k <= MAXN) {                                         \
      asm volatile("s_waitcnt vmcnt(" #k ")" ::: "memory");  \
      break;                                                 \
    }                                                        \
    [[fallthrough]];
  switch (n) {
    DG_VMCNT(1) DG_VMCNT(2) DG_VMCNT(3) DG_VMCNT(4) DG_VMCNT(5) DG_VMCNT(6) DG_VMCNT(7) DG_VMCNT(8) DG_VMCNT(9) DG_VMCNT(10)
    DG_VMCNT(11) DG_VMCNT(12) DG_VMCNT(13) DG_VMCNT(14) DG_VMCNT(15) DG_VMCNT(16) DG_VMCNT(17) DG_VMCNT(18) DG_VMCNT(19) DG_VMCNT(20)
    DG_VMCNT(21) DG_VMCNT(22) DG_VMCNT(23) DG_VMCNT(24) DG_VMCNT(25) DG_VMCNT(26) DG_VMCNT(27) DG_VMCNT(28) DG_VMCNT(29) DG_VMCNT(30)
    DG_VMCNT(31) DG_VMCNT(32) DG_VMCNT(33) DG_VMCNT(34) DG_VMCNT(35) DG_VMCNT(36) DG_VMCNT(37) DG_VMCNT(38) DG_VMCNT(39) DG_VMCNT(40)
    default: asm volatile("s_waitcnt vmcnt(0)" ::: "memory"); break;
  }
#undef DG_VMCNT
}
// workgroup barrier that orders LDS traffic only: __syncthreads() would also drain vmcnt, i.e. wait for DMA in flight
__device__ __forceinline__ void lds_barrier() { asm volatile("s_waitcnt lgkmcnt(0)\n\ts_barrier" ::: "memory"); }
__device__ __forceinline__ unsigned lds_addr_of(const void *p) {
  return __builtin_amdgcn_readfirstlane((unsigned)(size_t)(lds_void_t *)p);
}

}  // namespace
