// dev_prims.h — the device primitives every kernel file shares: one-
// instruction bit operations, 16- / 8-byte accesses at 4-byte alignment, and
// the wave-wide reductions.  Everything has internal linkage and is inlined.
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>

namespace espgpu {

namespace {

__device__ __forceinline__ uint32_t xor3(uint32_t a, uint32_t b, uint32_t c) {
  return __builtin_amdgcn_bitop3_b32(a, b, c, 0x96);
}
__device__ __forceinline__ uint32_t perm(uint32_t hi, uint32_t lo, uint32_t sel) {
  return __builtin_amdgcn_perm(hi, lo, sel);
}
__device__ __forceinline__ uint32_t ror16(uint32_t x) { return __builtin_amdgcn_alignbit(x, x, 16); }
__device__ __forceinline__ uint32_t rotl(uint32_t x, int n) { return __builtin_amdgcn_alignbit(x, x, 32 - n); }
__device__ __forceinline__ uint32_t rotr(uint32_t x, int n) { return __builtin_amdgcn_alignbit(x, x, n); }
__device__ __forceinline__ uint32_t bswap32(uint32_t x) { return perm(x, x, 0x00010203u); }

// 16- and 8-byte accesses at 4-byte alignment as single vector memory
// operations (one IR access each, so the backend never splits or re-merges them)
typedef uint32_t V4a __attribute__((ext_vector_type(4), aligned(4)));
typedef uint32_t V2a __attribute__((ext_vector_type(2), aligned(4)));
// (nontemporal hints on these measured 4-14 % slower: DESIGN.md §6)
__device__ __forceinline__ uint4 ld16(const uint8_t *p) {
  const V4a v = *reinterpret_cast<const V4a *>(p);
  return make_uint4(v.x, v.y, v.z, v.w);
}
__device__ __forceinline__ void st16(uint8_t *p, uint4 v) {
  V4a u = {v.x, v.y, v.z, v.w};
  *reinterpret_cast<V4a *>(p) = u;
}
__device__ __forceinline__ void st8(uint8_t *p, uint32_t a, uint32_t b) {
  V2a u = {a, b};
  *reinterpret_cast<V2a *>(p) = u;
}

// Store the first `rem` bytes (a multiple of 4) of v.
__device__ __forceinline__ void st_partial(uint8_t *p, uint4 v, int rem) {
  if (rem >= 16) {
    st16(p, v);
    return;
  }
  // the last block of a record: 4, 8 or 12 bytes, no store shared with the
  // full-block path (a common first-word store would be hoisted out of both
  // branches and split every full block into three stores)
  if (rem > 4)
    st8(p, v.x, v.y);
  else
    *reinterpret_cast<uint32_t *>(p) = v.x;
  if (rem > 8) *reinterpret_cast<uint32_t *>(p + 8) = v.z;
}

__device__ __forceinline__ uint4 xor4(uint4 a, uint4 b) {
  return make_uint4(a.x ^ b.x, a.y ^ b.y, a.z ^ b.z, a.w ^ b.w);
}

// Wave-wide (64 lanes) reductions; every lane of the wave calls them.  Sum and
// maximum leave the result in every lane; the scan is inclusive, lane by lane.
__device__ __forceinline__ uint32_t wave_sum(uint32_t x) {
  for (uint32_t d = 32; d > 0; d >>= 1) x += __shfl_xor(x, d);
  return x;
}
__device__ __forceinline__ uint32_t wave_max(uint32_t v) {
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) v = max(v, (uint32_t)__shfl_xor((int)v, o));
  return v;
}
__device__ __forceinline__ uint32_t wave_incl_add(uint32_t x, uint32_t lane) {
  for (uint32_t d = 1; d < 64; d <<= 1) {
    const uint32_t y = __shfl_up(x, d);
    if (lane >= d) x += y;
  }
  return x;
}

}  // namespace

}  // namespace espgpu
