// dev_prims.h — the device primitives every kernel file shares: one-
// instruction bit operations, 16- / 8-byte accesses at 4-byte alignment, and
// the wave-wide reductions.  Everything has internal linkage and is inlined.
#pragma once
#include <hip/hip_runtime.h>

#include <stdint.h>

#include "bounds_chk.h"

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

// The other global-memory accesses of esp_gcm.hip and esp_ah.hip, spelled once so that the bounds-checked build
// (bounds_chk.h) can stand in front of every one of them: a 4-byte access at a
// record pointer; element i of a per-record array, of the chunk list or of the
// SA table (K: the CHK_* kind that names its bound), loaded, stored or
// addressed; a descriptor as one 16-byte load.  Here each is the single
// access it spells.  (esp_ld4w: dword k at a dword pointer formed from a
// record pointer.)
#ifndef ESPGPU_BOUNDS
#define esp_ld4(p) (*reinterpret_cast<const uint32_t *>(p))
#define esp_st4(p, v) (*reinterpret_cast<uint32_t *>(p) = (v))
#define esp_ld4w(q, k) ((q)[k])
#define esp_at_ld(K, a, i) ((a)[i])
#define esp_at_st(K, a, i, v) ((a)[i] = (v))
#define esp_at_ptr(K, a, i) ((a) + (i))
#define esp_desc_ld16(a, i) (*reinterpret_cast<const uint4 *>((a) + (i)))
#else
#ifndef ESPGPU_CHK_TAG
#define ESPGPU_CHK_TAG 0   // a file outside the checked three: its block is never set, nothing is checked
#endif
#define CHK_SITE ((uint32_t)(ESPGPU_CHK_TAG) << 16 | (uint32_t)__LINE__)
__device__ __forceinline__ uint4 chk_ld16(const uint8_t *p, uint32_t site) {
  return chk_range(p, 16, false, site) ? ld16(p) : make_uint4(0, 0, 0, 0);
}
__device__ __forceinline__ void chk_st16(uint8_t *p, uint4 v, uint32_t site) {
  if (chk_range(p, 16, true, site)) st16(p, v);
}
__device__ __forceinline__ void chk_st8(uint8_t *p, uint32_t a, uint32_t b, uint32_t site) {
  if (chk_range(p, 8, true, site)) st8(p, a, b);
}
__device__ __forceinline__ void chk_st_partial(uint8_t *p, uint4 v, int rem, uint32_t site) {
  if (chk_range(p, rem >= 16 ? 16u : (uint32_t)rem, true, site)) st_partial(p, v, rem);
}
__device__ __forceinline__ uint32_t chk_ld4(const uint8_t *p, uint32_t site) {
  return chk_range(p, 4, false, site) ? *reinterpret_cast<const uint32_t *>(p) : 0u;
}
__device__ __forceinline__ void chk_st4(uint8_t *p, uint32_t v, uint32_t site) {
  if (chk_range(p, 4, true, site)) *reinterpret_cast<uint32_t *>(p) = v;
}
template <class T>
__device__ __forceinline__ T chk_at_ld(uint32_t kind, const T *a, uint64_t i, uint32_t site) {
  return chk_index(kind, i, site) ? a[i] : T{};
}
template <class T, class V>
__device__ __forceinline__ void chk_at_st(uint32_t kind, T *a, uint64_t i, V v, uint32_t site) {
  if (chk_index(kind, i, site)) a[i] = (T)v;
}
template <class T>
__device__ __forceinline__ T *chk_at_ptr(uint32_t kind, T *a, uint64_t i, uint32_t site) {
  return a + (chk_index(kind, i, site) ? i : 0);
}
template <class T>
__device__ __forceinline__ uint4 chk_desc_ld16(const T *a, uint64_t i, uint32_t site) {
  return chk_index(CHK_DESC, i, site) ? *reinterpret_cast<const uint4 *>(a + i) : make_uint4(0, 0, 0, 0);
}
#define ld16(p) chk_ld16((p), CHK_SITE)
#define st16(p, v) chk_st16((p), (v), CHK_SITE)
#define st8(p, a, b) chk_st8((p), (a), (b), CHK_SITE)
#define st_partial(p, v, rem) chk_st_partial((p), (v), (rem), CHK_SITE)
#define esp_ld4(p) chk_ld4((p), CHK_SITE)
#define esp_st4(p, v) chk_st4((p), (v), CHK_SITE)
#define esp_ld4w(q, k) chk_ld4(reinterpret_cast<const uint8_t *>(q) + 4 * (k), CHK_SITE)
#define esp_at_ld(K, a, i) chk_at_ld((K), (a), (i), CHK_SITE)
#define esp_at_st(K, a, i, v) chk_at_st((K), (a), (i), (v), CHK_SITE)
#define esp_at_ptr(K, a, i) chk_at_ptr((K), (a), (i), CHK_SITE)
#define esp_desc_ld16(a, i) chk_desc_ld16((a), (i), CHK_SITE)
#endif

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
