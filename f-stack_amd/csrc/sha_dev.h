// sha_dev.h — device-side hash primitives shared by the HIP kernels that run
// HMAC per record (esp_cbc.hip: ESP encrypt-then-MAC; esp_ah.hip: AH digest
// sessions): the SHA-1 / SHA2-256 / SHA2-512 compressions, the HMAC outer
// block, the quad transpose behind the coalesced block loads, and the
// measurement-knob hook.  Everything has internal linkage: each kernel file
// gets its own copy (and, in `make knobs` builds, its own knob word).
#pragma once
#include <hip/hip_runtime.h>

#include "dev_prims.h"
#include "espgpu_internal.h"
#include "sha512_consts.h"

namespace espgpu {

namespace {

constexpr int HS_SHA1 = 0, HS_SHA256 = 1;

typedef const __attribute__((address_space(4))) uint32_t *kptr;

// Measurement knobs for the decrypt kernels, compiled in only by `make knobs`
// (bench.py --tuning eta_opts=N with ESPGPU_LIB pointing at
// libespgpu_knobs.so): 0x10000 skips the verify pass (every record decrypts),
// 0x20000 the HMAC compressions (the loads stay), 0x40000 the decrypt pass's
// AES, 0x80000 its loads and stores; in the fused CBC + HMAC encrypt pass
// 0x100000 skips the stores, 0x200000 the loads, 0x400000 the compressions,
// 0x800000 the AES.  They break results on purpose, to split the kernel's time.
#ifdef ESPGPU_KNOBS
__device__ uint32_t e_opts;
__device__ __forceinline__ uint32_t eopts() {
  return *(const __attribute__((address_space(4))) uint32_t *)(const void *)&e_opts;
}
#else
__device__ __forceinline__ constexpr uint32_t eopts() { return 0; }
#endif

// ---- SHA-1 compression (sha1_step, freebsd/crypto/sha1.c:94-176) ----------
__device__ __forceinline__ void sha1_compress(uint32_t h[5], uint32_t w[16]) {
  uint32_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4];
#pragma unroll
  for (int t = 0; t < 80; ++t) {
    uint32_t wt;
    if (t < 16) {
      wt = w[t];
    } else {
      wt = rotl(xor3(w[(t - 3) & 15], w[(t - 8) & 15], w[(t - 14) & 15]) ^ w[t & 15], 1);
      w[t & 15] = wt;
    }
    uint32_t f, k;
    if (t < 20) {
      f = __builtin_amdgcn_bitop3_b32(b, c, d, 0xCA);   // (b & c) | (~b & d)
      k = 0x5a827999u;
    } else if (t < 40) {
      f = xor3(b, c, d);
      k = 0x6ed9eba1u;
    } else if (t < 60) {
      f = __builtin_amdgcn_bitop3_b32(b, c, d, 0xE8);   // majority
      k = 0x8f1bbcdcu;
    } else {
      f = xor3(b, c, d);
      k = 0xca62c1d6u;
    }
    // e + K + W_t does not depend on a: summed first (and materialized, so
    // the adds are not reassociated), the round's critical path is a ->
    // {rotl 5, f} -> one add3 instead of a -> f -> add3 -> add3
    uint32_t ekw = e + k + wt;
    asm volatile("" : "+v"(ekw));
    const uint32_t tmp = rotl(a, 5) + f + ekw;
    e = d;
    d = c;
    c = rotl(b, 30);
    b = a;
    a = tmp;
  }
  h[0] += a; h[1] += b; h[2] += c; h[3] += d; h[4] += e;
}

// ---- SHA-256 compression (SHA256_Transform, freebsd/crypto/sha2/sha256c.c:135) ----
__constant__ uint32_t kK256[64] = {
    0x428a2f98u, 0x71374491u, 0xb5c0fbcfu, 0xe9b5dba5u, 0x3956c25bu, 0x59f111f1u, 0x923f82a4u, 0xab1c5ed5u,
    0xd807aa98u, 0x12835b01u, 0x243185beu, 0x550c7dc3u, 0x72be5d74u, 0x80deb1feu, 0x9bdc06a7u, 0xc19bf174u,
    0xe49b69c1u, 0xefbe4786u, 0x0fc19dc6u, 0x240ca1ccu, 0x2de92c6fu, 0x4a7484aau, 0x5cb0a9dcu, 0x76f988dau,
    0x983e5152u, 0xa831c66du, 0xb00327c8u, 0xbf597fc7u, 0xc6e00bf3u, 0xd5a79147u, 0x06ca6351u, 0x14292967u,
    0x27b70a85u, 0x2e1b2138u, 0x4d2c6dfcu, 0x53380d13u, 0x650a7354u, 0x766a0abbu, 0x81c2c92eu, 0x92722c85u,
    0xa2bfe8a1u, 0xa81a664bu, 0xc24b8b70u, 0xc76c51a3u, 0xd192e819u, 0xd6990624u, 0xf40e3585u, 0x106aa070u,
    0x19a4c116u, 0x1e376c08u, 0x2748774cu, 0x34b0bcb5u, 0x391c0cb3u, 0x4ed8aa4au, 0x5b9cca4fu, 0x682e6ff3u,
    0x748f82eeu, 0x78a5636fu, 0x84c87814u, 0x8cc70208u, 0x90befffau, 0xa4506cebu, 0xbef9a3f7u, 0xc67178f2u,
};

__device__ __forceinline__ void sha256_compress(uint32_t h[8], uint32_t w[16]) {
  uint32_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4], f = h[5], g = h[6], hh = h[7];
#pragma unroll
  for (int t = 0; t < 64; ++t) {
    uint32_t wt;
    if (t < 16) {
      wt = w[t];
    } else {
      const uint32_t x = w[(t - 15) & 15], y = w[(t - 2) & 15];
      const uint32_t s0 = xor3(rotr(x, 7), rotr(x, 18), x >> 3);
      const uint32_t s1 = xor3(rotr(y, 17), rotr(y, 19), y >> 10);
      wt = w[t & 15] + s0 + w[(t - 7) & 15] + s1;
      w[t & 15] = wt;
    }
    // h + K_t + W_t (and d + that) do not depend on this round's e or a:
    // summed first, so e' = S1 + ch + (d+h+K+W) and t1 are one add3 each
    uint32_t hkw = hh + kK256[t] + wt;
    asm volatile("" : "+v"(hkw));
    uint32_t dhkw = d + hkw;
    asm volatile("" : "+v"(dhkw));
    const uint32_t S1 = xor3(rotr(e, 6), rotr(e, 11), rotr(e, 25));
    const uint32_t ch = __builtin_amdgcn_bitop3_b32(e, f, g, 0xCA);     // (e & f) | (~e & g)
    const uint32_t t1 = S1 + ch + hkw;
    const uint32_t S0 = xor3(rotr(a, 2), rotr(a, 13), rotr(a, 22));
    const uint32_t mj = __builtin_amdgcn_bitop3_b32(a, b, c, 0xE8);     // majority
    hh = g; g = f; f = e; e = S1 + ch + dhkw;
    d = c; c = b; b = a; a = t1 + S0 + mj;
  }
  h[0] += a; h[1] += b; h[2] += c; h[3] += d; h[4] += e; h[5] += f; h[6] += g; h[7] += hh;
}

// The two HMAC hashes behind one interface: W chaining words.
template <int HS> struct Hash;
template <> struct Hash<HS_SHA1> {
  static constexpr int W = 5;
  static __device__ __forceinline__ void compress(uint32_t h[8], uint32_t w[16]) { sha1_compress(h, w); }
};
template <> struct Hash<HS_SHA256> {
  static constexpr int W = 8;
  static __device__ __forceinline__ void compress(uint32_t h[8], uint32_t w[16]) { sha256_compress(h, w); }
};

// the outer block: inner digest || 0x80 || 0... || bit length of (64 + digest)
template <int HS>
__device__ __forceinline__ void outer_block(const uint32_t h[8], uint32_t w[16]) {
  constexpr int W = Hash<HS>::W;
#pragma unroll
  for (int k = 0; k < 16; ++k) w[k] = k < W ? h[k] : (k == W ? 0x80000000u : 0u);
  w[15] = (64 + 4 * W) * 8;
}

template <int CTRL>
__device__ __forceinline__ uint32_t qdpp(uint32_t x) {
  return (uint32_t)__builtin_amdgcn_mov_dpp((int)x, CTRL, 0xf, 0xf, true);
}
template <int I>
__device__ __forceinline__ uint32_t qbcast(uint32_t x) { return qdpp<I * 0x55>(x); }   // quad_perm [I,I,I,I]

// A record address rebuilt from its broadcast halves, as a global-memory
// pointer: a plain integer-to-pointer cast is a generic (flat) address, and
// flat loads and stores count in lgkmcnt too, beside the LDS table reads
// (measured equal in time: profiles/r6_cfg3_encrypt_pipe_ab.txt).
__device__ __forceinline__ uint8_t *gptr(uint64_t a) {
  return (uint8_t *)(__attribute__((address_space(1))) uint8_t *)(uintptr_t)a;
}

// lane q of a quad: A[i] (i = 0..3) -> lane q holds, in A[k], lane k's A[q]
__device__ __forceinline__ void quad_transpose4(uint32_t (&A)[4], bool qb0, bool qb1) {
#pragma unroll
  for (int b = 0; b < 2; ++b) {                  // distance 2: pairs (0,2), (1,3)
    const uint32_t y = qdpp<0x4E>(qb1 ? A[b] : A[b + 2]);
    A[b] = qb1 ? y : A[b];
    A[b + 2] = qb1 ? A[b + 2] : y;
  }
#pragma unroll
  for (int b = 0; b < 4; b += 2) {               // distance 1: pairs (0,1), (2,3)
    const uint32_t y = qdpp<0xB1>(qb0 ? A[b] : A[b + 1]);
    A[b] = qb0 ? y : A[b];
    A[b + 1] = qb0 ? A[b + 1] : y;
  }
}

// ---- SHA-512 / SHA-384 compression (SHA512_Transform, freebsd/crypto/sha2/sha512c.c:196) ----
// 64-bit words held as uint64_t; rotations as two v_alignbit on the halves.
__constant__ uint64_t kK512[80] = ESPGPU_SHA512_K;

__device__ __forceinline__ uint64_t rotr64(uint64_t x, int n) {
  const uint32_t lo = (uint32_t)x, hi = (uint32_t)(x >> 32);
  uint32_t rl, rh;
  if (n < 32) {
    rl = __builtin_amdgcn_alignbit(hi, lo, n);
    rh = __builtin_amdgcn_alignbit(lo, hi, n);
  } else {
    rl = __builtin_amdgcn_alignbit(lo, hi, n - 32);
    rh = __builtin_amdgcn_alignbit(hi, lo, n - 32);
  }
  return ((uint64_t)rh << 32) | rl;
}

__device__ __forceinline__ void sha512_compress(uint64_t h[8], uint64_t w[16]) {
  uint64_t a = h[0], b = h[1], c = h[2], d = h[3], e = h[4], f = h[5], g = h[6], hh = h[7];
#pragma unroll
  for (int t = 0; t < 80; ++t) {
    uint64_t wt;
    if (t < 16) {
      wt = w[t];
    } else {
      const uint64_t x = w[(t - 15) & 15], y = w[(t - 2) & 15];
      const uint64_t s0 = rotr64(x, 1) ^ rotr64(x, 8) ^ (x >> 7);
      const uint64_t s1 = rotr64(y, 19) ^ rotr64(y, 61) ^ (y >> 6);
      wt = w[t & 15] + s0 + w[(t - 7) & 15] + s1;
      w[t & 15] = wt;
    }
    const uint64_t S1 = rotr64(e, 14) ^ rotr64(e, 18) ^ rotr64(e, 41);
    const uint64_t ch = (e & f) ^ (~e & g);
    const uint64_t t1 = hh + S1 + ch + kK512[t] + wt;
    const uint64_t S0 = rotr64(a, 28) ^ rotr64(a, 34) ^ rotr64(a, 39);
    const uint64_t mj = (a & b) ^ (a & c) ^ (b & c);
    hh = g; g = f; f = e; e = d + t1;
    d = c; c = b; b = a; a = t1 + S0 + mj;
  }
  h[0] += a; h[1] += b; h[2] += c; h[3] += d; h[4] += e; h[5] += f; h[6] += g; h[7] += hh;
}

__device__ __forceinline__ bool wide_hash(uint32_t aalg) {
  return aalg == ESPGPU_CRYPTO_SHA2_384_HMAC || aalg == ESPGPU_CRYPTO_SHA2_512_HMAC;
}

__device__ __forceinline__ kptr kp(const void *p) { return (kptr)p; }

}  // namespace

}  // namespace espgpu
