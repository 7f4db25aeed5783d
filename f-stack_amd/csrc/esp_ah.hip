// esp_ah.hip — AH digest sessions (CSP_MODE_DIGEST) for gfx950: HMAC-SHA1 or
// HMAC-SHA2-256 / -384 / -512 over a whole packet.
//
// Replaces swcr_authcompute (freebsd/opencrypto/cryptosoft.c:317-382) for the
// request ah_input / ah_output build (netipsec/xform_ah.c:613-664, :972-1047):
// the message is the packet, any byte length, then the ESN high word for
// CSP_F_ESN sessions; the ICV field (mlen bytes: 12 / 16 / 24 / 32,
// xform_ah_authsize) lies INSIDE the hashed range, at a multiple of 4.
//
// Mapping: lane = record, as esp_cbc.hip's verify pass -- each lane runs its
// record's compressions from the SA's precomputed ipad / opad states, and the
// whole blocks reach their lane through the quad (lane 4Q+k loads piece k of
// the quad's four records, a DPP transpose hands each lane its own), 128
// contiguous bytes of a record per step.  No table, no LDS: occupancy is set
// by registers alone, so the workgroup is 256 threads with no minimum-
// occupancy bound, and several workgroups share a CU.
//
// Against esp_cbc.hip's hmac_quad:
//  * byte tail: the message is rec[0, L0) || be32(esn_hi)? || 0x80 || 0...
//    with L0 any byte count, so the ESN word and the 0x80 start at any byte of
//    a dword (funnel shifts); whole blocks are read only while they end inside
//    L0 and no read goes beyond the dword holding byte L0 - 1;
//  * ICV hole: on the batch path the dwords of [salt, salt + mlen) read as
//    zero (ah_input's save-and-zero, ah_output's zeroing); only the blocks
//    overlapping the field take the masked path;
//  * the ICV is stored after the wave's block loop has ended for every lane: a
//    quad neighbour's coalesced load may read this lane's record until then.
#include <hip/hip_runtime.h>

#include <algorithm>

#define ESPGPU_CHK_TAG 3   // (bounds_chk.h site ids)
#include "espgpu_internal.h"
#include "sha_dev.h"

namespace espgpu {

namespace {

constexpr int kDigWG = 256;

// The tail of a record's inner message: the dword at byte offset o (a
// multiple of 4) of rec[0, L0) || suffix, where the suffix (the ESN word, if
// any, then 0x80) is the 64-bit big-endian value s_hi:s_lo starting at byte
// L0.  ob = L0 & ~3, sh = 8 * (L0 & 3).  Dwords inside the hole read as zero.
__device__ __forceinline__ uint32_t msg_word(const uint8_t *rec, uint32_t o, uint32_t L0, uint32_t ob, uint32_t sh,
                                             uint32_t s_hi, uint32_t s_lo, uint32_t hlo, uint32_t hhi) {
  uint32_t v = 0;
  if (o < L0) {                                   // (at most the dword holding byte L0 - 1)
    v = bswap32(esp_ld4(rec + o));
    if (o == ob) v &= ~(0xffffffffu >> sh);       // (o == ob < L0: sh is 8, 16 or 24)
    if (o >= hlo && o < hhi) v = 0;
  }
  if (o == ob) v |= s_hi >> sh;
  else if (o == ob + 4) v = __builtin_amdgcn_alignbit(s_hi, s_lo, sh);
  return v;
}

struct QuadRecs {
  const uint8_t *pr[4];
  uint32_t pn64[4];
};

// The quad's step: 128 contiguous bytes (two 64-byte halves) of each of the
// quad's four records, loaded coalesced (lane q takes piece q of every record
// while that half lies below the record's whole-block bytes, pn64 halves) and
// transposed, so that m[0..31] are this lane's record's 32 big-endian words.
// Every lane of the wave runs it: the DPP moves are outside any
// lane-dependent branch.
__device__ __forceinline__ void quad_step(const QuadRecs &qr, uint32_t half0, int q, bool qb0, bool qb1,
                                          uint32_t (&m)[32]) {
  uint4 PP[2][4];
#pragma unroll
  for (int nb = 0; nb < 2; ++nb)
#pragma unroll
    for (int i = 0; i < 4; ++i)
      PP[nb][i] = half0 + nb < qr.pn64[i] ? ld16(qr.pr[i] + 64 * (half0 + nb) + 16 * q) : make_uint4(0, 0, 0, 0);
#pragma unroll
  for (int nb = 0; nb < 2; ++nb) {
    const uint4 *P = PP[nb];
    uint32_t X[4] = {P[0].x, P[1].x, P[2].x, P[3].x}, Y[4] = {P[0].y, P[1].y, P[2].y, P[3].y};
    uint32_t Z[4] = {P[0].z, P[1].z, P[2].z, P[3].z}, V[4] = {P[0].w, P[1].w, P[2].w, P[3].w};
    quad_transpose4(X, qb0, qb1);
    quad_transpose4(Y, qb0, qb1);
    quad_transpose4(Z, qb0, qb1);
    quad_transpose4(V, qb0, qb1);
#pragma unroll
    for (int k = 0; k < 4; ++k) {                 // piece k of this lane's record
      m[16 * nb + 4 * k] = bswap32(X[k]);
      m[16 * nb + 4 * k + 1] = bswap32(Y[k]);
      m[16 * nb + 4 * k + 2] = bswap32(Z[k]);
      m[16 * nb + 4 * k + 3] = bswap32(V[k]);
    }
  }
}

// the quad's record addresses and whole-block bytes in 64-byte halves
__device__ __forceinline__ void quad_recs(const uint8_t *rec, uint32_t n64, QuadRecs &qr) {
  const uint64_t rp = (uint64_t)(uintptr_t)rec;
  const uint32_t rlo = (uint32_t)rp, rhi = (uint32_t)(rp >> 32);
  qr.pr[0] = gptr(((uint64_t)qbcast<0>(rhi) << 32) | qbcast<0>(rlo));
  qr.pr[1] = gptr(((uint64_t)qbcast<1>(rhi) << 32) | qbcast<1>(rlo));
  qr.pr[2] = gptr(((uint64_t)qbcast<2>(rhi) << 32) | qbcast<2>(rlo));
  qr.pr[3] = gptr(((uint64_t)qbcast<3>(rhi) << 32) | qbcast<3>(rlo));
  qr.pn64[0] = qbcast<0>(n64);
  qr.pn64[1] = qbcast<1>(n64);
  qr.pn64[2] = qbcast<2>(n64);
  qr.pn64[3] = qbcast<3>(n64);
}

// HMAC-SHA1 / SHA2-256 of rec[0, L0) || be32(esn_hi)? for a whole wave (act =
// this lane's record is hashed; every lane calls it; the block loop runs to
// the wave's longest message).  [hlo, hhi): the hole (empty: hlo = hhi = 0).
template <int HS>
__device__ void digest_quad(bool act, const uint8_t *rec, uint32_t L0, bool esn, uint32_t esn_hi, uint32_t hlo,
                            uint32_t hhi, kptr ipad, kptr opad, uint32_t out[16]) {
  constexpr int W = Hash<HS>::W;
  const int lane = threadIdx.x & 63, q = lane & 3;
  const bool qb0 = (q & 1) != 0, qb1 = (q & 2) != 0;
  const uint32_t L = act ? L0 + (esn ? 4u : 0u) : 0u;
  const uint32_t nfull = act ? L0 / 64 : 0u;
  const uint32_t total = act ? (L + 9 + 63) / 64 : 0u;
  const uint64_t bits = (uint64_t)(64 + L) * 8;
  const uint32_t s_hi = esn ? esn_hi : 0x80000000u, s_lo = esn ? 0x80000000u : 0u;
  const uint32_t ob = L0 & ~3u, sh = 8 * (L0 & 3u);
  uint32_t h[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) h[k] = (act && k < W) ? ipad[k] : 0u;
  QuadRecs qr;
  quad_recs(rec, nfull, qr);
  const uint32_t tw = wave_max(total);
  for (uint32_t b0 = 0; b0 <= tw; b0 += 2) {      // wave-uniform trip count
    uint32_t m[32];
    quad_step(qr, b0, q, qb0, qb1, m);
#pragma unroll
    for (int nb = 0; nb < 2; ++nb) {
      const uint32_t b = b0 + nb;
      if (nb > 0 && b > tw) continue;             // (wave-uniform)
      uint32_t w[16];
      if (b < nfull) {
#pragma unroll
        for (int k = 0; k < 16; ++k) w[k] = m[16 * nb + k];
        if (64 * b < hhi && 64 * b + 64 > hlo) {  // the block overlaps the ICV field
#pragma unroll
          for (int k = 0; k < 16; ++k) {
            const uint32_t o = 64 * b + 4 * k;
            if (o >= hlo && o < hhi) w[k] = 0;
          }
        }
      } else if (b < total) {
#pragma unroll
        for (int k = 0; k < 16; ++k) w[k] = msg_word(rec, 64 * b + 4 * k, L0, ob, sh, s_hi, s_lo, hlo, hhi);
        if (b == total - 1) {
          w[14] = (uint32_t)(bits >> 32);
          w[15] = (uint32_t)bits;
        }
      } else if (b == total) {                    // (lanes past their total keep their digest)
        outer_block<HS>(h, w);
        if (act) {
#pragma unroll
          for (int k = 0; k < W; ++k) h[k] = opad[k];
        }
      }
      if (b <= total) {
        if (eopts() & 0x20000) {                  // knob: the loads without the compression
#pragma unroll
          for (int k = 0; k < 16; ++k) h[k & 7] ^= w[k];
        } else {
          Hash<HS>::compress(h, w);
        }
      }
    }
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) out[k] = h[k];
}

// The same for HMAC-SHA2-384 / 512 (is384 per lane): 128-byte blocks, one per
// step; out = the digest as big-endian 32-bit words.
__device__ void digest_quad_wide(bool act, const uint8_t *rec, uint32_t L0, bool esn, uint32_t esn_hi, uint32_t hlo,
                                 uint32_t hhi, bool is384, kptr ipad, kptr opad, uint32_t out[16]) {
  const int lane = threadIdx.x & 63, q = lane & 3;
  const bool qb0 = (q & 1) != 0, qb1 = (q & 2) != 0;
  const uint32_t L = act ? L0 + (esn ? 4u : 0u) : 0u;
  const uint32_t nfull = act ? L0 / 128 : 0u;
  const uint32_t total = act ? (L + 17 + 127) / 128 : 0u;
  const uint64_t bits = (uint64_t)(128 + L) * 8;
  const uint32_t s_hi = esn ? esn_hi : 0x80000000u, s_lo = esn ? 0x80000000u : 0u;
  const uint32_t ob = L0 & ~3u, sh = 8 * (L0 & 3u);
  uint64_t h[8];
#pragma unroll
  for (int k = 0; k < 8; ++k) h[k] = act ? ((uint64_t)ipad[2 * k] << 32) | ipad[2 * k + 1] : 0ull;
  QuadRecs qr;
  quad_recs(rec, 2 * nfull, qr);
  const uint32_t tw = wave_max(total);
  for (uint32_t b = 0; b <= tw; ++b) {            // wave-uniform trip count
    uint32_t m[32];
    quad_step(qr, 2 * b, q, qb0, qb1, m);
    uint64_t w[16];
    if (b < nfull) {
      if (128 * b < hhi && 128 * b + 128 > hlo) { // the block overlaps the ICV field
#pragma unroll
        for (int k = 0; k < 32; ++k) {
          const uint32_t o = 128 * b + 4 * k;
          if (o >= hlo && o < hhi) m[k] = 0;
        }
      }
    } else if (b < total) {
#pragma unroll
      for (int k = 0; k < 32; ++k) m[k] = msg_word(rec, 128 * b + 4 * k, L0, ob, sh, s_hi, s_lo, hlo, hhi);
      if (b == total - 1) {                       // 128-bit length: the high 64 bits are zero
        m[30] = (uint32_t)(bits >> 32);
        m[31] = (uint32_t)bits;
      }
    }
    if (b < total) {
#pragma unroll
      for (int k = 0; k < 16; ++k) w[k] = ((uint64_t)m[2 * k] << 32) | m[2 * k + 1];
    } else if (b == total) {
      // outer block: inner digest (6 or 8 words) || 0x80 || 0... || bit length
#pragma unroll
      for (int k = 0; k < 16; ++k) w[k] = k < 6 ? h[k] : 0ull;
      w[6] = is384 ? 0x8000000000000000ull : h[6];
      w[7] = is384 ? 0ull : h[7];
      w[8] = is384 ? 0ull : 0x8000000000000000ull;
      w[15] = (uint64_t)(128 + (is384 ? 48 : 64)) * 8;
      if (act) {
#pragma unroll
        for (int k = 0; k < 8; ++k) h[k] = ((uint64_t)opad[2 * k] << 32) | opad[2 * k + 1];
      }
    }
    if (b <= total) sha512_compress(h, w);
  }
#pragma unroll
  for (int k = 0; k < 8; ++k) {
    out[2 * k] = (uint32_t)(h[k] >> 32);
    out[2 * k + 1] = (uint32_t)h[k];
  }
}

// WIDE: the launch for HMAC-SHA2-384 / 512 sessions (the narrow one carries
// no 64-bit code).  Units are one wave's worth of records: a 64-record
// ETA-range chunk of the planner (a DIGEST SA is keyed as an ETA one), or 64
// consecutive descriptors; the kernel takes the records whose SA is a DIGEST
// session of its hash width, writes each one's status exactly once, and
// leaves every other record alone.
template <bool WIDE>
__global__ __launch_bounds__(kDigWG) void digest_kernel(DigestParams p) {
  const int lane = threadIdx.x & 63;
  const bool implicit = p.chunks == nullptr;
  const uint32_t u0 = implicit ? 0u : p.nchunks[0];
  const uint32_t u1 = implicit ? (p.n + 63) / 64 : p.nchunks[1];
  for (;;) {
    uint32_t t = 0;
    if (lane == 0) t = atomicAdd(&p.queue[0], 1u);
    const uint32_t u = u0 + __builtin_amdgcn_readfirstlane(t);
    if (u >= u1) break;
    uint32_t di = 0;
    bool have;
    if (implicit) {
      di = u * 64 + lane;
      have = di < p.n;
    } else {
      const Chunk ch = esp_at_ld(CHK_CHUNKS, p.chunks, u);
      have = (uint32_t)lane < ch.count;
      if (have) di = esp_at_ld(CHK_ORDER, p.order, ch.start + lane);
    }
    bool mine = false, valid = false, verify = false, esn = false, ok = false;
    uint32_t off4 = 0, len = 0, sa = 0, esnh = 0, icvo = 0, mlen = 0;
    int hq = 0;                                   // narrow: 1 SHA-1, 2 SHA2-256; wide: 1 SHA2-384, 2 SHA2-512
    if (have) {
      const uint4 dv = esp_desc_ld16(p.desc, di);
      off4 = dv.x;
      len = dv.y & 0xffffu;
      sa = dv.y >> 16;
      esnh = dv.z;
      const DevSA *s = sa < p.nsas ? esp_at_ptr(CHK_SAS, p.sas, sa) : nullptr;
      if (s && s->mode == ESPGPU_CSP_MODE_DIGEST && wide_hash(s->aalg) == WIDE) {
        mine = true;
        mlen = s->mlen;
        esn = (s->flags & ESPGPU_CSP_F_ESN) != 0;
        verify = p.op == 0 || (p.op == 2 && (dv.w & kDigVerifyBit) != 0);
        const uint32_t so = p.op == 2 ? dv.w & ~kDigVerifyBit : dv.w;
        valid = len >= 1 && so <= 0xffffu && (so & 3) == 0 && so + mlen <= len;
        icvo = valid ? so : 0u;
        if (valid)
          hq = (s->aalg == ESPGPU_CRYPTO_SHA2_256_HMAC || s->aalg == ESPGPU_CRYPTO_SHA2_512_HMAC) ? 2 : 1;
      }
    }
    const uint8_t *rec = p.arena + (size_t)off4 * 4;
    // the batch path hashes the ICV field as zeros; the driver path the
    // record as it stands
    const uint32_t hlo = p.op == 2 ? 0u : icvo, hhi = p.op == 2 ? 0u : icvo + mlen;
    if (WIDE) {
      if (__any(hq != 0)) {
        const bool act = hq != 0;
        const DevSA *s = esp_at_ptr(CHK_SAS, p.sas, act ? sa : 0u);
        uint32_t dg[16];
        digest_quad_wide(act, rec, len, esn, esnh, hlo, hhi, hq == 1, kp(s->ipad), kp(s->opad), dg);
        // (the block loop has ended for every lane: the ICV may be stored)
        if (act && verify) {
          uint32_t diff = 0;
          for (uint32_t k = 0; k < mlen / 4; ++k)
            diff |= bswap32(dg[k]) ^ esp_ld4(rec + icvo + 4 * k);
          ok = diff == 0;
        } else if (act) {
          for (uint32_t k = 0; k < mlen / 4; ++k)
            esp_st4(p.icv_out + (size_t)off4 * 4 + icvo + 4 * k, bswap32(dg[k]));
        }
      }
    } else {
      for (int hs = 1; hs <= 2; ++hs) {           // (not unrolled: two digest_quad bodies)
        if (!__any(hq == hs)) continue;           // wave-uniform
        const bool act = hq == hs;
        const DevSA *s = esp_at_ptr(CHK_SAS, p.sas, act ? sa : 0u);
        uint32_t dg[16];
        if (hs == 2)
          digest_quad<HS_SHA256>(act, rec, len, esn, esnh, hlo, hhi, kp(s->ipad), kp(s->opad), dg);
        else
          digest_quad<HS_SHA1>(act, rec, len, esn, esnh, hlo, hhi, kp(s->ipad), kp(s->opad), dg);
        // (the block loop has ended for every lane, and the other hash's pass
        // loads only its own records: the ICV may be stored)
        if (act && verify) {
          uint32_t diff = 0;
          for (uint32_t k = 0; k < mlen / 4; ++k)
            diff |= bswap32(dg[k]) ^ esp_ld4(rec + icvo + 4 * k);
          ok = diff == 0;
        } else if (act) {
          for (uint32_t k = 0; k < mlen / 4; ++k)
            esp_st4(p.icv_out + (size_t)off4 * 4 + icvo + 4 * k, bswap32(dg[k]));
        }
      }
    }
    if (mine) {
      const bool good = valid && (ok || !verify);
      esp_at_st(CHK_STATUS, p.status, di, !valid ? ESPGPU_EINVAL : (good ? ESPGPU_OK : ESPGPU_EBADMSG));
      if (p.trailer) esp_at_st(CHK_TRAILER, p.trailer, di, good ? ESPGPU_TR_VALID : 0u);
    }
  }
  // Every wave leaves the loop after drawing one ticket past the end, so once
  // all have retired no ticket is drawn again: reset for the next launch.
  if (lane == 0 && atomicAdd(&p.queue[1], 1u) == gridDim.x * (kDigWG / 64) - 1) {
    atomicExch(&p.queue[0], 0u);
    atomicExch(&p.queue[1], 0u);
  }
}

}  // namespace

// Workgroups of 256 threads (one wave per SIMD each); per CU as many as the
// kernel's registers admit (3 narrow at 134 VGPRs, 2 wide at 177).
int launch_digest(const DigestParams &p, int narrow, int wide, int grid, void *stream) {
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (grid <= 0) grid = 256;
  // implicit units (64 records, one wave each): no more workgroups than units
  auto clamp = [&](int g) {
    if (p.chunks != nullptr) return g;
    const int units = (int)((p.n + 63) / 64), wpg = kDigWG / 64;
    return std::max(1, std::min(g, (units + wpg - 1) / wpg));
  };
#ifdef ESPGPU_BOUNDS
  ESPGPU_CHK_SET(p.chk, st);
#endif
  if (narrow) hipLaunchKernelGGL((digest_kernel<false>), dim3(clamp(3 * grid)), dim3(kDigWG), 0, st, p);
  if (wide) hipLaunchKernelGGL((digest_kernel<true>), dim3(clamp(2 * grid)), dim3(kDigWG), 0, st, p);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace espgpu
