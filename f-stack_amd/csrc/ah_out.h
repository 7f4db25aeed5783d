// ah_out.h — the outbound AH rules (include/espgpu.h, the outbound AH block):
// one set of functions for espgpu_ah_encap, espgpu_ah_frame and espgpu_ah_sent
// on the host and for aho_kernel, the ahf_* kernels and ahs_kernel on the
// device (ah_out.hip).  ipsec4/6_perform_request's transport-or-tunnel
// decision and ipsec_encap as encap.h states them, then ah_output
// (xform_ah.c:833-1065) with ah_massage_headers, out = 1 (:291-422), and
// ah_output_cb's m_copyback (:1120).
//
// Plain C++ with no HIP header, as encap.h and ah_in.h: the host side also
// builds with the host compiler alone (tools/ah_out_selftest.cpp runs it under
// its sanitizers).
#pragma once
#include <stdint.h>

#include "ah_in.h"
#include "encap.h"
#include "espgpu.h"
#include "frame.h"
#include "rule_hd.h"

namespace espgpu {

constexpr uint32_t kAhOutKnown = kEncKnown | ESPGPU_ENC_AH | ESPGPU_ENC_AH_KEEPTOS;

ESPGPU_HD inline bool ah_mlen_usable(uint32_t mlen) { return mlen >= 4 && mlen <= 64 && !(mlen & 3); }

// What checks 1-4 of espgpu_ah_encap leave for the build.
struct AhOutPlan {
  uint32_t skip;       // the packet's own header: ip_hl * 4, or 40
  uint32_t oh;         // the outer header: 0 (transport), 20 or 40
  uint32_t ahsize;
  uint32_t total;      // the wire packet's length
  bool tunnel, in6, af6;
};

// Checks 1-4 of espgpu_ah_encap.  Reads the SA and, of the packet, the first
// dword and (the proxy case) the destination address; writes nothing.
ESPGPU_HD inline int ah_out_plan(const espgpu_encsa *e, uint32_t mlen, const uint8_t *pkt, uint32_t len,
                                 uint32_t headroom, AhOutPlan *p) {
  // 1. the SA
  const uint32_t f = e->flags;
  if ((f & ~kAhOutKnown) || (f & kEncDf) == kEncDf || (f & kEncEcn) == kEncEcn) return ESPGPU_EINVAL;
  if (!(f & ESPGPU_ENC_AH)) return ESPGPU_EINVAL;
  if (f & ESPGPU_ENC_NATT) return ESPGPU_EINVAL;     // key.c:5702: NAT-T is ESP's alone
  if (!ah_mlen_usable(mlen)) return ESPGPU_EINVAL;
  const bool af6 = f & ESPGPU_ENC_AF6;
  uint32_t src[4], dst[4];
#pragma unroll
  for (uint32_t k = 0; k < 4; ++k) {
    src[k] = mem_ld32(e->src + 4 * k);
    dst[k] = mem_ld32(e->dst + 4 * k);
  }
  const bool src0 = af6 ? !(src[0] | src[1] | src[2] | src[3]) : !src[0];
  const bool dst0 = af6 ? !(dst[0] | dst[1] | dst[2] | dst[3]) : !dst[0];
  if (af6) {
    if (src0 || dst0) return ESPGPU_EINVAL;                                      // ipsec_output.c:961-964
    if (enc_linklocal(src[0]) || enc_linklocal(dst[0])) return ESPGPU_ENOTSUP;   // :975-981 is the host's
  }
  // 2. the packet
  if (len < 20) return ESPGPU_EINVAL;
  const uint32_t w0 = mem_ld32(pkt), ver = (w0 >> 4) & 0xfu;
  uint32_t skip;
  if (ver == 4) {
    const uint32_t ihl = w0 & 0xfu;
    if (ihl < 5 || ihl * 4 > len) return ESPGPU_EINVAL;
    skip = ihl * 4;
  } else if (ver == 6) {
    if (len < 40) return ESPGPU_EINVAL;
    skip = 40;                                       // :574-581, extension headers or not
  } else {
    return ESPGPU_EAFNOSUPPORT;                      // :932-933
  }
  if (len > 65535) return ESPGPU_EMSGSIZE;
  const bool in6 = ver == 6;
  // 3. tunnel or transport (:224-228, :543-547)
  bool tunnel = (f & ESPGPU_ENC_TUNNEL) || af6 != in6;
  if (!tunnel && !dst0) {                            // the proxy case
    if (in6) {
#pragma unroll
      for (uint32_t k = 0; k < 4; ++k) tunnel |= mem_ld32(pkt + 24 + 4 * k) != dst[k];
    } else {
      tunnel = mem_ld32(pkt + 16) != dst[0];
    }
  }
  if (tunnel && !af6 && (src0 || dst0)) return ESPGPU_EINVAL;                    // :938-941
  // 4. lengths
  const uint32_t ahsize = ah_hdrsiz(mlen, af6), oh = tunnel ? (af6 ? 40u : 20u) : 0u;
  const uint32_t total = len + ahsize + oh;
  if (total > 65535) return ESPGPU_EMSGSIZE;                                     // xform_ah.c:882
  if (ahsize + oh > headroom) return ESPGPU_ENOBUFS;                             // m_makespace, :907
  p->skip = skip;
  p->oh = oh;
  p->ahsize = ahsize;
  p->total = total;
  p->tunnel = tunnel;
  p->in6 = in6;
  p->af6 = af6;
  return 0;
}

// ah_opt_walk (ah_in.h) with out = 1: on top of the zero mask, whether a
// source-route option was seen and the last four bytes of the last one (the
// hashed ip_dst, xform_ah.c:362-365), as a memory-order dword.  A source-route
// option shorter than 4 bytes is refused (a deliberate difference: its "last
// address" would start in front of the option).  Reads bytes [20, skip) of the
// packet as it arrived and writes nothing.
ESPGPU_HD inline int ah_opt_walk_out(const uint8_t *pkt, uint32_t skip, uint64_t *zero, bool *sr, uint32_t *srdst) {
  uint64_t z = 0;
  bool seen = false;
  uint32_t last = 0;
  for (uint32_t off = 20; off < skip;) {
    const uint32_t o = pkt[off];
    if (o == 0) break;                                             // IPOPT_EOL, :315
    if (o == 1) {                                                  // IPOPT_NOP
      ++off;
      continue;
    }
    if (off + 1 >= skip) return ESPGPU_EINVAL;                     // :303-312
    const uint32_t count = pkt[off + 1];
    if (count < 2) return ESPGPU_EINVAL;                           // :329, :344, :370
    const bool keep = o == 0x82 || o == 0x85 || o == 0x86 || o == 0x94 || o == 0x95;
    if (off + count > skip) return ESPGPU_EINVAL;                  // :386
    if (o == 0x83 || o == 0x89) {                                  // IPOPT_LSRR, IPOPT_SSRR
      if (count < 4) return ESPGPU_EINVAL;
      const uint8_t *q = pkt + off + count - 4;
      last = (uint32_t)q[0] | (uint32_t)q[1] << 8 | (uint32_t)q[2] << 16 | (uint32_t)q[3] << 24;
      seen = true;
    }
    if (!keep) z |= ((1ull << count) - 1) << (off - 20);           // count <= 40 here
    off += count;
  }
  *zero = z;
  *sr = seen;
  *srdst = last;
  return 0;
}

// in_cksum over w[0..NW) (unused dwords zero, the checksum field zero), as
// enc_cksum
template <uint32_t NW>
ESPGPU_HD inline uint32_t ah_out_cksum(const uint32_t *w) {
  uint64_t acc = 0;
#pragma unroll
  for (uint32_t k = 0; k < NW; ++k) acc += w[k];
  acc = (acc & 0xffffffffu) + (acc >> 32);
  acc = (acc & 0xffffu) + ((acc >> 16) & 0xffffu) + (acc >> 32);
  acc = (acc & 0xffffu) + (acc >> 16);
  acc = (acc & 0xffffu) + (acc >> 16);
  return ~(uint32_t)acc & 0xffffu;
}

// Steps 5-8 of espgpu_ah_encap, after ah_out_plan returned 0.  NW is the
// number of header dwords the caller provides registers for, as
// ah_in_massage's: 10 serves every packet whose own header has no IPv4 options
// and leaves the option loop out; 15 serves all.  p.skip / 4 <= NW is the
// caller's.  Every load precedes every store, and the one refusal (the option
// loop's) precedes them too.
template <uint32_t NW>
ESPGPU_HD inline int ah_out_build(const espgpu_encsa *e, uint32_t mlen, uint8_t *pkt, uint32_t len, uint32_t ip_id,
                                  const AhOutPlan &p, uint8_t *hsave) {
  const uint32_t f = e->flags, nw = p.skip / 4;
  uint32_t w[NW];
#pragma unroll
  for (uint32_t k = 0; k < NW; ++k) w[k] = k < nw ? mem_ld32(pkt + 4 * k) : 0u;
  uint64_t zero = 0;
  bool sr = false;
  uint32_t srdst = 0;
  if (NW > 10 && !p.tunnel && !p.in6) {
    if (const int st = ah_opt_walk_out(pkt, p.skip, &zero, &sr, &srdst)) return st;
  }
  const uint32_t hs = p.tunnel ? p.oh : p.skip, hn = hs / 4;
  uint8_t *const wire = pkt - p.ahsize - p.oh;
  uint32_t nxt;
  if (p.tunnel) {
    // 5. the inner header as ipsec4/6_perform_request leave it, then the outer
    // header takes the registers
    uint32_t itos, idf;
    if (p.in6) {
      itos = ((w[0] & 0xfu) << 4) | ((w[0] >> 12) & 0xfu);                       // ipsec_output.c:925
      idf = 0;
      mem_st32(pkt + 4, (w[1] & 0xffff0000u) | enc_be16(len - 40));              // :533
      nxt = 41;
    } else {
      itos = (w[0] >> 8) & 0xffu;
      idf = (w[1] >> 16) & 0x40u;                                                // IP_DF, :916
      w[0] = (w[0] & 0xffffu) | enc_be16(len) << 16;                             // :230
      w[2] &= 0xffffu;                                                           // :231
      w[2] |= ah_out_cksum<NW>(w) << 16;                                         // :232
      mem_st32(pkt, w[0]);
      mem_st32(pkt + 8, w[2]);
      nxt = 4;
    }
    uint32_t otos = itos;                                                        // ip_ecn_ingress (ip_ecn.c:97-122)
    if (f & ESPGPU_ENC_ECN_ALLOWED) {
      if ((itos & 3u) == 3u) otos &= ~1u;
    } else if (!(f & ESPGPU_ENC_ECN_NOCARE)) {
      otos &= ~3u;
    }
#pragma unroll
    for (uint32_t k = 0; k < NW; ++k) w[k] = 0;
    if (p.af6) {                                                                 // :969-984
      w[0] = 0x60u | (otos >> 4) | (otos & 0xfu) << 12;
      w[1] = enc_be16(p.total - 40) | 51u << 16 | (uint32_t)e->ttl << 24;        // :742
#pragma unroll
      for (uint32_t k = 0; k < 4; ++k) {
        w[2 + k] = mem_ld32(e->src + 4 * k);
        w[6 + k] = mem_ld32(e->dst + 4 * k);
      }
    } else {                                                                     // :946-956
      const bool setdf = p.in6 ? (f & kEncDf) != 0                               // :926
                               : (f & ESPGPU_ENC_DF_SET) || ((f & ESPGPU_ENC_DF_COPY) && idf);   // :910-917
      const uint32_t id = (f & ESPGPU_ENC_RFC6864) && setdf ? 0u : ip_id & 0xffffu;   // ip_id.c:252
      w[0] = 0x45u | otos << 8 | enc_be16(p.total) << 16;                        // :727
      w[1] = enc_be16(id) | (setdf ? 0x40u << 16 : 0u);
      w[2] = (uint32_t)e->ttl | 51u << 8;
      w[3] = mem_ld32(e->src);
      w[4] = mem_ld32(e->dst);
      w[2] |= ah_out_cksum<NW>(w) << 16;                                         // ip_output.c:780-782
    }
  } else {
    // 6. transport: the header moves down by ahsize, fixed on the way
    if (p.in6) {
      nxt = (w[1] >> 16) & 0xffu;
      w[1] = (w[1] & 0xff000000u) | 51u << 16 | enc_be16(p.total - 40);          // :742, xform_ah.c:1024
    } else {
      nxt = (w[2] >> 8) & 0xffu;
      w[0] = (w[0] & 0xffffu) | enc_be16(p.total) << 16;                         // :727
      w[2] = (w[2] & 0xffu) | 51u << 8;
      w[2] |= ah_out_cksum<NW>(w) << 16;
    }
  }
  // 8. the wire header into the slot (what ah_output_cb copies back) ...
#pragma unroll
  for (uint32_t k = 0; k < NW; ++k)
    if (k < hn) mem_st32(hsave + 4 * k, w[k]);
  // ... and massaged over the packet (ah_massage_headers, out = 1)
  if (p.af6) {
    w[0] = 0x60u;                                                  // ip6_flow = 0, the version kept (:410-413)
    w[1] &= 0x00ffffffu;                                           // ip6_hlim
    if (enc_linklocal(w[2])) w[2] &= 0x0000ffffu;                  // s6_addr16[1] (:416-419)
    if (enc_linklocal(w[6])) w[6] &= 0x0000ffffu;
  } else {
    if (!(f & ESPGPU_ENC_AH_KEEPTOS)) w[0] &= 0xffff00ffu;         // ip_tos (V_ah_cleartos, :293)
    w[1] &= 0x0000ffffu;                                           // ip_off (:297)
    w[2] &= 0x0000ff00u;                                           // ip_ttl, ip_sum (:295-296)
    if (sr) w[4] = srdst;                                          // :362-365
#pragma unroll
    for (uint32_t k = 5; k < NW; ++k) w[k] &= ~ah_spread4((uint32_t)(zero >> (4 * (k - 5))) & 0xfu);
  }
#pragma unroll
  for (uint32_t k = 0; k < NW; ++k)
    if (k < hn) mem_st32(wire + 4 * k, w[k]);
  // 7. ah_nxt, ah_len, ah_reserve (:925-927); the padding behind the ICV field (:934)
  mem_st32(wire + hs, nxt | ((p.ahsize - 8) / 4) << 8);
  if (p.ahsize > 12 + mlen) mem_st32(wire + hs + 12 + mlen, 0u);
  return 0;
}

// espgpu_ah_encap's rule: status, and on 0 the plan in *p.
ESPGPU_HD inline int ah_encap_rule(const espgpu_encsa *e, uint32_t mlen, uint8_t *pkt, uint32_t len,
                                   uint32_t headroom, uint32_t ip_id, uint8_t *hsave, AhOutPlan *p) {
  const int st = ah_out_plan(e, mlen, pkt, len, headroom, p);
  return st ? st : ah_out_build<15>(e, mlen, pkt, len, ip_id, *p, hsave);
}

// Which records espgpu_ah_frame takes, apart from the SA and the session.
ESPGPU_HD inline bool ah_frame_takes(uint32_t len, uint32_t salt) {
  return len != 0 && salt >= 12 && salt <= len && !(salt & 3);
}

// Sequence numbers the SA may still give out: ah_output always checks
// (xform_ah.c:940-943).
ESPGPU_HD inline uint64_t ah_out_room(uint64_t count, uint32_t oflags) {
  return esp_out_room(count, oflags | ESPGPU_OUT_WRAPCHECK);
}

// ah_spi and ah_seq (:928, :957) of the record whose number is `count`
ESPGPU_HD inline void ah_frame_write(uint8_t *pkt, uint32_t salt, uint32_t spi, uint64_t count) {
  mem_st32(pkt + salt - 8, __builtin_bswap32(spi));
  mem_st32(pkt + salt - 4, __builtin_bswap32((uint32_t)count));
}

// espgpu_ah_frame's rule.
inline int ah_frame_rule(espgpu_outsa *o, uint8_t *pkt, uint32_t len, uint32_t salt, uint32_t *esn_hi) {
  if (!ah_frame_takes(len, salt)) return ESPGPU_EINVAL;
  if (ah_out_room(o->count, o->flags) == 0) return ESPGPU_EACCES;              // :949
  o->count++;                                                                    // :956
  ah_frame_write(pkt, salt, o->spi, o->count);
  *esn_hi = (o->flags & ESPGPU_OUT_ESN) ? (uint32_t)(o->count >> 32) : 0u;       // :1045-1048
  return 0;
}

// espgpu_ah_sent's restore (ah_output_cb, :1120) without the counters: the
// slot's first salt - 12 bytes back over the packet's.
ESPGPU_HD inline int ah_sent_rule(uint32_t eflags, uint8_t *pkt, uint32_t len, uint32_t salt, const uint8_t *hsave) {
  if (salt < 32 || salt > len) return ESPGPU_EINVAL;
  const uint32_t hs = salt - 12, hn = hs / 4;
  const bool af6 = eflags & ESPGPU_ENC_AF6;
  if ((hs & 3) || (af6 ? hs != 40 : hs > 60)) return ESPGPU_EINVAL;
  uint32_t w[15];
#pragma unroll
  for (uint32_t k = 0; k < 15; ++k) w[k] = k < hn ? mem_ld32(hsave + 4 * k) : 0u;
  if (((w[0] >> 4) & 0xfu) != (af6 ? 6u : 4u)) return ESPGPU_EINVAL;
#pragma unroll
  for (uint32_t k = 0; k < 15; ++k)
    if (k < hn) mem_st32(pkt + 4 * k, w[k]);
  return 0;
}

}  // namespace espgpu
