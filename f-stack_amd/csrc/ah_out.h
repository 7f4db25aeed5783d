// ah_out.h — the outbound AH rules (include/espgpu.h, the outbound AH block):
// one set of functions for espgpu_ah_encap, espgpu_ah_frame and espgpu_ah_sent
// on the host and for aho_kernel, the numbering kernels (sa_group.h over AhfRule) and ahs_kernel on the
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
  if (!ah_mlen_usable(mlen)) return ESPGPU_EINVAL;
  // 1.-3.; key.c:5702: NAT-T is ESP's alone
  uint32_t src[4], dst[4];
  EncapMode m;
  if (const int st = encap_decide(e, kAhOutKnown, ESPGPU_ENC_AH, ESPGPU_ENC_NATT, pkt, len, src, dst, &m)) return st;
  // 4. lengths
  const uint32_t ahsize = ah_hdrsiz(mlen, m.af6), oh = m.tunnel ? (m.af6 ? 40u : 20u) : 0u;
  const uint32_t total = len + ahsize + oh;
  if (total > 65535) return ESPGPU_EMSGSIZE;                                     // xform_ah.c:882
  if (ahsize + oh > headroom) return ESPGPU_ENOBUFS;                             // m_makespace, :907
  p->skip = m.skip;
  p->oh = oh;
  p->ahsize = ahsize;
  p->total = total;
  p->tunnel = m.tunnel;
  p->in6 = m.in6;
  p->af6 = m.af6;
  return 0;
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
    if (const int st = ah_opt_walk<true>(pkt, p.skip, &zero, &sr, &srdst)) return st;
  }
  const uint32_t hs = p.tunnel ? p.oh : p.skip, hn = hs / 4;
  uint8_t *const wire = pkt - p.ahsize - p.oh;
  uint32_t nxt;
  if (p.tunnel) {
    // 5. the inner header as ipsec4/6_perform_request leave it, then the outer
    // header takes the registers.  Steps 5 and 6 stay written out here, not as
    // calls of encap.h's encap_inner_fix / encap_outer_header /
    // encap_transport_fix: with the calls aho_kernel measured 15-25 % slower
    // (profiles/stage_rules_shared_ab.txt).
    uint32_t itos, idf;
    if (p.in6) {
      itos = ((w[0] & 0xfu) << 4) | ((w[0] >> 12) & 0xfu);                       // ipsec_output.c:925
      idf = 0;
      mem_st32(pkt + 4, (w[1] & 0xffff0000u) | ip_be16(len - 40));               // :533
      nxt = 41;
    } else {
      itos = (w[0] >> 8) & 0xffu;
      idf = (w[1] >> 16) & 0x40u;                                                // IP_DF, :916
      w[0] = (w[0] & 0xffffu) | ip_be16(len) << 16;                              // :230
      w[2] &= 0xffffu;                                                           // :231
      w[2] |= ip_hdr_cksum<NW>(w) << 16;                                         // :232
      mem_st32(pkt, w[0]);
      mem_st32(pkt + 8, w[2]);
      nxt = 4;
    }
    const uint32_t otos = ip_ecn_ingress(f, itos);
#pragma unroll
    for (uint32_t k = 0; k < NW; ++k) w[k] = 0;
    if (p.af6) {                                                                 // :969-984
      w[0] = 0x60u | (otos >> 4) | (otos & 0xfu) << 12;
      w[1] = ip_be16(p.total - 40) | 51u << 16 | (uint32_t)e->ttl << 24;         // :742
#pragma unroll
      for (uint32_t k = 0; k < 4; ++k) {
        w[2 + k] = mem_ld32(e->src + 4 * k);
        w[6 + k] = mem_ld32(e->dst + 4 * k);
      }
    } else {                                                                     // :946-956
      const bool setdf = p.in6 ? (f & kEncDf) != 0                               // :926
                               : (f & ESPGPU_ENC_DF_SET) || ((f & ESPGPU_ENC_DF_COPY) && idf);   // :910-917
      const uint32_t id = (f & ESPGPU_ENC_RFC6864) && setdf ? 0u : ip_id & 0xffffu;   // ip_id.c:252
      w[0] = 0x45u | otos << 8 | ip_be16(p.total) << 16;                         // :727
      w[1] = ip_be16(id) | (setdf ? 0x40u << 16 : 0u);
      w[2] = (uint32_t)e->ttl | 51u << 8;
      w[3] = mem_ld32(e->src);
      w[4] = mem_ld32(e->dst);
      w[2] |= ip_hdr_cksum<NW>(w) << 16;                                         // ip_output.c:780-782
    }
  } else {
    // 6. transport: the header moves down by ahsize, fixed on the way
    if (p.in6) {
      nxt = (w[1] >> 16) & 0xffu;
      w[1] = (w[1] & 0xff000000u) | 51u << 16 | ip_be16(p.total - 40);           // :742, xform_ah.c:1024
    } else {
      nxt = (w[2] >> 8) & 0xffu;
      w[0] = (w[0] & 0xffffu) | ip_be16(p.total) << 16;                          // :727
      w[2] = (w[2] & 0xffu) | 51u << 8;
      w[2] |= ip_hdr_cksum<NW>(w) << 16;
    }
  }
  // 8. the wire header into the slot (what ah_output_cb copies back) ...
#pragma unroll
  for (uint32_t k = 0; k < NW; ++k)
    if (k < hn) mem_st32(hsave + 4 * k, w[k]);
  // ... and massaged over the packet (ah_massage_headers, out = 1)
  ah_massage<NW>(w, p.af6, f & ESPGPU_ENC_AH_KEEPTOS, zero, sr, srdst);
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
