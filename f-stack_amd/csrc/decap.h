// decap.h — the inbound decapsulation rule (include/espgpu.h, the
// decapsulation block): one function pair for espgpu_esp_decap on the host and
// dcp_kernel on the device (decap.hip).
//
// Plain C++ with no HIP header, as classify.h: the host side also builds with
// the host compiler alone (tools/decap_selftest.cpp runs it under its
// sanitizers).
#pragma once
#include <stdint.h>

#include "espgpu.h"
#include "ip_hdr.h"
#include "rule_hd.h"

namespace espgpu {

constexpr uint32_t kInKnown =
    ESPGPU_IN_TRANSPORT | ESPGPU_IN_TUNNEL | ESPGPU_IN_PAD_RAND | ESPGPU_IN_AF6 | ESPGPU_IN_NATT;

// What the rule decides without the packet: checks 1-3, and the result and
// the booked bytes of checks 4 and 5.
struct DecapPlan {
  uint32_t transport;   // 1: the header moves (dcp_transport); 0: tunnel, nothing is touched
  uint32_t off, len;    // the result, relative to the outer header
  uint32_t nxt, q;
};

// Checks 2 and 3 of espgpu_esp_decap: what ipsec4/6_common_input_cb make of
// next header nxt with q bytes behind the stripped header.  Shared with the AH
// decapsulation (ah_in.h).
ESPGPU_HD inline int dcp_mode(uint32_t flags, uint32_t nxt, uint32_t q, bool *tunnel) {
  const uint32_t mode = flags & (ESPGPU_IN_TRANSPORT | ESPGPU_IN_TUNNEL);
  const bool inner4 = nxt == 4 && mode != ESPGPU_IN_TRANSPORT, inner6 = nxt == 41 && mode != ESPGPU_IN_TRANSPORT;
  *tunnel = false;
  if (inner4 || inner6) {                            // ipsec_input.c:334-355, :539-562
    if (q < (inner4 ? 20u : 40u)) return ESPGPU_EINVAL;
    *tunnel = true;
  } else if (!(flags & ESPGPU_IN_AF6) && mode == ESPGPU_IN_TUNNEL) {   // :411-416; ipsec6's protocol loop has no such end
    return ESPGPU_EPFNOSUPPORT;
  }
  return 0;
}

// Checks 1-3 of espgpu_esp_decap.  hlen = 8 + ivlen is the caller's.
ESPGPU_HD inline int dcp_plan(uint32_t flags, uint32_t hlen, uint32_t alen, uint32_t skip, uint32_t rlen,
                              uint32_t trailer, DecapPlan *p) {
  const uint32_t mode = flags & (ESPGPU_IN_TRANSPORT | ESPGPU_IN_TUNNEL);
  const bool af6 = flags & ESPGPU_IN_AF6;
  // a NAT-T SA's skip holds the 8 UDP bytes behind the IP header (udpencap.c:196)
  const uint32_t u = (flags & ESPGPU_IN_NATT) ? 8u : 0u;
  if ((flags & ~kInKnown) || mode == (ESPGPU_IN_TRANSPORT | ESPGPU_IN_TUNNEL) || (u && af6)) return ESPGPU_EINVAL;
  if (skip & 3) return ESPGPU_EINVAL;
  if (af6 ? skip != 40 : (skip < 20 + u || skip > 60 + u)) return ESPGPU_EINVAL;
  if ((uint64_t)rlen < (uint64_t)hlen + alen + 2) return ESPGPU_EINVAL;          // plen < 2
  const uint32_t plen = rlen - hlen - alen;
  if (!(trailer & ESPGPU_TR_VALID)) return ESPGPU_EINVAL;
  if (trailer & ESPGPU_TR_BADLEN) return ESPGPU_EINVAL;                          // xform_esp.c:601-610
  if ((trailer & ESPGPU_TR_BADPAD) && !(flags & ESPGPU_IN_PAD_RAND)) return ESPGPU_EINVAL;   // :613-623
  if (trailer & ESPGPU_TR_NONE) return ESPGPU_ENODATA;                           // :629-630
  const uint32_t nxt = trailer & 0xffu, padlen = (trailer >> 8) & 0xffu;
  if (padlen + 2 > plen) return ESPGPU_EINVAL;       // a word that lacks the BADLEN it should carry
  const uint32_t q = plen - padlen - 2;                                          // m_adj, :633
  bool tunnel;
  if (const int st = dcp_mode(flags, nxt, q, &tunnel)) return st;
  p->transport = !tunnel;
  p->off = tunnel ? skip + hlen : hlen + u;
  p->len = tunnel ? q : skip - u + q;
  p->nxt = nxt;
  p->q = q;
  return 0;
}

// Check 5: the outer header's skip bytes from src to dst + hlen, fixed on the
// way; for a NAT-T SA its skip - 8 bytes to dst + hlen + 8, over the UDP header.  Every dword is loaded before the first is stored: with src == dst the
// ranges overlap whenever hlen < skip.  The loops have constant bounds so that
// the device keeps w[] in registers.
ESPGPU_HD inline int dcp_transport(const uint8_t *src, uint8_t *dst, uint32_t flags, uint32_t hlen, uint32_t skip,
                                   const DecapPlan &p) {
  const uint32_t u = (flags & ESPGPU_IN_NATT) ? 8u : 0u;
  const uint32_t nw = (skip - u) / 4;                // 5 .. 15
  uint32_t w[15];
#pragma unroll
  for (uint32_t k = 0; k < 15; ++k) w[k] = k < nw ? mem_ld32(src + 4 * k) : 0u;
  if (flags & ESPGPU_IN_AF6) {
    if (((w[0] >> 4) & 0xfu) != 6) return ESPGPU_EINVAL;
    // ip6_plen (ipsec_input.c:532), ip6_nxt (xform_esp.c:636); the hop limit stays
    w[1] = (w[1] & 0xff000000u) | p.nxt << 16 | ip_be16(p.q & 0xffffu);
  } else {
    if ((w[0] & 0xffu) != (0x40u | nw)) return ESPGPU_EINVAL;
    w[0] = (w[0] & 0xffffu) | ip_be16((skip - u + p.q) & 0xffffu) << 16;         // ip_len, :312
    w[2] = (w[2] & 0x000000ffu) | p.nxt << 8;                                    // ip_p; ip_sum = 0, :313
    w[2] |= ip_hdr_cksum<15>(w) << 16;                                           // in_cksum, :314
  }
#pragma unroll
  for (uint32_t k = 0; k < 15; ++k)
    if (k < nw) mem_st32(dst + hlen + u + 4 * k, w[k]);
  return 0;
}

// espgpu_esp_decap's rule without the counters: status, and on 0 the result
// in *p (p->len is also what the SA books: m_pkthdr.len at key_sa_recordxfer).
ESPGPU_HD inline int esp_decap_rule(uint32_t flags, uint32_t ivlen, uint32_t alen, const uint8_t *src, uint8_t *dst,
                                    uint32_t skip, uint32_t rlen, uint32_t trailer, DecapPlan *p) {
  const uint32_t hlen = 8 + ivlen;
  int st = dcp_plan(flags, hlen, alen, skip, rlen, trailer, p);
  if (st == 0 && p->transport) st = dcp_transport(src, dst, flags, hlen, skip, *p);
  return st;
}

}  // namespace espgpu
