// ah_in.h — the inbound AH rules (include/espgpu.h, the inbound AH block): one
// function pair for espgpu_ah_input and espgpu_ah_decap on the host and for
// ahi_kernel and ahd_kernel on the device (ah_in.hip).  ah_input's length
// checks and ah_massage_headers with out = 0 (xform_ah.c:576-600, :261-525),
// then ah_input_cb's restore and strip (:758-791) in front of decap.h's mode
// logic and header fix.
//
// Plain C++ with no HIP header, as classify.h and decap.h: the host side also
// builds with the host compiler alone (tools/ah_in_selftest.cpp runs it under
// its sanitizers).
#pragma once
#include <stdint.h>

#include "decap.h"
#include "espgpu.h"
#include "ip_hdr.h"
#include "rule_hd.h"

namespace espgpu {

constexpr uint32_t kAhInKnown =
    ESPGPU_IN_TRANSPORT | ESPGPU_IN_TUNNEL | ESPGPU_IN_AF6 | ESPGPU_IN_AH | ESPGPU_IN_AH_KEEPTOS;
constexpr uint32_t kAhSaveSlot = 64;                 // bytes of d_hsave per record: an IPv4 header with all its options fits

// an ICV length the ABI allows
ESPGPU_HD inline bool ah_mlen_usable(uint32_t mlen) { return mlen >= 4 && mlen <= 64 && !(mlen & 3); }

// ah_hdrsiz (xform_ah.c:144-169): struct newah and the ICV, rounded up to 4
// (RFC 4302) or, for an IPv6 SA, to 8.
ESPGPU_HD inline uint32_t ah_hdrsiz(uint32_t mlen, bool af6) {
  const uint32_t align = af6 ? 8u : 4u;
  return (12u + mlen + align - 1) & ~(align - 1);
}

// What both rules ask of the SA and the descriptor before they read the
// packet: the flag, skip and length rows of espgpu_ah_input's check 1.
ESPGPU_HD inline bool ah_shape_ok(uint32_t flags, uint32_t len, uint32_t salt) {
  const uint32_t mode = flags & (ESPGPU_IN_TRANSPORT | ESPGPU_IN_TUNNEL);
  if (!(flags & ESPGPU_IN_AH) || (flags & ~kAhInKnown) || mode == (ESPGPU_IN_TRANSPORT | ESPGPU_IN_TUNNEL))
    return false;
  if (salt < 32) return false;
  const uint32_t skip = salt - 12;
  if (skip & 3) return false;
  if ((flags & ESPGPU_IN_AF6) ? skip != 40 : skip > 60) return false;
  return (uint64_t)len >= (uint64_t)skip + 12;
}

// Checks 1 and 2 of espgpu_ah_input.  Reads the packet's first dword and the
// AH header's, both inside len once ah_shape_ok has passed.
ESPGPU_HD inline int ah_in_plan(uint32_t flags, uint32_t mlen, const uint8_t *pkt, uint32_t len, uint32_t salt) {
  if (!ah_shape_ok(flags, len, salt)) return ESPGPU_EINVAL;
  const uint32_t skip = salt - 12;
  const bool af6 = flags & ESPGPU_IN_AF6;
  const uint32_t vhl = mem_ld32(pkt) & 0xffu;
  if (af6 ? (vhl >> 4) != 6 : vhl != (0x40u | skip / 4)) return ESPGPU_EINVAL;
  const uint32_t ahsize = ah_hdrsiz(mlen, af6), ah_len = (mem_ld32(pkt + skip) >> 8) & 0xffu;
  if (8 + ah_len * 4 != ahsize) return ESPGPU_EACCES;              // xform_ah.c:581
  if ((uint64_t)skip + ahsize > len) return ESPGPU_EACCES;         // :591
  return 0;
}

// The IPv4 option loop of ah_massage_headers (xform_ah.c:302-393) over the
// bytes [20, skip) of pkt: status, and on 0 bit j of *zero is set for every
// option byte 20 + j that the massage zeroes.  The loop never reads a byte it
// has zeroed, so it runs on the packet as it arrived and writes nothing.
// OUT is the reference's `out`: the outbound walk also reports whether a
// source-route option was seen and the last four bytes of the last one (the
// hashed ip_dst, :362-365) as a memory-order dword, and refuses one shorter
// than 4 bytes (a deliberate difference: its "last address" would start in
// front of the option).  The inbound walk does neither.
template <bool OUT>
ESPGPU_HD inline int ah_opt_walk(const uint8_t *pkt, uint32_t skip, uint64_t *zero, bool *sr = nullptr,
                                 uint32_t *srdst = nullptr) {
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
    if constexpr (OUT) {
      if (o == 0x83 || o == 0x89) {                                // IPOPT_LSRR, IPOPT_SSRR
        if (count < 4) return ESPGPU_EINVAL;
        const uint8_t *q = pkt + off + count - 4;
        last = (uint32_t)q[0] | (uint32_t)q[1] << 8 | (uint32_t)q[2] << 16 | (uint32_t)q[3] << 24;
        seen = true;
      }
    }
    if (!keep) z |= ((1ull << count) - 1) << (off - 20);           // count <= 40 here
    off += count;
  }
  *zero = z;
  if constexpr (OUT) {
    *sr = seen;
    *srdst = last;
  }
  return 0;
}

// a 4-bit byte mask spread to the dword's bytes
ESPGPU_HD inline uint32_t ah_spread4(uint32_t m) {
  return ((m & 1u) ? 0x000000ffu : 0u) | ((m & 2u) ? 0x0000ff00u : 0u) | ((m & 4u) ? 0x00ff0000u : 0u) |
         ((m & 8u) ? 0xff000000u : 0u);
}

// ah_massage_headers on the header in w[0..NW): the mutable fields zeroed
// (:291-300, :404-419), the option bytes of `zero` too, and, outbound, the
// destination replaced by a source route's last address.  The loop has a
// constant bound so that the device keeps w[] in registers.
template <uint32_t NW>
ESPGPU_HD inline void ah_massage(uint32_t *w, bool af6, bool keeptos, uint64_t zero, bool sr = false,
                                 uint32_t srdst = 0) {
  if (af6) {
    w[0] = 0x60u;                                                  // ip6_flow = 0, the version kept (:410-413)
    w[1] &= 0x00ffffffu;                                           // ip6_hlim
    if (ip6_linklocal(w[2])) w[2] &= 0x0000ffffu;                  // s6_addr16[1] of a link-local source (:416-419)
    if (ip6_linklocal(w[6])) w[6] &= 0x0000ffffu;                  // ... destination
  } else {
    if (!keeptos) w[0] &= 0xffff00ffu;                             // ip_tos (V_ah_cleartos, :293)
    w[1] &= 0x0000ffffu;                                           // ip_off (:297)
    w[2] &= 0x0000ff00u;                                           // ip_ttl, ip_sum (:295-296)
    if (sr) w[4] = srdst;                                          // :362-365
#pragma unroll
    for (uint32_t k = 5; k < NW; ++k) w[k] &= ~ah_spread4((uint32_t)(zero >> (4 * (k - 5))) & 0xfu);
  }
}

// Checks 3 and 4 of espgpu_ah_input, after ah_in_plan returned 0.  NW is the
// number of header dwords the caller provides registers for: 10 serves every
// header without IPv4 options (5 dwords, or IPv6's 10) and leaves the option
// loop out; 15 serves all.  skip / 4 <= NW is the caller's.  The loops have
// constant bounds so that the device keeps w[] in registers; the option loop
// reads the packet's bytes, not w[], for the same reason.
template <uint32_t NW>
ESPGPU_HD inline int ah_in_massage(uint32_t flags, uint8_t *pkt, uint32_t skip, uint8_t *hsave) {
  const uint32_t nw = skip / 4;
  uint32_t w[NW];
#pragma unroll
  for (uint32_t k = 0; k < NW; ++k) w[k] = k < nw ? mem_ld32(pkt + 4 * k) : 0u;
  uint64_t zero = 0;
  if (flags & ESPGPU_IN_AF6) {
    if ((w[1] & 0xffffu) == 0) return ESPGPU_EMSGSIZE;             // ip6_plen == 0, xform_ah.c:404
  } else if (NW > 10) {
    if (const int st = ah_opt_walk<false>(pkt, skip, &zero)) return st;
  }
  // the header as it arrived (the front of xform_data, :632)
#pragma unroll
  for (uint32_t k = 0; k < NW; ++k)
    if (k < nw) mem_st32(hsave + 4 * k, w[k]);
  ah_massage<NW>(w, flags & ESPGPU_IN_AF6, flags & ESPGPU_IN_AH_KEEPTOS, zero);
#pragma unroll
  for (uint32_t k = 0; k < NW; ++k)
    if (k < nw) mem_st32(pkt + 4 * k, w[k]);
  return 0;
}

// espgpu_ah_input's rule.
ESPGPU_HD inline int ah_input_rule(uint32_t flags, uint32_t mlen, uint8_t *pkt, uint32_t len, uint32_t salt,
                                   uint8_t *hsave) {
  const int st = ah_in_plan(flags, mlen, pkt, len, salt);
  return st ? st : ah_in_massage<15>(flags, pkt, salt - 12, hsave);
}

// espgpu_ah_decap's rule without the counters: status, and on 0 the result in
// *p (p->len is also what the SA books).  The saved header travels through
// dcp_transport, which sets the protocol field, the length and the checksum
// and refuses a header that does not agree with skip.
ESPGPU_HD inline int ah_decap_rule(uint32_t flags, uint32_t mlen, uint8_t *pkt, uint32_t len, uint32_t salt,
                                   const uint8_t *hsave, DecapPlan *p) {
  if (!ah_shape_ok(flags, len, salt)) return ESPGPU_EINVAL;
  const uint32_t skip = salt - 12, ahsize = ah_hdrsiz(mlen, flags & ESPGPU_IN_AF6);
  if ((uint64_t)len < (uint64_t)skip + ahsize) return ESPGPU_EINVAL;
  const uint32_t nxt = mem_ld32(pkt + skip) & 0xffu, q = len - skip - ahsize;    // ah_nxt (:638), m_striphdr (:791)
  bool tunnel;
  if (const int st = dcp_mode(flags, nxt, q, &tunnel)) return st;
  p->transport = !tunnel;
  p->off = tunnel ? skip + ahsize : ahsize;
  p->len = tunnel ? q : skip + q;
  p->nxt = nxt;
  p->q = q;
  return tunnel ? 0 : dcp_transport(hsave, pkt, flags & ESPGPU_IN_AF6, ahsize, skip, *p);
}

}  // namespace espgpu
