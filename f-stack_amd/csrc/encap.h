// encap.h — the outbound encapsulation rule (include/espgpu.h, the
// encapsulation block): one function for espgpu_esp_encap on the host and
// enc_kernel on the device (encap.hip).  The transport-or-tunnel decision
// (encap_decide) is a function of its own, which the outbound AH rule
// (ah_out.h) takes too; ipsec_encap's header work is three more.
//
// Plain C++ with no HIP header, as decap.h and frame.h: the host side also
// builds with the host compiler alone (tools/encap_selftest.cpp runs it under
// its sanitizers).  Packets in the arena are in wire form, so ipsec_encap's
// in6_clearscope (ipsec_output.c:928-929) has nothing to clear.
#pragma once
#include <stdint.h>

#include "espgpu.h"
#include "frame.h"
#include "ip_hdr.h"
#include "rule_hd.h"

namespace espgpu {

constexpr uint32_t kEncDf = ESPGPU_ENC_DF_SET | ESPGPU_ENC_DF_COPY;
constexpr uint32_t kEncEcn = ESPGPU_ENC_ECN_ALLOWED | ESPGPU_ENC_ECN_NOCARE;
constexpr uint32_t kEncKnown =
    ESPGPU_ENC_TUNNEL | ESPGPU_ENC_AF6 | kEncDf | kEncEcn | ESPGPU_ENC_RFC6864 | ESPGPU_ENC_NATT;

// What checks 1-3 leave: the packet's own header length and the mode.
struct EncapMode {
  uint32_t skip;       // ip_hl * 4, or 40
  bool tunnel, in6, af6;
};

// Checks 1-3 of espgpu_esp_encap and espgpu_ah_encap: the SA, the packet, and
// ipsec4/6_perform_request's transport-or-tunnel decision.  `known` are the
// flags the protocol has, `must` those its SA has to carry and `never` those
// it may not (both EINVAL, as an unknown flag).  Reads the SA's addresses into
// src[] / dst[] and, of the packet, the first dword and (the proxy case) the
// destination address; writes nothing.
ESPGPU_HD inline int encap_decide(const espgpu_encsa *e, uint32_t known, uint32_t must, uint32_t never,
                                  const uint8_t *pkt, uint32_t len, uint32_t src[4], uint32_t dst[4], EncapMode *m) {
  // 1. the SA
  const uint32_t f = e->flags;
  if ((f & ~known) || (f & kEncDf) == kEncDf || (f & kEncEcn) == kEncEcn) return ESPGPU_EINVAL;
  if ((f & must) != must || (f & never)) return ESPGPU_EINVAL;
  const bool af6 = f & ESPGPU_ENC_AF6;
  const bool natt = f & ~never & ESPGPU_ENC_NATT;    // (a constant where the protocol has no NAT-T)
  if (natt && af6) return ESPGPU_EAFNOSUPPORT;                                   // udpencap.c:222-223
#pragma unroll
  for (uint32_t k = 0; k < 4; ++k) {
    src[k] = mem_ld32(e->src + 4 * k);
    dst[k] = mem_ld32(e->dst + 4 * k);
  }
  const bool src0 = af6 ? !(src[0] | src[1] | src[2] | src[3]) : !src[0];
  const bool dst0 = af6 ? !(dst[0] | dst[1] | dst[2] | dst[3]) : !dst[0];
  // natt->sport, natt->dport in dst[4..7], as they lie in the UDP header's first dword
  if (natt && (src[1] | src[2] | src[3] | dst[2] | dst[3])) return ESPGPU_EINVAL;
  if (af6) {
    if (src0 || dst0) return ESPGPU_EINVAL;                                      // ipsec_output.c:961-964
    if (ip6_linklocal(src[0]) || ip6_linklocal(dst[0])) return ESPGPU_ENOTSUP;   // :975-981 is the host's
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
  // the reference answers ENXIO for an IPv6 inner packet here (:548-552) and
  // does not look for IPv4: one code for both, deliberately
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
  m->skip = skip;
  m->tunnel = tunnel;
  m->in6 = in6;
  m->af6 = af6;
  return 0;
}

// The steps below work on the header in w[0..NW), NW a constant: the loops have
// constant bounds so that the device keeps w[] in registers and never indexes
// it by a variable.

// Step 5, tunnel: the inner header in w[] as ipsec4/6_perform_request leave it;
// only the dwords that hold ip_len and ip_sum, or ip6_plen, are stored.
// Returns the outer next header; *itos and *idf are the inner TOS / traffic
// class and IP_DF.
template <uint32_t NW>
ESPGPU_HD inline uint32_t encap_inner_fix(uint32_t *w, uint8_t *pkt, uint32_t len, bool in6, uint32_t *itos,
                                          uint32_t *idf) {
  if (in6) {
    *itos = ((w[0] & 0xfu) << 4) | ((w[0] >> 12) & 0xfu);                        // ipsec_output.c:925
    *idf = 0;
    mem_st32(pkt + 4, (w[1] & 0xffff0000u) | ip_be16(len - 40));                 // :533
    return 41;
  }
  *itos = (w[0] >> 8) & 0xffu;
  *idf = (w[1] >> 16) & 0x40u;                                                   // IP_DF, :916
  w[0] = (w[0] & 0xffffu) | ip_be16(len) << 16;                                  // :230
  w[2] &= 0xffffu;                                                               // :231
  w[2] |= ip_hdr_cksum<NW>(w) << 16;                                             // :232
  mem_st32(pkt, w[0]);
  mem_st32(pkt + 8, w[2]);
  return 4;
}

// Where encap_outer_header takes the SA's addresses from: the registers that
// encap_decide filled, or the SA itself (loaded where the header needs them:
// one dword each for IPv4, four for IPv6).
struct EncapAddrRegs {
  const uint32_t *s, *d;
  ESPGPU_HD uint32_t src(uint32_t k) const { return s[k]; }
  ESPGPU_HD uint32_t dst(uint32_t k) const { return d[k]; }
};
struct EncapAddrSa {
  const espgpu_encsa *e;
  ESPGPU_HD uint32_t src(uint32_t k) const { return mem_ld32(e->src + 4 * k); }
  ESPGPU_HD uint32_t dst(uint32_t k) const { return mem_ld32(e->dst + 4 * k); }
};

// Step 5, tunnel: ipsec_encap's outer header into w[] (5 or 10 dwords, the
// rest zero) for protocol `proto` and a wire packet of `total` bytes.
template <uint32_t NW, class Addr>
ESPGPU_HD inline void encap_outer_header(uint32_t *w, uint32_t f, const uint8_t *ttl, const Addr &a, bool af6, bool in6,
                                         uint32_t itos, uint32_t idf, uint32_t proto, uint32_t total,
                                         uint32_t ip_id) {
  const uint32_t otos = ip_ecn_ingress(f, itos);
#pragma unroll
  for (uint32_t k = 0; k < NW; ++k) w[k] = 0;
  if (af6) {                                                                     // :969-984
    w[0] = 0x60u | (otos >> 4) | (otos & 0xfu) << 12;
    w[1] = ip_be16(total - 40) | proto << 16 | (uint32_t)*ttl << 24;          // :742
#pragma unroll
    for (uint32_t k = 0; k < 4; ++k) {
      w[2 + k] = a.src(k);
      w[6 + k] = a.dst(k);
    }
  } else {                                                                       // :946-956
    const bool setdf = in6 ? (f & kEncDf) != 0                                   // :926
                           : (f & ESPGPU_ENC_DF_SET) || ((f & ESPGPU_ENC_DF_COPY) && idf);   // :910-917
    const uint32_t id = (f & ESPGPU_ENC_RFC6864) && setdf ? 0u : ip_id & 0xffffu;   // ip_id.c:252
    w[0] = 0x45u | otos << 8 | ip_be16(total) << 16;                             // :727, udpencap.c:240
    w[1] = ip_be16(id) | (setdf ? 0x40u << 16 : 0u);
    w[2] = (uint32_t)*ttl | proto << 8;
    w[3] = a.src(0);
    w[4] = a.dst(0);
    w[2] |= ip_hdr_cksum<NW>(w) << 16;                                           // ip_output.c:780-782
  }
}

// Step 6, transport: the packet's own header in w[] with the protocol field,
// the length and the checksum of the wire packet.  Returns the next header it
// had.
template <uint32_t NW>
ESPGPU_HD inline uint32_t encap_transport_fix(uint32_t *w, bool in6, uint32_t proto, uint32_t total) {
  if (in6) {
    const uint32_t nxt = (w[1] >> 16) & 0xffu;
    w[1] = (w[1] & 0xff000000u) | proto << 16 | ip_be16(total - 40);             // :742
    return nxt;
  }
  const uint32_t nxt = (w[2] >> 8) & 0xffu;
  w[0] = (w[0] & 0xffffu) | ip_be16(total) << 16;                                // :727, udpencap.c:240
  w[2] = (w[2] & 0xffu) | proto << 8;
  w[2] |= ip_hdr_cksum<NW>(w) << 16;
  return nxt;
}

// The result of an accepted packet (check 7).
struct EncapOut {
  uint32_t front;      // hlen + oh (+ 8 for a NAT-T SA): the wire packet starts that far before pkt
  uint32_t total;      // the wire packet's length
  uint32_t reclen;     // the ESP record's: the wire packet's last bytes
  uint32_t frame;      // rlen | next header << 16
};

// espgpu_esp_encap's rule.  A usable shape (ivlen 0 / 8 / 16, blks 4 / 16,
// alen <= 0xffff) is the caller's check.  The loops have constant bounds so
// that the device keeps w[] in registers.
ESPGPU_HD inline int esp_encap_rule(const espgpu_encsa *e, const espgpu_eshape &s, uint8_t *pkt, uint32_t len,
                                    uint32_t headroom, uint32_t tailroom, uint32_t ip_id, EncapOut *o) {
  // 1.-3.
  uint32_t src[4], dst[4];
  EncapMode m;
  if (const int st = encap_decide(e, kEncKnown, 0, 0, pkt, len, src, dst, &m)) return st;
  const uint32_t skip = m.skip;
  const bool tunnel = m.tunnel;
  // udp_ipsec_output's 8 bytes between the IP and the ESP header
  const uint32_t f = e->flags, u = (f & ESPGPU_ENC_NATT) ? 8u : 0u;
  // 4. lengths
  const uint32_t hlen = 8 + s.ivlen, oh = tunnel ? (m.af6 ? 40u : 20u) : 0u;
  const uint32_t rlen = tunnel ? len : len - skip, padding = esp_padding(rlen, s.blks);
  const uint32_t reclen = hlen + rlen + padding + s.alen, total = (tunnel ? oh : skip) + reclen;
  if (total > 65535) return ESPGPU_EMSGSIZE;                                     // xform_esp.c:747
  // (the reference would let ip_len wrap, udpencap.c:240: refused deliberately)
  if (total + u > 65535) return ESPGPU_EMSGSIZE;
  // :772-780, :810-818, udpencap.c:227-231
  if (hlen + oh + u > headroom || padding + s.alen > tailroom) return ESPGPU_ENOBUFS;
  const uint32_t ipp = u ? 17u : 50u;                                            // udpencap.c:241, xform_esp.c:842
  // the header: 5 .. 15 dwords, all loaded before anything is stored
  const uint32_t nw = skip / 4;
  uint32_t w[15];
#pragma unroll
  for (uint32_t k = 0; k < 15; ++k) w[k] = k < nw ? mem_ld32(pkt + 4 * k) : 0u;
  uint32_t nxt;
  if (tunnel) {
    // 5. the inner header fixed in place, the outer one in front of it
    uint32_t itos, idf, h[10];
    nxt = encap_inner_fix<15>(w, pkt, len, m.in6, &itos, &idf);
    encap_outer_header<10>(h, f, &e->ttl, EncapAddrRegs{src, dst}, m.af6, m.in6, itos, idf, ipp, total + u, ip_id);
    uint8_t *oip = pkt - hlen - oh - u;
#pragma unroll
    for (uint32_t k = 0; k < 10; ++k)
      if (k < oh / 4) mem_st32(oip + 4 * k, h[k]);
    if (u) {                                                                     // udpencap.c:233-237
      mem_st32(oip + 20, dst[1]);
      mem_st32(oip + 24, ip_be16(total + u - 20));                               // uh_ulen; uh_sum = 0
    }
  } else {
    // 6. transport: the header moves down by hlen (+ 8), fixed on the way
    nxt = encap_transport_fix<15>(w, m.in6, ipp, total + u);
#pragma unroll
    for (uint32_t k = 0; k < 15; ++k)
      if (k < nw) mem_st32(pkt - hlen - u + 4 * k, w[k]);
    if (u) {                                                                     // udpencap.c:233-237
      mem_st32(pkt - hlen - 8 + skip, dst[1]);
      mem_st32(pkt - hlen - 4 + skip, ip_be16(total + u - skip));                // uh_ulen; uh_sum = 0
    }
  }
  // 7.
  o->front = hlen + oh + u;
  o->total = total + u;
  o->reclen = reclen;
  o->frame = rlen | nxt << 16;
  return 0;
}

}  // namespace espgpu
