// encap.h — the outbound encapsulation rule (include/espgpu.h, the
// encapsulation block): one function for espgpu_esp_encap on the host and
// enc_kernel on the device (encap.hip).
//
// Plain C++ with no HIP header, as decap.h and frame.h: the host side also
// builds with the host compiler alone (tools/encap_selftest.cpp runs it under
// its sanitizers).  Packets in the arena are in wire form, so ipsec_encap's
// in6_clearscope (ipsec_output.c:928-929) has nothing to clear.
#pragma once
#include <stdint.h>

#include "espgpu.h"
#include "frame.h"
#include "rule_hd.h"

namespace espgpu {

constexpr uint32_t kEncDf = ESPGPU_ENC_DF_SET | ESPGPU_ENC_DF_COPY;
constexpr uint32_t kEncEcn = ESPGPU_ENC_ECN_ALLOWED | ESPGPU_ENC_ECN_NOCARE;
constexpr uint32_t kEncKnown =
    ESPGPU_ENC_TUNNEL | ESPGPU_ENC_AF6 | kEncDf | kEncEcn | ESPGPU_ENC_RFC6864 | ESPGPU_ENC_NATT;

// a 16-bit value as the big-endian field in one half of a memory-order dword
ESPGPU_HD inline uint32_t enc_be16(uint32_t x) { return ((x & 0xffu) << 8) | ((x >> 8) & 0xffu); }

// in_cksum over w[0..14] (unused dwords zero, the checksum field zero) as the
// memory-order half that goes into the field: the one's-complement sum of the
// 16-bit words is the same in either byte order up to a byte swap
ESPGPU_HD inline uint32_t enc_cksum(const uint32_t *w) {
  uint64_t acc = 0;
#pragma unroll
  for (uint32_t k = 0; k < 15; ++k) acc += w[k];
  acc = (acc & 0xffffffffu) + (acc >> 32);
  acc = (acc & 0xffffu) + ((acc >> 16) & 0xffffu) + (acc >> 32);
  acc = (acc & 0xffffu) + (acc >> 16);
  acc = (acc & 0xffffu) + (acc >> 16);
  return ~(uint32_t)acc & 0xffffu;
}

// first dword of an IPv6 address in fe80::/10 (IN6_IS_SCOPE_LINKLOCAL)
ESPGPU_HD inline bool enc_linklocal(uint32_t a0) { return (a0 & 0xc0ffu) == 0x80feu; }

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
  // 1. the SA
  const uint32_t f = e->flags;
  if ((f & ~kEncKnown) || (f & kEncDf) == kEncDf || (f & kEncEcn) == kEncEcn) return ESPGPU_EINVAL;
  const bool af6 = f & ESPGPU_ENC_AF6;
  // udp_ipsec_output's 8 bytes between the IP and the ESP header
  const uint32_t u = (f & ESPGPU_ENC_NATT) ? 8u : 0u;
  if (u && af6) return ESPGPU_EAFNOSUPPORT;                                      // udpencap.c:222-223
  uint32_t src[4], dst[4];
#pragma unroll
  for (uint32_t k = 0; k < 4; ++k) {
    src[k] = mem_ld32(e->src + 4 * k);
    dst[k] = mem_ld32(e->dst + 4 * k);
  }
  const bool src0 = af6 ? !(src[0] | src[1] | src[2] | src[3]) : !src[0];
  const bool dst0 = af6 ? !(dst[0] | dst[1] | dst[2] | dst[3]) : !dst[0];
  // natt->sport, natt->dport in dst[4..7], as they lie in the UDP header's first dword
  if (u && (src[1] | src[2] | src[3] | dst[2] | dst[3])) return ESPGPU_EINVAL;
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
    skip = 40;                                       // :580, extension headers or not
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
  // 4. lengths
  const uint32_t hlen = 8 + s.ivlen, oh = tunnel ? (af6 ? 40u : 20u) : 0u;
  const uint32_t rlen = tunnel ? len : len - skip, padding = esp_padding(rlen, s.blks);
  const uint32_t reclen = hlen + rlen + padding + s.alen, total = (tunnel ? oh : skip) + reclen;
  if (total > 65535) return ESPGPU_EMSGSIZE;                                     // xform_esp.c:747
  // (the reference would let ip_len wrap, udpencap.c:240: refused deliberately)
  if (total + u > 65535) return ESPGPU_EMSGSIZE;
  // :772-780, :810-818, udpencap.c:227-231
  if (hlen + oh + u > headroom || padding + s.alen > tailroom) return ESPGPU_ENOBUFS;
  const uint32_t ipp = u ? 17u : 50u;                                            // udpencap.c:241
  // the header: 5 .. 15 dwords, all loaded before anything is stored
  const uint32_t nw = skip / 4;
  uint32_t w[15];
#pragma unroll
  for (uint32_t k = 0; k < 15; ++k) w[k] = k < nw ? mem_ld32(pkt + 4 * k) : 0u;
  uint32_t nxt;
  if (tunnel) {
    // 5. the inner header as ipsec4/6_perform_request leave it; only the dwords
    // that hold ip_len and ip_sum, or ip6_plen, are stored
    uint32_t itos, idf;
    if (in6) {
      itos = ((w0 & 0xfu) << 4) | ((w0 >> 12) & 0xfu);                           // ipsec_output.c:925
      idf = 0;
      mem_st32(pkt + 4, (w[1] & 0xffff0000u) | enc_be16(len - 40));              // :533
      nxt = 41;
    } else {
      itos = (w0 >> 8) & 0xffu;
      idf = (w[1] >> 16) & 0x40u;                                                // IP_DF, :916
      w[0] = (w0 & 0xffffu) | enc_be16(len) << 16;                               // :230
      w[2] &= 0xffffu;                                                           // :231
      w[2] |= enc_cksum(w) << 16;                                                // :232
      mem_st32(pkt, w[0]);
      mem_st32(pkt + 8, w[2]);
      nxt = 4;
    }
    // ip_ecn_ingress (ip_ecn.c:97-122)
    uint32_t otos = itos;
    if (f & ESPGPU_ENC_ECN_ALLOWED) {
      if ((itos & 3u) == 3u) otos &= ~1u;                                        // CE: ECT(0) outside
    } else if (!(f & ESPGPU_ENC_ECN_NOCARE)) {
      otos &= ~3u;                                                               // ECN_FORBIDDEN
    }
    uint8_t *oip = pkt - hlen - oh - u;
    if (af6) {                                                                   // :969-984
      mem_st32(oip, 0x60u | (otos >> 4) | (otos & 0xfu) << 12);
      mem_st32(oip + 4, enc_be16(total - 40) | 50u << 16 | (uint32_t)e->ttl << 24);   // :742, xform_esp.c:842
#pragma unroll
      for (uint32_t k = 0; k < 4; ++k) {
        mem_st32(oip + 8 + 4 * k, src[k]);
        mem_st32(oip + 24 + 4 * k, dst[k]);
      }
    } else {                                                                     // :946-956
      const bool setdf = in6 ? (f & kEncDf) != 0                                 // :926
                             : (f & ESPGPU_ENC_DF_SET) || ((f & ESPGPU_ENC_DF_COPY) && idf);   // :910-917
      const uint32_t id = (f & ESPGPU_ENC_RFC6864) && setdf ? 0u : ip_id & 0xffffu;   // ip_id.c:252
      uint32_t h[15];
#pragma unroll
      for (uint32_t k = 5; k < 15; ++k) h[k] = 0;
      h[0] = 0x45u | otos << 8 | enc_be16(total + u) << 16;                      // :727, udpencap.c:240
      h[1] = enc_be16(id) | (setdf ? 0x40u << 16 : 0u);
      h[2] = (uint32_t)e->ttl | ipp << 8;
      h[3] = src[0];
      h[4] = dst[0];
      h[2] |= enc_cksum(h) << 16;                                                // ip_output.c:780-782
#pragma unroll
      for (uint32_t k = 0; k < 5; ++k) mem_st32(oip + 4 * k, h[k]);
      if (u) {                                                                   // udpencap.c:233-237
        mem_st32(oip + 20, dst[1]);
        mem_st32(oip + 24, enc_be16(total + u - 20));                            // uh_ulen; uh_sum = 0
      }
    }
  } else {
    // 6. transport: the header moves down by hlen (+ 8), fixed on the way
    if (in6) {
      nxt = (w[1] >> 16) & 0xffu;
      w[1] = (w[1] & 0xff000000u) | 50u << 16 | enc_be16(total - 40);            // :742, xform_esp.c:842
    } else {
      nxt = (w[2] >> 8) & 0xffu;
      w[0] = (w0 & 0xffffu) | enc_be16(total + u) << 16;                         // :727, udpencap.c:240
      w[2] = (w[2] & 0xffu) | ipp << 8;
      w[2] |= enc_cksum(w) << 16;
    }
#pragma unroll
    for (uint32_t k = 0; k < 15; ++k)
      if (k < nw) mem_st32(pkt - hlen - u + 4 * k, w[k]);
    if (u) {                                                                     // udpencap.c:233-237
      mem_st32(pkt - hlen - 8 + skip, dst[1]);
      mem_st32(pkt - hlen - 4 + skip, enc_be16(total + u - skip));               // uh_ulen; uh_sum = 0
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
