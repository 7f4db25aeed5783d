// natt.h — the NAT-T checksum fix's rule (include/espgpu.h, the NAT-T block):
// udp_ipsec_adjust_cksum (udpencap.c:245-293) with in_delayed_cksum
// (ip_output.c:1059-1091), one set of functions for espgpu_esp_natt_cksum on
// the host and the two kernels of natt.hip.
//
// Plain C++ with no HIP header, as decap.h: the host side also builds with the
// host compiler alone (tools/natt_selftest.cpp runs it under its sanitizers).
//
// All sums are over memory-order dwords: the one's-complement sum of the
// 16-bit words is the same in either byte order up to a byte swap, so a sum of
// memory-order halves goes back into a memory-order half (ip_hdr.h's fold),
// and sav->natt->cksum is kept as the value the reference adds to the field's
// two bytes as they lie in memory.
#pragma once
#include <stdint.h>

#include "espgpu.h"
#include "ip_hdr.h"
#include "rule_hd.h"

namespace espgpu {

// Lanes per packet of the recompute kernel.  16: four packets per wave, a
// group step covers 256 contiguous bytes.  The choice was made unmeasured;
// tools/natt_bench.py has since run (at 1500-byte packets 8
// lanes measured 7-9 % faster, 32 lanes about 40 % slower), and the default
// stays until that is repeated at other packet sizes.
constexpr uint32_t kNattLanes = 16;

// in_addword (in_cksum.c:174-181)
ESPGPU_HD inline uint32_t natt_addword(uint32_t a, uint32_t b) {
  uint32_t sum = a + b;
  if (sum > 65535) sum -= 65535;
  return sum;
}

// Where the fix works in a packet that takes part.
struct NattPlan {
  uint32_t ihl;      // the transport header starts here: ip_hl * 4
  uint32_t proto;    // 6 or 17
  uint32_t fat;      // byte offset of the checksum field: ihl + 16 (TCP) or ihl + 6 (UDP)
  uint32_t cklen;    // recompute: bytes summed from ihl on
  uint32_t pseudo;   // recompute: in_pseudo(src, dst, htons(len - ihl + proto))
};

// The checksum field's two bytes in memory order.  The device accesses the
// aligned dword that holds them: the field is 2-byte aligned in a 4-byte
// aligned packet, and a dword that holds the field holds only bytes of the
// packet's own record.  The host touches the two bytes alone.
ESPGPU_HD inline uint32_t natt_ld_field(const uint8_t *pkt, uint32_t fat) {
#ifdef __HIP_DEVICE_COMPILE__
  return (mem_ld32(pkt + (fat & ~3u)) >> ((fat & 2u) * 8)) & 0xffffu;
#else
  return (uint32_t)pkt[fat] | (uint32_t)pkt[fat + 1] << 8;
#endif
}
ESPGPU_HD inline void natt_st_field(uint8_t *pkt, uint32_t fat, uint32_t v) {
#ifdef __HIP_DEVICE_COMPILE__
  uint8_t *at = pkt + (fat & ~3u);
  const uint32_t sh = (fat & 2u) * 8;
  mem_st32(at, (mem_ld32(at) & ~(0xffffu << sh)) | (v & 0xffffu) << sh);
#else
  pkt[fat] = (uint8_t)v;
  pkt[fat + 1] = (uint8_t)(v >> 8);
#endif
}

// Does the packet of `len` bytes at pkt, whose trailer said `proto`, take part
// under `policy`, and where?  Reads the IP header's first, fourth and fifth
// dword and, for UDP under recompute, uh_ulen.
ESPGPU_HD inline bool natt_plan(const uint8_t *pkt, uint32_t len, uint32_t proto, uint32_t policy, NattPlan *p) {
  if (proto != 6 && proto != 17) return false;
  if (len < 20 || len > 65535) return false;
  const uint32_t w0 = mem_ld32(pkt);
  const uint32_t ihl = (w0 & 0xfu) * 4;
  if ((w0 & 0xf0u) != 0x40u || ihl < 20 || ihl > len) return false;
  const uint32_t seg = len - ihl, foff = proto == 6 ? 16u : 6u;
  if (seg < foff + 2) return false;                    // no room for the field: left alone
  p->ihl = ihl;
  p->proto = proto;
  p->fat = ihl + foff;
  p->cklen = 0;
  p->pseudo = 0;
  if (policy == 0) return true;
  if (proto == 17) {                                   // ip_output.c:1068-1078
    const uint32_t ulen = ip_be16(mem_ld32(pkt + ihl + 4));
    // the reference would sum past the mbuf (or sum nothing the field is in): left alone
    if (ulen < 8 || ulen > seg) return false;
    p->cklen = ulen;
  } else {                                             // :1082-1083: ip_len - offset
    const uint32_t ip_len = ((w0 >> 8) & 0xff00u) | (w0 >> 24);
    if (ip_len != len) return false;                   // (decapsulation leaves ip_len == len)
    p->cklen = seg;
  }
  // in_pseudo's three addends (udpencap.c:284-285); folded with the rest
  const uint64_t ps = (uint64_t)mem_ld32(pkt + 12) + mem_ld32(pkt + 16) + ip_be16(seg + proto);
  p->pseudo = ip_fold16(ps);
  return true;
}

// Policy auto (udpencap.c:261-281).  Returns the packet's cflags.
ESPGPU_HD inline uint32_t natt_auto(uint8_t *pkt, const NattPlan &p, uint32_t delta) {
  delta &= 0xffffu;
  if (delta != 0) {
    const uint32_t cksum = natt_ld_field(pkt, p.fat);
    if (p.proto == 17 && cksum == 0) return 0;         // :267-268
    natt_st_field(pkt, p.fat, natt_addword(cksum, delta));
    return 0;
  }
  if (p.proto == 6) return ESPGPU_NATT_CSUM_VALID;     // :272-278
  natt_st_field(pkt, p.fat, 0);                        // :279
  return 0;
}

// Dword k of the summed span in memory order, the bytes past cklen as zeros
// (in_masks, in_cksum.c:75-81, :168-169).  The device loads the aligned dword,
// which holds at least one byte of the span; the host loads the span's bytes
// alone.
ESPGPU_HD inline uint32_t natt_dword(const uint8_t *seg, uint32_t k, uint32_t cklen) {
  const uint32_t rem = cklen - 4 * k;                  // >= 1
#ifdef __HIP_DEVICE_COMPILE__
  const uint32_t w = mem_ld32(seg + 4 * k);
  return rem >= 4 ? w : w & ((1u << (8 * rem)) - 1u);
#else
  uint32_t w = 0;
  for (uint32_t b = 0; b < (rem < 4 ? rem : 4u); ++b) w |= (uint32_t)seg[4 * k + b] << (8 * b);
  return w;
#endif
}

// Policy recompute, the end (udpencap.c:284-292, ip_output.c:1078-1090): `sum`
// is the span's dwords added up (natt_dword; any partial folding of it is
// fine), the field as it stood among them.  The reference stores in_pseudo's
// value into the field and sums then: here the field's old value leaves the
// sum as its one's complement, which no fold can bring to 0 beside a nonzero
// pseudo-header sum, so 0x0000 and 0xffff come out as the reference's do.
ESPGPU_HD inline void natt_finish(uint8_t *pkt, const NattPlan &p, uint64_t sum) {
  const uint32_t old = natt_ld_field(pkt, p.fat);
  uint32_t csum = ~ip_fold16((uint64_t)ip_fold16(sum) + p.pseudo + (0xffffu - old)) & 0xffffu;
  if (p.proto == 17 && csum == 0) csum = 0xffffu;      // ip_output.c:1079-1080
  natt_st_field(pkt, p.fat, csum);
}

// espgpu_esp_natt_cksum's rule for one packet that belongs to a NAT-T SA.
ESPGPU_HD inline uint32_t natt_cksum_rule(uint8_t *pkt, uint32_t len, uint32_t proto, uint32_t policy,
                                          uint32_t delta) {
  NattPlan p;
  if (!natt_plan(pkt, len, proto, policy, &p)) return 0;
  if (policy == 0) return natt_auto(pkt, p, delta);
  uint64_t sum = 0;
  for (uint32_t k = 0; 4 * k < p.cklen; ++k) sum += natt_dword(pkt + p.ihl, k, p.cklen);
  natt_finish(pkt, p, sum);
  return 0;
}

}  // namespace espgpu
