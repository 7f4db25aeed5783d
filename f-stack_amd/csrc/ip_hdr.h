// ip_hdr.h — what the rule headers (classify.h, decap.h, encap.h, ah_in.h,
// ah_out.h, natt.h) share about an IP header held as memory-order dwords: a
// 16-bit field, the header checksum, the link-local test and the tunnel's ECN
// rule.  Plain C++ with no HIP header, as rule_hd.h.
#pragma once
#include <stdint.h>

#include "espgpu.h"
#include "rule_hd.h"

namespace espgpu {

// a 16-bit value as the big-endian field in the low half of a memory-order
// dword (htons); its own inverse, so also such a field's value
ESPGPU_HD inline uint32_t ip_be16(uint32_t x) { return ((x & 0xffu) << 8) | ((x >> 8) & 0xffu); }

// REDUCE16 with ADDCARRY (amd64/in_cksum.c:61-73): a 64-bit sum of dwords to
// 16 bits.  0 only for a sum of 0; every other multiple of 65535 gives 0xffff.
// The one's-complement sum of the 16-bit words is the same in either byte
// order up to a byte swap, so a sum of memory-order halves goes back into a
// memory-order half.
ESPGPU_HD inline uint32_t ip_fold16(uint64_t acc) {
  acc = (acc & 0xffffffffu) + (acc >> 32);
  acc = (acc & 0xffffu) + ((acc >> 16) & 0xffffu) + (acc >> 32);
  acc = (acc & 0xffffu) + (acc >> 16);
  acc = (acc & 0xffffu) + (acc >> 16);
  return (uint32_t)acc;
}

// in_cksum over the header in w[0..NW) (unused dwords zero, the checksum field
// zero) as the memory-order half that goes into the field.  The loop has a
// constant bound so that the device keeps w[] in registers.
template <uint32_t NW>
ESPGPU_HD inline uint32_t ip_hdr_cksum(const uint32_t *w) {
  uint64_t acc = 0;
#pragma unroll
  for (uint32_t k = 0; k < NW; ++k) acc += w[k];
  return ~ip_fold16(acc) & 0xffffu;
}

// first dword of an IPv6 address in fe80::/10 (IN6_IS_SCOPE_LINKLOCAL)
ESPGPU_HD inline bool ip6_linklocal(uint32_t a0) { return (a0 & 0xc0ffu) == 0x80feu; }

// ip_ecn_ingress (ip_ecn.c:97-122): the outer TOS / traffic class for inner
// `itos` under an SA's ESPGPU_ENC_ECN_* flags
ESPGPU_HD inline uint32_t ip_ecn_ingress(uint32_t encflags, uint32_t itos) {
  uint32_t otos = itos;
  if (encflags & ESPGPU_ENC_ECN_ALLOWED) {
    if ((itos & 3u) == 3u) otos &= ~1u;                // CE: ECT(0) outside
  } else if (!(encflags & ESPGPU_ENC_ECN_NOCARE)) {
    otos &= ~3u;                                       // ECN_FORBIDDEN
  }
  return otos;
}

}  // namespace espgpu
