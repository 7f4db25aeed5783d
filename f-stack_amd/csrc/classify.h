// classify.h — the inbound classification rule (include/espgpu.h, the
// classification block): one function for espgpu_esp_classify on the host and
// cls_kernel on the device (classify.hip), and espgpu_sad_build's table.
//
// Plain C++ with no HIP header, so the host side also builds with the host
// compiler alone (tools/classify_selftest.cpp runs it under its sanitizers).
#pragma once
#include <stdint.h>
#include <string.h>

#include "espgpu.h"
#include "ip_hdr.h"
#include "rule_hd.h"

namespace espgpu {

// key_u32hash (key.c:295-299): fnv_32_buf (sys/fnv_hash.h:23-31) over the SPI
// as struct secasvar stores it, in network byte order.
ESPGPU_HD inline uint32_t key_u32hash(uint32_t spi) {
  uint32_t h = 33554467u;                              // FNV1_32_INIT
  for (int s = 24; s >= 0; s -= 8) h = (h * 0x01000193u) ^ ((spi >> s) & 0xffu);
  return h;
}

constexpr uint32_t kClsKnown = ESPGPU_CLS_IPCSUM | ESPGPU_CLS_AH | 0xffff0000u;   // and ESPGPU_CLS_NATT_PORT's bits

ESPGPU_HD inline uint32_t cls_bswap32(uint32_t x) { return __builtin_bswap32(x); }
// the big-endian 16-bit field in the high half of a memory-order dword (the low half's is ip_be16)
ESPGPU_HD inline uint32_t cls_be16hi(uint32_t w) { return ((w >> 8) & 0xff00u) | (w >> 24); }

// The first half of a slot: SPI, sa | proto << 16 | af << 24, salt, flags.  One
// 16-byte load on the device (the table is 16-byte aligned there).
struct ClsSlotHead {
  uint32_t spi, ids, salt, flags;
};
static_assert(sizeof(espgpu_sad_entry) == 32 && sizeof(ClsSlotHead) == 16, "SPI table slot layout");
static_assert(sizeof(espgpu_pkt) == 8 && sizeof(espgpu_desc) == 16, "classification record layouts");

ESPGPU_HD inline ClsSlotHead cls_slot_head(const espgpu_sad_entry *e) {
  ClsSlotHead h;
#ifdef __HIP_DEVICE_COMPILE__
  const uint4 v = *reinterpret_cast<const uint4 *>(e);
  h.spi = v.x;
  h.ids = v.y;
  h.salt = v.z;
  h.flags = v.w;
#else
  h.spi = e->spi;
  h.ids = (uint32_t)e->sa | (uint32_t)e->proto << 16 | (uint32_t)e->af << 24;
  h.salt = e->salt;
  h.flags = e->flags;
#endif
  return h;
}

// Probe from the SPI's home slot to a match or a free slot, at most nslots
// steps (key_allocsa, key.c:1091-1133: the SPI first, then protocol, family
// and destination).  proto is the packet's, 50 or 51; dst[] is its destination in memory-order
// dwords, one for af 4 and four for af 6.  True: *sa and *salt are the entry's,
// *eflags its flags and, for an ESPGPU_SAD_NATT entry, *ports its dst[4..7]
// (natt->sport, natt->dport as they lie in a UDP header's first dword).
ESPGPU_HD inline bool cls_find(const espgpu_sad_entry *table, uint32_t nslots, uint32_t spi, uint32_t proto,
                               uint32_t af, const uint32_t dst[4], uint32_t *sa, uint32_t *salt, uint32_t *eflags,
                               uint32_t *ports) {
  if (spi == 0) return false;
  const uint32_t mask = nslots - 1;
  uint32_t slot = key_u32hash(spi) & mask;
  for (uint32_t k = 0; k < nslots; ++k, slot = (slot + 1) & mask) {
    const ClsSlotHead h = cls_slot_head(table + slot);
    if (h.spi == 0) return false;
    if (h.spi != spi) continue;
    // SPIs are unique in the table: this entry decides
    if (h.ids >> 16 != (proto | af << 8)) return false;
    const uint8_t *ed = table[slot].dst;
    for (uint32_t j = 0; j < (af == 4 ? 1u : 4u); ++j)
      if (mem_ld32(ed + 4 * j) != dst[j]) return false;
    *sa = h.ids & 0xffffu;
    *salt = h.salt;
    *eflags = h.flags;
    *ports = (h.flags & ESPGPU_SAD_NATT) ? mem_ld32(ed + 4) : 0u;
    return true;
  }
  return false;
}

ESPGPU_HD inline bool cls_lookup(const espgpu_sad_entry *table, uint32_t nslots, uint32_t spi, uint32_t af,
                                 const uint32_t dst[4], uint32_t *sa, uint32_t *salt) {
  uint32_t eflags, ports;
  return cls_find(table, nslots, spi, 50, af, dst, sa, salt, &eflags, &ports);
}

// espgpu_esp_classify's rule; *desc is written in every case.  `table` usable
// (nslots a power of two) is the caller's check.
ESPGPU_HD inline int esp_classify_rule(const espgpu_sad_entry *table, uint32_t nslots, const uint8_t *pkt,
                                       uint32_t len, uint32_t off4, uint32_t flags, espgpu_desc *desc) {
  int st = ESPGPU_EINVAL;
  uint32_t skip = 0, rlen = 0, af = 0, spi = 0, sa = 0, salt = 0, dst[4] = {0, 0, 0, 0};
  uint32_t udp = 0, uports = 0;                        // a UDP-encapsulated packet and its port dword
  uint32_t ah = 0;                                     // an AH packet (only under ESPGPU_CLS_AH)
  do {
    if (len < 20) break;
    // the 20 bytes every packet has, in one round of loads
    const uint32_t w0 = mem_ld32(pkt), w1 = mem_ld32(pkt + 4), w2 = mem_ld32(pkt + 8), w3 = mem_ld32(pkt + 12),
                   w4 = mem_ld32(pkt + 16);
    const uint32_t ver = (w0 >> 4) & 0xfu;
    if (ver == 4) {                                    // ip_input.c:488-561
      const uint32_t ihl = w0 & 0xfu, hlen = ihl * 4;
      if (hlen < 20 || hlen > len) break;
      if (flags & ESPGPU_CLS_IPCSUM) {
        // one's-complement sum of the 16-bit words: the same in either byte
        // order up to a byte swap, and 0xffff is its own swap (in_cksum)
        uint64_t acc = (uint64_t)w0 + w1 + w2 + w3 + w4;
        for (uint32_t k = 5; k < ihl; ++k) acc += mem_ld32(pkt + 4 * k);
        if (ip_fold16(acc) != 0xffffu) break;
      }
      const uint32_t ip_len = cls_be16hi(w0);
      if (ip_len < hlen || ip_len > len) break;
      st = ESPGPU_ENOTSUP;
      if (cls_be16hi(w1) & 0x3fffu) break;             // IP_MF | IP_OFFMASK, :807
      const uint32_t ip_p = (w2 >> 8) & 0xffu, port = flags >> 16;
      if (ip_p == 17 && port) {
        // udp_input up to the UF_ESPINUDP socket, then udp_ipsec_input
        if (ip_len - hlen < 8) break;                  // no UDP header: an ordinary datagram's error
        uports = mem_ld32(pkt + hlen);
        const uint32_t u1 = mem_ld32(pkt + hlen + 4), ulen = ip_be16(u1);
        if (cls_be16hi(uports) != port) break;         // another socket's, udp_usrreq.c:335
        st = ESPGPU_EINVAL;
        if (ulen < 8 || ulen > ip_len - hlen) break;   // :468-472; a longer ip_len is trimmed, :474
        st = ESPGPU_ENOTSUP;
        if (u1 >> 16) break;                           // uh_sum: udp_input verifies it, :489-520
        if (ulen - 8 < 8) break;                       // the keepalive, udpencap.c:131-132
        if (mem_ld32(pkt + hlen + 8) == 0) break;      // the non-ESP marker, :135
        st = ESPGPU_EINVAL;
        if ((ulen - 8) & 3) break;                     // xform_esp.c:279
        udp = 1;
        af = 4;
        skip = hlen + 8;
        rlen = ulen - 8;
        dst[0] = w4;
      } else if (ip_p == 51 && (flags & ESPGPU_CLS_AH)) {
        st = ESPGPU_EINVAL;
        if (ip_len - hlen < 12) break;                 // struct newah up to the ICV (the header's 2b)
        ah = 1;
        af = 4;
        skip = hlen;
        rlen = ip_len;
        dst[0] = w4;
      } else {
        if (ip_p != 50) break;
        st = ESPGPU_EINVAL;
        if (ip_len - hlen < 8) break;                  // ipsec_input.c:141
        if (ip_len & 3) break;                         // xform_esp.c:279
        af = 4;
        skip = hlen;
        rlen = ip_len - hlen;
        dst[0] = w4;
      }
    } else if (ver == 6) {                             // ip6_input, ipsec6_input
      if (len < 40) break;
      const uint32_t plen = ip_be16(w1);
      st = ESPGPU_ENOTSUP;
      if (plen == 0) break;                            // jumbogram
      st = ESPGPU_EINVAL;
      if (40 + plen > len) break;
      st = ESPGPU_ENOTSUP;
      const uint32_t nxt = (w1 >> 16) & 0xffu;         // ip6_nxt
      ah = nxt == 51 && (flags & ESPGPU_CLS_AH);
      if (nxt != 50 && !ah) break;
      for (uint32_t j = 0; j < 4; ++j) dst[j] = mem_ld32(pkt + 24 + 4 * j);
      if (ip6_linklocal(dst[0])) break;
      st = ESPGPU_EINVAL;
      if (ah) {
        if (plen < 12) break;
        st = ESPGPU_ENOTSUP;
        if (40 + plen > 65535) break;                  // espgpu_desc.len has 16 bits
      } else if (plen < 8 || (plen & 3)) {
        break;
      }
      af = 6;
      skip = 40;
      rlen = ah ? 40 + plen : plen;
    } else {
      break;
    }
    spi = cls_bswap32(mem_ld32(pkt + skip + 4 * ah));  // ipsec_input.c:144-153
    uint32_t eflags = 0, eports = 0;
    st = cls_find(table, nslots, spi, 50 + ah, af, dst, &sa, &salt, &eflags, &eports) ? 0 : ESPGPU_ENOENT;
    if (st == 0 && udp) {                              // udpencap.c:173-181
      if (!(eflags & ESPGPU_SAD_NATT) || eports != uports) st = ESPGPU_ENOENT;
    } else if (st == 0 && (eflags & ESPGPU_SAD_NATT)) {
      // the later steps tell a UDP-encapsulated packet by its SA alone: the host's
      st = ESPGPU_ENOTSUP;
    }
  } while (0);
  espgpu_desc d;
  // an AH record is the whole packet, with the ICV field's offset as its salt
  if (ah) salt = skip + 12;
  d.off4 = (st || ah) ? off4 : off4 + skip / 4;
  d.len = st ? (uint16_t)0 : (uint16_t)rlen;
  d.sa = st ? (uint16_t)0xffffu : (uint16_t)sa;
  d.esn_hi = 0;
  d.salt = st ? 0u : salt;
  *desc = d;
  return st;
}

// espgpu_sad_build.
inline int sad_build(const espgpu_sad_entry *sas, uint32_t nsas, espgpu_sad_entry *table, uint32_t nslots) {
  if (!table || (nsas && !sas) || nslots == 0 || (nslots & (nslots - 1)) || nslots / 2 < nsas) return ESPGPU_EINVAL;
  memset(table, 0, (size_t)nslots * sizeof(*table));
  const uint32_t mask = nslots - 1;
  for (uint32_t i = 0; i < nsas; ++i) {
    const espgpu_sad_entry &e = sas[i];
    if (e.spi == 0 || (e.proto != 50 && e.proto != 51) || (e.af != 4 && e.af != 6) ||
        (e.flags & ~(uint32_t)ESPGPU_SAD_NATT))
      return ESPGPU_EINVAL;
    const bool natt = e.flags & ESPGPU_SAD_NATT;
    if (natt && (e.proto != 50 || e.af != 4)) return ESPGPU_EINVAL;      // udpencap.c:155-163
    if (e.af == 4)
      for (int k = natt ? 8 : 4; k < 16; ++k)
        if (e.dst[k]) return ESPGPU_EINVAL;
    uint32_t slot = key_u32hash(e.spi) & mask;
    while (table[slot].spi != 0) {                     // a free slot exists: nslots >= 2 * nsas
      if (table[slot].spi == e.spi) return ESPGPU_EINVAL;   // key.c:1106-1109
      slot = (slot + 1) & mask;
    }
    table[slot] = e;
  }
  return 0;
}

}  // namespace espgpu
