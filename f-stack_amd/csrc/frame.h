// frame.h — the outbound framing rule (include/espgpu.h, the framing block):
// one set of functions for espgpu_esp_frame on the host and the frm_* kernels
// on the device (frame.hip): the shape of a session, how many numbers an SA may
// still give out, and the bytes of one framed record.  decap.hip and encap.h
// read the shape from it too.
//
// Plain C++ with no HIP header, as classify.h and decap.h: the host side also
// builds with the host compiler alone.
#pragma once
#include <stdint.h>

#include "espgpu.h"
#include "rule_hd.h"

namespace espgpu {

// esp_output's hlen - 8, blks and alen (xform_esp.c:698-718) from what DevSA
// keeps of a session; false for a free slot or a DIGEST session.
ESPGPU_HD inline bool esp_shape_of(uint32_t mode, uint32_t calg, uint32_t mlen, uint32_t oflags, espgpu_eshape *s) {
  if (mode == ESPGPU_CSP_MODE_AEAD) {
    s->ivlen = 8;
    s->blks = 4;
  } else if (mode == ESPGPU_CSP_MODE_ETA && calg == ESPGPU_CRYPTO_AES_CBC) {
    s->ivlen = 16;
    s->blks = 16;
  } else if (mode == ESPGPU_CSP_MODE_ETA && calg == ESPGPU_CRYPTO_AES_ICM) {
    s->ivlen = 8;
    s->blks = (oflags & ESPGPU_OUT_CTRCOMPAT) ? 16 : 4;   // native_blocksize, :710-711
  } else if (mode == ESPGPU_CSP_MODE_ETA && calg == ESPGPU_CRYPTO_NULL_CBC) {
    s->ivlen = 0;
    s->blks = 4;
  } else {
    return false;
  }
  s->alen = mlen;
  return true;
}

ESPGPU_HD inline uint32_t esp_padding(uint32_t rlen, uint32_t blks) {
  return ((blks - ((rlen + 2) % blks)) % blks) + 2;       // :716
}

// Sequence numbers the SA may still give out from `count`: ah_output's
// condition (xform_ah.c:940-943) under WRAPCHECK, else no limit.
ESPGPU_HD inline uint64_t esp_out_room(uint64_t count, uint32_t oflags) {
  if (!(oflags & ESPGPU_OUT_WRAPCHECK) || (oflags & ESPGPU_OUT_CYCSEQ)) return ~0ull;
  return (oflags & ESPGPU_OUT_ESN) ? ~count : (uint64_t)(0xffffffffu - (uint32_t)count);
}

// The bytes esp_output writes into one record: header (:783-797), counter IV
// (:875-881), padding and trailer (:824-839).  `count` is the record's
// sequence number, `cntr` its explicit IV.  Every store lies inside the
// record; the header dwords are whole (the record is 4-byte aligned on the
// device), the padding starts at any byte and goes byte by byte.
ESPGPU_HD inline void esp_frame_write(uint8_t *rec, const espgpu_eshape &s, uint32_t oflags, uint32_t spi,
                                      uint64_t count, uint64_t cntr, uint32_t rlen, uint8_t nh) {
  auto put32 = [](uint8_t *p, uint32_t v) { mem_st32(p, __builtin_bswap32(v)); };   // big-endian
  put32(rec, spi);
  put32(rec + 4, (uint32_t)count);
  if (s.ivlen == 8) {
    put32(rec + 8, (uint32_t)(cntr >> 32));
    put32(rec + 12, (uint32_t)cntr);
  }
  const uint32_t padding = esp_padding(rlen, s.blks);
  uint8_t *pad = rec + 8 + s.ivlen + rlen;
  if (oflags & ESPGPU_OUT_PAD_SEQ) {
    for (uint32_t k = 0; k + 2 < padding; ++k) pad[k] = (uint8_t)(k + 1);
  } else if (oflags & ESPGPU_OUT_PAD_ZERO) {
    for (uint32_t k = 0; k + 2 < padding; ++k) pad[k] = 0;
  }
  pad[padding - 2] = (uint8_t)(padding - 2);
  pad[padding - 1] = nh;
}

// espgpu_esp_frame's rule: esp_output between m_makespace and crypto_dispatch
// (xform_esp.c:703-716, :782-887) for one record.  A usable shape is the
// caller's check.
inline int esp_frame_rule(espgpu_outsa *o, const espgpu_eshape &s, uint8_t *rec, uint32_t len, uint32_t rlen,
                          uint8_t next_header, uint32_t *esn_hi) {
  if (rlen > 0xffffu || 8 + s.ivlen + rlen + esp_padding(rlen, s.blks) + s.alen != len) return ESPGPU_EINVAL;
  if (esp_out_room(o->count, o->flags) == 0) return ESPGPU_EINVAL;
  o->count++;                                                    // :793
  const uint64_t cntr = o->cntr;
  if (s.ivlen == 8) o->cntr++;                                   // :802-803
  esp_frame_write(rec, s, o->flags, o->spi, o->count, cntr, rlen, next_header);
  *esn_hi = (o->flags & ESPGPU_OUT_ESN) ? (uint32_t)(o->count >> 32) : 0u;   // :799
  return 0;
}

}  // namespace espgpu
