// req_shape.h — the ESP / AH request rule of espgpu_process: what esp_input,
// esp_output, ah_input and ah_output may hand to a driver, per session mode,
// and the record, header, salt, ESN and result spans a request yields.  Pure
// host logic over espgpu_req and five session fields: no HIP, no context
// (tools/req_shape_selftest.cpp runs it on the CPU).
#pragma once
#include <stdint.h>
#include <string.h>

#include <algorithm>

#include "espgpu.h"

namespace espgpu {

constexpr uint32_t kDigVerifyBit = 0x80000000u;   // driver path: desc.salt bit 31 = VERIFY_DIGEST

inline uint32_t le32(const uint8_t *p) { return (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) | ((uint32_t)p[3] << 24); }
inline uint32_t be32(const uint8_t *p) { return ((uint32_t)p[0] << 24) | ((uint32_t)p[1] << 16) | ((uint32_t)p[2] << 8) | p[3]; }

// Copy `n` bytes at logical offset `off` of a segmented buffer.
inline bool seg_copy_out(const espgpu_seg *segs, uint32_t nsegs, uint32_t off, uint32_t n, uint8_t *dst) {
  for (uint32_t i = 0; i < nsegs; ++i) {
    const espgpu_seg &s = segs[i];
    if (off >= s.len) { off -= s.len; continue; }
    uint32_t k = std::min(n, s.len - off);
    memcpy(dst, (const uint8_t *)s.base + off, k);
    dst += k; n -= k; off = 0;
    if (!n) return true;
  }
  return n == 0;
}
inline bool seg_copy_in(const espgpu_seg *segs, uint32_t nsegs, uint32_t off, uint32_t n, const uint8_t *src) {
  for (uint32_t i = 0; i < nsegs; ++i) {
    const espgpu_seg &s = segs[i];
    if (off >= s.len) { off -= s.len; continue; }
    uint32_t k = std::min(n, s.len - off);
    memcpy((uint8_t *)s.base + off, src, k);
    src += k; n -= k; off = 0;
    if (!n) return true;
  }
  return n == 0;
}

// [off, off + n) of a segmented buffer if it lies in one segment, else nullptr.
inline const uint8_t *seg_span(const espgpu_seg *segs, uint32_t nsegs, uint32_t off, uint32_t n) {
  for (uint32_t i = 0; i < nsegs; ++i) {
    if (off >= segs[i].len) { off -= segs[i].len; continue; }
    return off + n <= segs[i].len ? (const uint8_t *)segs[i].base + off : nullptr;
  }
  return nullptr;
}

// Where result bytes go back: [buf_off, buf_off + n) of the request buffer
// receives staged bytes [stage_from, stage_from + n) of the record.
struct ReqSpan { uint32_t buf_off, stage_from, n; };

// The session fields the rule reads.
struct ReqSession {
  int mode = 0, flags = 0, mlen = 0;
  bool ctr = false;       // ETA / CIPHER with AES-ICM (RFC 3686 ESP AES-CTR)
  bool null = false;      // ETA / CIPHER with CRYPTO_NULL_CBC (ESP-NULL)
};

// An accepted request: the record the kernels read and what comes back.
struct ReqPlan {
  int op;                     // 0 decrypt, 1 encrypt
  uint8_t kind;               // 1 GCM, 2 ETA, 4 DIGEST (Slot::kinds)
  int hlen, plen, alen;       // header (SPI | SN | IV), payload and ICV bytes of the record
  uint32_t rlen;              // hlen + plen + alen
  uint32_t rec_start;         // where the record starts in the request buffer
  int aad_start;
  uint8_t hdr[8];             // GCM: SPI | SN as authenticated (else zero)
  uint32_t esn_hi, salt;      // espgpu_desc's
  int nspan;
  ReqSpan span[2];
  // GCM: gathered as hdr, crp_iv + 4, then the buffer from crp_payload_start;
  // else one run of rlen bytes from aad_start
  bool gcm_gather;
};

// Validate that a request has the shape esp_input / esp_output build
// (xform_esp.c:364-461, 820-900), or ah_input / ah_output for a DIGEST
// session.  0 and *out, or ESPGPU_EINVAL.
inline int req_plan(const ReqSession &ses, const espgpu_req &rq, uint32_t batch_bytes, ReqPlan *out) {
  const espgpu_req *r = &rq;
  const int op = (r->crp_op & ESPGPU_CRYPTO_OP_ENCRYPT) ? 1 : 0;
  size_t total = 0;
  for (int i = 0; i < r->nsegs; ++i) total += r->segs[i].len;
  const bool gcm = ses.mode == ESPGPU_CSP_MODE_AEAD, cipher_only = ses.mode == ESPGPU_CSP_MODE_CIPHER;
  // AH (CSP_MODE_DIGEST): the record is the hashed range itself, no header,
  // and the ICV field lies inside it
  const bool dig = ses.mode == ESPGPU_CSP_MODE_DIGEST;
  // ICV bytes in the record: the session's (possibly truncated) mlen, 16/12/8
  // for GCM (cryptosoft.c:1112-1117), 12 or 20 for HMAC-SHA1, 16 for
  // HMAC-SHA2-256-128, none without auth.  IV: 8 for GCM / CTR, none for
  // ESP-NULL (ivsize 0), else 16.
  const int ivlen = (gcm || ses.ctr) ? 8 : ses.null ? 0 : 16, hlen = dig ? 0 : 8 + ivlen, alen = dig ? 0 : ses.mlen;
  const int plen = r->crp_payload_length;
  int aad_start = cipher_only ? r->crp_payload_start - hlen : r->crp_aad_start;
  // ESP shape checks
  if (plen <= 0 || r->crp_payload_start < hlen ||
      (size_t)(r->crp_payload_start + plen + alen) > total ||
      (alen && (size_t)(r->crp_digest_start + alen) > total))
    return ESPGPU_EINVAL;
  if (cipher_only && (r->crp_aad || r->crp_aad_length != 0 || (r->crp_op & ESPGPU_CRYPTO_OP_VERIFY_DIGEST)))
    return ESPGPU_EINVAL;
  uint8_t *hdr = out->hdr;
  memset(hdr, 0, 8);
  uint32_t esn_hi = 0, salt = 0;
  if (dig) {
    // swcr_authcompute's request as ah_input / ah_output build it
    // (xform_ah.c:613-664, :972-1047): no AAD, COMPUTE or VERIFY, the digest
    // field inside the payload range at a multiple of 4
    const int doff = r->crp_digest_start - r->crp_payload_start;
    if (r->crp_aad || r->crp_aad_length != 0 || op == 1 || plen > 65535 || doff < 0 || (doff & 3) ||
        doff + ses.mlen > plen)
      return ESPGPU_EINVAL;
    if (ses.flags & ESPGPU_CSP_F_ESN) esn_hi = be32(r->crp_esn);
    salt = (uint32_t)doff | ((r->crp_op & ESPGPU_CRYPTO_OP_VERIFY_DIGEST) ? kDigVerifyBit : 0u);
    aad_start = r->crp_payload_start;
  } else if (gcm) {
    if (!(r->crp_flags & ESPGPU_CRYPTO_F_IV_SEPARATE)) return ESPGPU_EINVAL;   // cryptosoft.c:496
    if (r->crp_aad) {
      if (!(ses.flags & ESPGPU_CSP_F_SEPARATE_AAD) || r->crp_aad_length != 12) return ESPGPU_EINVAL;
      const uint8_t *a = (const uint8_t *)r->crp_aad;
      memcpy(hdr, a, 4);
      memcpy(hdr + 4, a + 8, 4);
      esn_hi = be32(a + 4);
      aad_start = r->crp_payload_start - hlen;   // header bytes in the buffer (unused by the cipher)
    } else {
      if (r->crp_aad_length != 8 || (ses.flags & ESPGPU_CSP_F_SEPARATE_AAD)) return ESPGPU_EINVAL;
      if (r->crp_payload_start != aad_start + hlen) return ESPGPU_EINVAL;
      if (!seg_copy_out(r->segs, (uint32_t)r->nsegs, (uint32_t)aad_start, 8, hdr)) return ESPGPU_EINVAL;
    }
    salt = le32(r->crp_iv);
  } else if (ses.ctr) {
    // AES-CTR: crp_iv = nonce || explicit IV || be32(1) (xform_esp.c:453-458),
    // and the explicit IV is the record's; the kernel rebuilds the counter
    // blocks from the descriptor's salt (the nonce) and the record
    if (!(r->crp_flags & ESPGPU_CRYPTO_F_IV_SEPARATE) || r->crp_aad ||
        (!cipher_only && r->crp_aad_length != hlen) || r->crp_payload_start != aad_start + hlen ||
        be32(r->crp_iv + 12) != 1u)
      return ESPGPU_EINVAL;
    uint8_t ivb[8];
    if (!seg_copy_out(r->segs, (uint32_t)r->nsegs, (uint32_t)(aad_start + 8), 8, ivb) ||
        memcmp(ivb, r->crp_iv + 4, 8) != 0)
      return ESPGPU_EINVAL;
    salt = le32(r->crp_iv);
    if (ses.flags & ESPGPU_CSP_F_ESN) esn_hi = be32(r->crp_esn);
  } else if (ses.null) {
    // ESP-NULL: no IV (crp_iv_start unset, xform_esp.c:459-461), payload a
    // multiple of the null blocksize 4 (:316-324)
    if (r->crp_aad || (!cipher_only && r->crp_aad_length != hlen) || r->crp_payload_start != aad_start + hlen ||
        (plen & 3))
      return ESPGPU_EINVAL;
    if (ses.flags & ESPGPU_CSP_F_ESN) esn_hi = be32(r->crp_esn);
  } else {
    if (r->crp_aad || (!cipher_only && r->crp_aad_length != hlen) || r->crp_iv_start != aad_start + 8 ||
        r->crp_payload_start != aad_start + hlen || (plen & 15))
      return ESPGPU_EINVAL;
    if (ses.flags & ESPGPU_CSP_F_ESN) esn_hi = be32(r->crp_esn);
  }
  if (alen && r->crp_digest_start != r->crp_payload_start + plen) return ESPGPU_EINVAL;
  const uint32_t rlen = (uint32_t)(hlen + plen + alen);
  if (rlen > 65535 || (!dig && (rlen & 3)) || rlen + 16 > batch_bytes) return ESPGPU_EINVAL;
  ReqPlan &p = *out;
  p.op = op; p.hlen = hlen; p.plen = plen; p.alen = alen; p.rlen = rlen;
  p.rec_start = (uint32_t)(r->crp_payload_start - hlen);
  p.aad_start = aad_start; p.esn_hi = esn_hi; p.salt = salt; p.gcm_gather = gcm;
  // results: payload (+ digest when encrypting) go back to the request buffer
  p.nspan = 1;
  p.span[0] = {(uint32_t)r->crp_payload_start, (uint32_t)hlen, (uint32_t)plen};
  p.span[1] = {0, 0, 0};
  if (op == 1 && alen) {
    p.nspan = 2;
    p.span[1] = {(uint32_t)r->crp_digest_start, (uint32_t)(hlen + plen), (uint32_t)ses.mlen};
  }
  if (dig) {
    // COMPUTE: the mlen digest bytes and nothing else; VERIFY: nothing
    const bool verify = (salt & kDigVerifyBit) != 0;
    p.nspan = verify ? 0 : 1;
    p.span[0] = {(uint32_t)r->crp_digest_start, salt & ~kDigVerifyBit, verify ? 0u : (uint32_t)ses.mlen};
  }
  p.kind = gcm ? 1 : dig ? 4 : 2;
  return 0;
}

// The record bytes as the kernels read them: SPI | SN | IV | payload | ICV
// (rlen bytes at dst); false if the buffer does not hold them.
inline bool req_gather(const ReqPlan &p, const espgpu_req &r, uint8_t *dst) {
  if (p.gcm_gather) {
    memcpy(dst, p.hdr, 8);
    memcpy(dst + 8, r.crp_iv + 4, 8);
    return seg_copy_out(r.segs, (uint32_t)r.nsegs, (uint32_t)r.crp_payload_start, (uint32_t)(p.plen + p.alen),
                        dst + p.hlen);
  }
  return seg_copy_out(r.segs, (uint32_t)r.nsegs, (uint32_t)p.aad_start, p.rlen, dst);
}

}  // namespace espgpu
