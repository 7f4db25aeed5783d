// CPU self-test of the ESP / AH request rule (f-stack_amd/csrc/req_shape.h:
// req_plan, req_gather), the security boundary in front of espgpu_process's
// staging.  Requests as esp_input / esp_output / ah_input / ah_output build
// them (xform_esp.c:364-461, :820-900; xform_ah.c:613-664, :972-1047) over
// one- and multi-segment buffers, for every session kind: what is accepted,
// with the record length, header, salt, ESN, kind, result spans and gathered
// bytes written out here, and one rejected request per condition of the rule.
// Run by tests/test_host_selftests.py.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "req_shape.h"

using namespace espgpu;

namespace {

int fails = 0, checks = 0;
const char *ctx_name = "";
#define CHECK(c)                                                        \
  do {                                                                  \
    ++checks;                                                           \
    if (!(c)) {                                                         \
      printf("FAIL line %d [%s]: %s\n", __LINE__, ctx_name, #c);        \
      if (++fails > 30) exit(1);                                        \
    }                                                                   \
  } while (0)

constexpr int AEAD = ESPGPU_CSP_MODE_AEAD, ETA = ESPGPU_CSP_MODE_ETA, CIPHER = ESPGPU_CSP_MODE_CIPHER,
              DIGEST = ESPGPU_CSP_MODE_DIGEST;
constexpr int SEP = ESPGPU_CSP_F_SEPARATE_AAD, ESN = ESPGPU_CSP_F_ESN;
constexpr int ENC = ESPGPU_CRYPTO_OP_ENCRYPT, VERIFY = ESPGPU_CRYPTO_OP_VERIFY_DIGEST;
constexpr uint32_t kBatch = 1u << 20;       // batch_bytes
constexpr int kLead = 20;                   // bytes in front of the record (an IP header)

// A session kind and the numbers the rule must give for it: header and ICV
// bytes (SPI | SN | IV: 8 + 8 for GCM / CTR, 8 + 16 for CBC, 8 for ESP-NULL;
// AH has neither), the smallest legal payload with its record length, and the
// payload that makes a 1480-byte record.
struct Kind {
  const char *name;
  ReqSession ses;
  int hlen, alen;
  uint8_t kind;
  int small_plen;
  uint32_t small_rlen;
  int big_plen;
};
const Kind kKinds[] = {
    {"gcm16", {AEAD, 0, 16, false, false}, 16, 16, 1, 16, 48, 1448},
    {"gcm12", {AEAD, 0, 12, false, false}, 16, 12, 1, 16, 44, 1452},
    {"gcm8", {AEAD, 0, 8, false, false}, 16, 8, 1, 16, 40, 1456},
    {"gcm16-aad", {AEAD, SEP, 16, false, false}, 16, 16, 1, 16, 48, 1448},
    {"gcm12-aad", {AEAD, SEP, 12, false, false}, 16, 12, 1, 16, 44, 1452},
    {"gcm8-aad", {AEAD, SEP, 8, false, false}, 16, 8, 1, 16, 40, 1456},
    {"cbc-hmac", {ETA, 0, 16, false, false}, 24, 16, 2, 16, 56, 1440},
    {"cbc-hmac-esn", {ETA, ESN, 16, false, false}, 24, 16, 2, 16, 56, 1440},
    {"ctr-hmac", {ETA, 0, 12, true, false}, 16, 12, 2, 16, 44, 1452},
    {"ctr-hmac-esn", {ETA, ESN, 12, true, false}, 16, 12, 2, 16, 44, 1452},
    {"null-hmac", {ETA, 0, 12, false, true}, 8, 12, 2, 4, 24, 1460},
    {"null-hmac-esn", {ETA, ESN, 12, false, true}, 8, 12, 2, 4, 24, 1460},
    {"cbc", {CIPHER, 0, 0, false, false}, 24, 0, 2, 16, 40, 1456},
    {"ctr", {CIPHER, 0, 0, true, false}, 16, 0, 2, 16, 32, 1464},
    {"null", {CIPHER, 0, 0, false, true}, 8, 0, 2, 4, 12, 1472},
    {"ah", {DIGEST, 0, 12, false, false}, 0, 0, 4, 16, 16, 1480},
    {"ah-esn", {DIGEST, ESN, 12, false, false}, 0, 0, 4, 16, 16, 1480},
};
const Kind &kind_of(const char *name) {
  for (const Kind &k : kKinds)
    if (!strcmp(k.name, name)) return k;
  abort();
}

uint32_t g_seed = 1;
uint8_t rnd8() { g_seed = g_seed * 1664525u + 1013904223u; return (uint8_t)(g_seed >> 24); }

// A request of kind k with payload plen: the record (random bytes) at kLead
// of a buffer cut into segments of seglens (the last takes the rest), each in
// memory of its own.
struct Built {
  std::vector<uint8_t> rec;
  std::vector<std::vector<uint8_t>> mem;
  std::vector<espgpu_seg> segs;
  uint8_t aad[12];
  espgpu_req r;
  int doff;                                  // AH: the ICV field's offset
  void cut(const std::vector<uint8_t> &buf, const std::vector<uint32_t> &seglens) {
    mem.clear();
    segs.clear();
    size_t o = 0;
    for (size_t i = 0; i <= seglens.size(); ++i) {
      const size_t n = i < seglens.size() ? seglens[i] : buf.size() - o;
      mem.emplace_back(buf.begin() + o, buf.begin() + o + n);
      o += n;
    }
    for (auto &m : mem) segs.push_back(espgpu_seg{m.data(), (uint32_t)m.size()});
    r.segs = segs.data();
    r.nsegs = (int)segs.size();
  }
};

void build(const Kind &k, int plen, int op, const std::vector<uint32_t> &seglens, int tail, Built *b) {
  const ReqSession &s = k.ses;
  const size_t rlen = (size_t)k.hlen + plen + k.alen;
  b->rec.resize(rlen);
  for (auto &x : b->rec) x = rnd8();
  std::vector<uint8_t> buf(kLead + rlen + tail);
  for (auto &x : buf) x = rnd8();
  memcpy(buf.data() + kLead, b->rec.data(), rlen);
  espgpu_req &r = b->r;
  memset(&r, 0, sizeof r);
  r.session = 3;
  r.crp_op = op;
  r.opaque = b;
  const uint8_t esn[4] = {0x01, 0x02, 0x03, 0x04};
  memcpy(r.crp_esn, esn, 4);
  b->doff = 0;
  if (s.mode == DIGEST) {
    b->doff = plen >= 64 ? 32 : 4;            // IP header + AH header in front of the ICV; or a tiny one
    r.crp_payload_start = kLead;
    r.crp_payload_length = plen;
    r.crp_digest_start = kLead + b->doff;
  } else {
    r.crp_aad_start = kLead;
    r.crp_aad_length = k.hlen;
    r.crp_payload_start = kLead + k.hlen;
    r.crp_payload_length = plen;
    r.crp_digest_start = k.alen ? kLead + k.hlen + plen : 0;
    if (s.mode == AEAD || s.ctr) {
      // salt / nonce | the record's explicit IV | be32(1)
      const uint8_t salt[4] = {0xA1, 0xB2, 0xC3, 0xD4};
      memcpy(r.crp_iv, salt, 4);
      memcpy(r.crp_iv + 4, b->rec.data() + 8, 8);
      r.crp_iv[15] = 1;
      r.crp_flags = ESPGPU_CRYPTO_F_IV_SEPARATE;
    } else if (!s.null) {
      r.crp_iv_start = kLead + 8;
    }
    if (s.mode == AEAD) {
      r.crp_aad_length = 8;
      if (s.flags & SEP) {                    // SPI | ESN high half | SN, outside the buffer
        const uint8_t hi[4] = {0x0A, 0x0B, 0x0C, 0x0D};
        memcpy(b->aad, b->rec.data(), 4);
        memcpy(b->aad + 4, hi, 4);
        memcpy(b->aad + 8, b->rec.data() + 4, 4);
        r.crp_aad = b->aad;
        r.crp_aad_length = 12;
        r.crp_aad_start = 0;
      }
    }
    if (s.mode == CIPHER) {                   // esp_output sets no AAD for it
      r.crp_aad_start = -7;
      r.crp_aad_length = 0;
    }
  }
  b->cut(buf, seglens);
}

// An accepted request: every field of the plan against the numbers above.
void accept(const Kind &k, int plen, uint32_t rlen, int op, const std::vector<uint32_t> &seglens) {
  ctx_name = k.name;
  const ReqSession &s = k.ses;
  Built b;
  build(k, plen, op, seglens, 7, &b);
  ReqPlan p;
  memset(&p, 0xEE, sizeof p);
  CHECK(req_plan(s, b.r, kBatch, &p) == 0);
  CHECK(p.op == ((op & ENC) ? 1 : 0));
  CHECK(p.kind == k.kind);
  CHECK(p.hlen == k.hlen && p.plen == plen && p.alen == k.alen);
  CHECK(p.rlen == rlen && b.rec.size() == rlen);
  CHECK(p.rec_start == (uint32_t)kLead);
  CHECK(p.aad_start == kLead);
  CHECK(p.gcm_gather == (s.mode == AEAD));
  const bool dig = s.mode == DIGEST, verify = (op & VERIFY) != 0;
  if (dig) {
    CHECK(p.salt == ((uint32_t)b.doff | (verify ? 0x80000000u : 0u)));
  } else {
    CHECK(p.salt == ((s.mode == AEAD || s.ctr) ? 0xD4C3B2A1u : 0u));   // crp_iv[0..3] in memory order
  }
  const uint32_t esn = s.mode == AEAD ? ((s.flags & SEP) ? 0x0A0B0C0Du : 0u) : ((s.flags & ESN) ? 0x01020304u : 0u);
  CHECK(p.esn_hi == esn);
  if (s.mode == AEAD) CHECK(memcmp(p.hdr, b.rec.data(), 8) == 0);
  // result spans: the payload, and the ICV when encrypting; AH: the ICV when computing
  if (dig) {
    CHECK(p.nspan == (verify ? 0 : 1));
    CHECK(p.span[0].buf_off == (uint32_t)(kLead + b.doff) && p.span[0].stage_from == (uint32_t)b.doff);
    CHECK(p.span[0].n == (verify ? 0u : 12u));
  } else {
    CHECK(p.nspan == (((op & ENC) && k.alen) ? 2 : 1));
    CHECK(p.span[0].buf_off == (uint32_t)(kLead + k.hlen) && p.span[0].stage_from == (uint32_t)k.hlen &&
          p.span[0].n == (uint32_t)plen);
    if (p.nspan == 2)
      CHECK(p.span[1].buf_off == (uint32_t)(kLead + k.hlen + plen) &&
            p.span[1].stage_from == (uint32_t)(k.hlen + plen) && p.span[1].n == (uint32_t)k.alen);
  }
  // the gathered bytes are the record the kernels read: SPI | SN | IV | payload | ICV
  std::vector<uint8_t> got(rlen + 16, 0x5A);
  CHECK(req_gather(p, b.r, got.data()));
  CHECK(memcmp(got.data(), b.rec.data(), rlen) == 0);
  for (int i = 0; i < 16; ++i) CHECK(got[rlen + i] == 0x5A);
  // and where it lies in one segment, seg_span finds it there
  if (seglens.empty()) CHECK(seg_span(b.r.segs, 1, p.rec_start, rlen) == b.mem[0].data() + kLead);
  else CHECK(seg_span(b.r.segs, (uint32_t)b.r.nsegs, p.rec_start, rlen) == nullptr);
}

// A request one change away from an accepted one is EINVAL.
template <class F>
void reject(const char *what, const char *kind, int plen, int op, F change, uint32_t batch = kBatch) {
  ctx_name = what;
  const Kind &k = kind_of(kind);
  Built b;
  build(k, plen, op, {}, 0, &b);
  ReqPlan p;
  const int before = req_plan(k.ses, b.r, kBatch, &p);
  ReqSession s = k.ses;
  change(b, s);
  const int after = req_plan(s, b.r, batch, &p);
  CHECK(before == 0);
  CHECK(after == ESPGPU_EINVAL);
}

void rejections() {
  auto none = [](Built &, ReqSession &) {};
  reject("plen 0", "gcm16", 16, 0, [](Built &b, ReqSession &) { b.r.crp_payload_length = 0; });
  reject("plen < 0", "cbc-hmac", 16, 0, [](Built &b, ReqSession &) { b.r.crp_payload_length = -16; });
  reject("payload_start < hlen", "gcm16", 16, 0, [](Built &b, ReqSession &) {
    b.r.crp_payload_start = 8;
    b.r.crp_aad_start = -8;
  });
  reject("payload + ICV past the buffer", "gcm16", 16, 0, [](Built &b, ReqSession &) { b.segs.back().len -= 1; });
  reject("payload past the buffer, no ICV", "cbc", 16, ENC, [](Built &b, ReqSession &) { b.segs.back().len -= 1; });
  reject("digest before payload end", "cbc-hmac", 32, 0, [](Built &b, ReqSession &) { b.r.crp_digest_start -= 4; });
  reject("digest past the buffer", "ctr-hmac", 16, 0, [](Built &b, ReqSession &) { b.r.crp_digest_start += 4; });
  reject("gcm without IV_SEPARATE", "gcm16", 16, 0, [](Built &b, ReqSession &) { b.r.crp_flags = 0; });
  reject("gcm aad_length 12 without SEPARATE_AAD", "gcm16", 16, 0, [](Built &b, ReqSession &) { b.r.crp_aad_length = 12; });
  reject("gcm separate aad on a session without the flag", "gcm16-aad", 16, 0, [](Built &, ReqSession &s) { s.flags = 0; });
  reject("gcm aad_length 8 with SEPARATE_AAD", "gcm16-aad", 16, 0, [](Built &b, ReqSession &) { b.r.crp_aad_length = 8; });
  reject("gcm SEPARATE_AAD session, aad in the buffer", "gcm16", 16, 0, [](Built &, ReqSession &s) { s.flags = SEP; });
  reject("gcm header not in front of the payload", "gcm16", 16, 0, [](Built &b, ReqSession &) { b.r.crp_aad_start -= 4; });
  reject("ctr counter word 2", "ctr-hmac", 16, 0, [](Built &b, ReqSession &) { b.r.crp_iv[15] = 2; });
  reject("ctr explicit IV differs from the record's", "ctr", 16, ENC, [](Built &b, ReqSession &) { b.r.crp_iv[5] ^= 1; });
  reject("ctr without IV_SEPARATE", "ctr-hmac", 16, 0, [](Built &b, ReqSession &) { b.r.crp_flags = 0; });
  reject("cbc payload 24", "cbc-hmac", 32, 0, [](Built &b, ReqSession &) {
    b.r.crp_payload_length = 24;
    b.r.crp_digest_start -= 8;
  });
  reject("cbc iv_start off", "cbc", 16, 0, [](Built &b, ReqSession &) { b.r.crp_iv_start += 4; });
  reject("null payload 6", "null-hmac", 8, 0, [](Built &b, ReqSession &) {
    b.r.crp_payload_length = 6;
    b.r.crp_digest_start -= 2;
  });
  reject("eta aad_length not the header", "null-hmac", 8, 0, [](Built &b, ReqSession &) { b.r.crp_aad_length = 12; });
  reject("eta record length not a multiple of 4", "ctr-hmac", 20, 0, [](Built &b, ReqSession &) {
    b.r.crp_payload_length = 17;
    b.r.crp_digest_start -= 3;
  });
  static const uint8_t some_aad[12] = {0};
  reject("cipher-only with AAD", "cbc", 16, 0, [](Built &b, ReqSession &) { b.r.crp_aad = some_aad; });
  reject("cipher-only with aad_length", "ctr", 16, 0, [](Built &b, ReqSession &) { b.r.crp_aad_length = 16; });
  reject("cipher-only with VERIFY_DIGEST", "null", 4, 0, [](Built &b, ReqSession &) { b.r.crp_op = VERIFY; });
  reject("ah encrypt op", "ah", 64, 0, [](Built &b, ReqSession &) { b.r.crp_op = ENC; });
  reject("ah digest offset 6", "ah", 64, VERIFY, [](Built &b, ReqSession &) { b.r.crp_digest_start = kLead + 6; });
  reject("ah digest past the payload", "ah", 64, 0, [](Built &b, ReqSession &) { b.r.crp_digest_start = kLead + 56; });
  reject("ah digest before the payload", "ah", 64, 0, [](Built &b, ReqSession &) { b.r.crp_digest_start = kLead - 4; });
  reject("ah with aad_length", "ah-esn", 64, 0, [](Built &b, ReqSession &) { b.r.crp_aad_length = 8; });
  reject("ah with AAD", "ah", 64, VERIFY, [](Built &b, ReqSession &) { b.r.crp_aad = some_aad; });
  reject("ah payload 65536", "ah", 65532, 0, [](Built &b, ReqSession &) {
    b.mem[0].resize(kLead + 65536);
    b.segs[0] = espgpu_seg{b.mem[0].data(), kLead + 65536};
    b.r.crp_payload_length = 65536;
  });
  // 16 + 65504 + 16 = 65536 > 65535; the record before it, 65532 bytes, is accepted
  reject("rlen 65536", "gcm16", 65500, 0, [](Built &b, ReqSession &) {
    b.mem[0].resize(kLead + 65536);
    b.segs[0] = espgpu_seg{b.mem[0].data(), kLead + 65536};
    b.r.crp_payload_length = 65504;
    b.r.crp_digest_start += 4;
  });
  // a 48-byte record needs 48 + 16 bytes of batch
  reject("rlen + 16 > batch_bytes", "gcm16", 16, 0, none, 63);
  ctx_name = "rlen + 16 == batch_bytes";
  Built b;
  build(kind_of("gcm16"), 16, 0, {}, 0, &b);
  ReqPlan p;
  CHECK(req_plan(kind_of("gcm16").ses, b.r, 64, &p) == 0);
  // a buffer that ends inside the record fails the gather, not only the plan
  ctx_name = "gather past the buffer";
  build(kind_of("cbc"), 16, 0, {}, 0, &b);
  CHECK(req_plan(kind_of("cbc").ses, b.r, kBatch, &p) == 0);
  b.segs[0].len -= 1;
  std::vector<uint8_t> got(64);
  CHECK(!req_gather(p, b.r, got.data()));
}

}  // namespace

int main() {
  for (const Kind &k : kKinds) {
    const bool dig = k.ses.mode == DIGEST, cipher_only = k.ses.mode == CIPHER;
    // decrypt / verify, then encrypt / compute
    const int op0 = cipher_only ? 0 : VERIFY, op1 = dig ? 0 : ENC;
    for (int op : {op0, op1}) {
      accept(k, k.small_plen, k.small_rlen, op, {});
      accept(k, k.small_plen, k.small_rlen, op, {(uint32_t)kLead + 5});
      accept(k, k.big_plen, 1480, op, {});
      accept(k, k.big_plen, 1480, op, {(uint32_t)kLead + 9, 700});      // 1480 bytes over three segments
      accept(k, k.big_plen, 1480, op, {3, (uint32_t)kLead + 20, 1400});  // and four, the first before the record
    }
  }
  rejections();
  if (fails) return 1;
  printf("OK req_shape: %d checks\n", checks);
  return 0;
}
