// espgpu_session.cpp — sessions of the host runtime (espgpu_ctx.h): what the
// engine serves, the driver's bid, and the SA table.
//
// Reference interfaces mirrored (F-Stack 1.25 tree):
//   probesession  freebsd/opencrypto/cryptosoft.c:1244-1303 (swcr_probesession)
//                 + check_csp, freebsd/opencrypto/crypto.c:746-870
//   newsession    cryptosoft.c:1309-1409, swcr_setup_gcm :1087, _cipher :976, _auth :1003
//   freesession   cryptosoft.c:1412
#include <stdlib.h>

#include "espgpu_ctx.h"
#include "host_crypto.h"

namespace espgpu {

// Whether the driver bids for AH (CSP_MODE_DIGEST) sessions: set_tuning
// "ah_offer" (process-wide, like the probe itself), else FF_GPUCRYPTO_AH in
// the environment.  Off by default, and decided here rather than only in the
// F-Stack shim: a binary linked before the engine knew the mode forwards every
// csp to the probe, and must keep AH on cryptosoft under a newer library.
int g_ah_offer = -1;                       // -1: the environment decides
static bool ah_offered() {
  if (g_ah_offer >= 0) return g_ah_offer != 0;
  const char *e = getenv("FF_GPUCRYPTO_AH");
  return e && atoi(e) > 0;
}

// The HMAC's hash length (xform_sha1.c, xform_sha2.c); 0: not served.
static int hmac_hashlen(int auth_alg) {
  switch (auth_alg) {
    case ESPGPU_CRYPTO_SHA1_HMAC: return 20;
    case ESPGPU_CRYPTO_SHA2_256_HMAC: return 32;
    case ESPGPU_CRYPTO_SHA2_384_HMAC: return 48;
    case ESPGPU_CRYPTO_SHA2_512_HMAC: return 64;
  }
  return 0;
}

// swcr_probesession + check_csp restricted to what this engine serves:
// ESPGPU_PROBE_HARDWARE or ESPGPU_EINVAL (espgpu_newsession's check).
int probe_caps(const espgpu_session_params *csp) {
  if (!csp) return ESPGPU_EINVAL;
  const int supported_flags = ESPGPU_CSP_F_SEPARATE_AAD | ESPGPU_CSP_F_ESN;
  if (csp->csp_flags & ~supported_flags) return ESPGPU_EINVAL;
  if (csp->csp_ivlen < 0 || csp->csp_cipher_klen < 0 || csp->csp_auth_klen < 0 || csp->csp_auth_mlen < 0)
    return ESPGPU_EINVAL;
  const int k = csp->csp_cipher_klen;
  const bool aes_klen = (k == 16 || k == 24 || k == 32);
  const int hashlen = hmac_hashlen(csp->csp_auth_alg);
  switch (csp->csp_mode) {
    case ESPGPU_CSP_MODE_AEAD:
      if (csp->csp_cipher_alg != ESPGPU_CRYPTO_AES_NIST_GCM_16 || !aes_klen) return ESPGPU_EINVAL;
      if (csp->csp_ivlen != 12) return ESPGPU_EINVAL;                 // cryptosoft.c:1093
      if (csp->csp_auth_alg != 0 || csp->csp_auth_klen != 0) return ESPGPU_EINVAL;
      // ICVs of 8/12/16 bytes (RFC 4106 s3.3; 0 = 16); other truncations,
      // which ESP never sets up, are left to cryptosoft (probe ESPGPU_EINVAL)
      if (csp->csp_auth_mlen != 0 && csp->csp_auth_mlen != 8 && csp->csp_auth_mlen != 12 &&
          csp->csp_auth_mlen != 16)
        return ESPGPU_EINVAL;
      if (csp->csp_flags & ESPGPU_CSP_F_ESN) return ESPGPU_EINVAL;    // ESN for GCM = SEPARATE_AAD
      return ESPGPU_PROBE_HARDWARE;
    case ESPGPU_CSP_MODE_CIPHER:
      // ESP with encryption and no auth (esp_init :230-231): AES-CBC or
      // AES-ICM (csp_ivlen = the enc_xform's 16), or ESP-NULL (no key, no
      // IV: swcr_null); swcr_probesession :1257-1266 / swcr_cipher_supported
      // :1228-1239.  No auth fields; esp_init sets no flags for it.
      if (csp->csp_auth_alg != 0 || csp->csp_auth_klen != 0 || csp->csp_auth_mlen != 0) return ESPGPU_EINVAL;
      if (csp->csp_flags) return ESPGPU_EINVAL;
      if (csp->csp_cipher_alg == ESPGPU_CRYPTO_NULL_CBC) return csp->csp_cipher_klen == 0 ? ESPGPU_PROBE_HARDWARE : ESPGPU_EINVAL;
      if ((csp->csp_cipher_alg != ESPGPU_CRYPTO_AES_CBC && csp->csp_cipher_alg != ESPGPU_CRYPTO_AES_ICM) ||
          !aes_klen || csp->csp_ivlen != 16)
        return ESPGPU_EINVAL;
      return ESPGPU_PROBE_HARDWARE;
    case ESPGPU_CSP_MODE_ETA:
      // AES-CBC or AES-ICM (CTR; csp_ivlen = the enc_xform's 16, the nonce
      // rides in crp_iv), or ESP-NULL (CRYPTO_NULL_CBC: no key; cryptosoft
      // degrades the session to the digest, cryptosoft.c:1394-1398), with
      // HMAC-SHA1 or HMAC-SHA2-256/384/512 (esp_init :225-241)
      if (csp->csp_cipher_alg == ESPGPU_CRYPTO_NULL_CBC) {
        if (csp->csp_cipher_klen != 0) return ESPGPU_EINVAL;
      } else if ((csp->csp_cipher_alg != ESPGPU_CRYPTO_AES_CBC && csp->csp_cipher_alg != ESPGPU_CRYPTO_AES_ICM) ||
                 !aes_klen || csp->csp_ivlen != 16) {
        return ESPGPU_EINVAL;
      }
      if (!hashlen || csp->csp_auth_klen <= 0) return ESPGPU_EINVAL;
      if (csp->csp_auth_mlen > hashlen || (csp->csp_auth_mlen & 3)) return ESPGPU_EINVAL;
      if (csp->csp_flags & ESPGPU_CSP_F_SEPARATE_AAD) return ESPGPU_EINVAL;
      return ESPGPU_PROBE_HARDWARE;
    case ESPGPU_CSP_MODE_DIGEST:
      // AH (ah_init, xform_ah.c:231-246): an HMAC over the whole packet,
      // check_csp's CSP_MODE_DIGEST rules (crypto.c:792-821: no cipher
      // algorithm, key or IV) and swcr_auth_supported.  CRYPTO_NULL_HMAC,
      // RIPEMD, plain hashes and AES-GMAC (which ah_init sets up with
      // csp_ivlen 0, refused by cryptosoft itself) stay with cryptosoft.
      if (csp->csp_cipher_alg != 0 || csp->csp_cipher_klen != 0 || csp->csp_cipher_key != nullptr ||
          csp->csp_ivlen != 0)
        return ESPGPU_EINVAL;
      if (csp->csp_flags & ~ESPGPU_CSP_F_ESN) return ESPGPU_EINVAL;
      if (!hashlen || csp->csp_auth_klen <= 0 || !csp->csp_auth_key) return ESPGPU_EINVAL;
      if (csp->csp_auth_mlen > hashlen || (csp->csp_auth_mlen & 3)) return ESPGPU_EINVAL;
      return ESPGPU_PROBE_HARDWARE;
    default:
      return ESPGPU_EINVAL;
  }
}

// (for parameters probe_caps accepted: an ETA or DIGEST session's algorithm
// is one hmac_hashlen knows)
void session_filed(const espgpu_session_params *csp, uint32_t *mode, uint32_t *mlen) {
  const int m = csp->csp_mode;
  // CSP_MODE_CIPHER sessions run in the ETA kernels (aalg 0: no MAC pass)
  *mode = (uint32_t)(m == ESPGPU_CSP_MODE_CIPHER ? ESPGPU_CSP_MODE_ETA : m);
  // mlen 0 = the whole tag, or the whole hash (swcr_setup_auth,
  // cryptosoft.c:1013-1018); no ICV without auth
  *mlen = m == ESPGPU_CSP_MODE_CIPHER ? 0u
        : csp->csp_auth_mlen          ? (uint32_t)csp->csp_auth_mlen
        : m == ESPGPU_CSP_MODE_AEAD   ? 16u
                                      : (uint32_t)hmac_hashlen(csp->csp_auth_alg);
}

namespace {

uint32_t bswap(uint32_t v) { return __builtin_bswap32(v); }
uint32_t ror16(uint32_t v) { return (v >> 16) | (v << 16); }

// The ETA-kernel session counter a session belongs to: which decrypt and
// cipher-pass kernels a batch may need (launch_eta kinds).  ESP-NULL sessions
// need no cipher pass; they count as CTR so that no CBC pass is launched.
int &eta_count(espgpu_ctx *c, const Session &s) {
  const bool ctr = s.ctr || s.null;
  return s.wide ? (ctr ? c->n_wctr : c->n_wcbc) : (ctr ? c->n_ctr : c->n_cbc);
}

}  // namespace
}  // namespace espgpu

using namespace espgpu;

extern "C" {

// The driver's bid: what the engine serves, AH only when it is offered.
int espgpu_probesession(const espgpu_session_params *csp) {
  const int r = probe_caps(csp);
  if (r == ESPGPU_PROBE_HARDWARE && csp->csp_mode == ESPGPU_CSP_MODE_DIGEST && !ah_offered()) return ESPGPU_EINVAL;
  return r;
}

int espgpu_newsession(espgpu_ctx *c, const espgpu_session_params *csp, int32_t *sid_out) {
  if (!c || !csp || !sid_out) return ESPGPU_EINVAL;
  if (c->failed) return ESPGPU_EIO;                  // (espgpu_last_error keeps the cause)
  int pr = probe_caps(csp);                          // (served whether or not the driver bids for it)
  if (pr >= 0) return fail(c, ESPGPU_EINVAL, "session parameters not supported");
  const bool digest = csp->csp_mode == ESPGPU_CSP_MODE_DIGEST;
  const bool null_cipher = csp->csp_cipher_alg == ESPGPU_CRYPTO_NULL_CBC || digest;
  if (!csp->csp_cipher_key && !null_cipher)
    return fail(c, ESPGPU_EINVAL, "per-request keys are not supported; session key required");
  int slot = -1;
  for (size_t i = 0; i < c->sessions.size(); ++i)
    if (!c->sessions[i].used) { slot = (int)i; break; }
  if (slot < 0) {
    if (c->sessions.size() >= c->cfg.max_sessions) return fail(c, ESPGPU_ENOMEM, "SA table full (%u)", c->cfg.max_sessions);
    slot = (int)c->sessions.size();
    c->sessions.emplace_back();
  }
  DevSA sa;
  memset(&sa, 0, sizeof sa);
  const uint8_t *key = (const uint8_t *)csp->csp_cipher_key;
  uint32_t rk[60];
  const int nr = null_cipher ? 0 : hc::aes_expand_enc(key, csp->csp_cipher_klen, rk);
  sa.nr = (uint32_t)nr;
  session_filed(csp, &sa.mode, &sa.mlen);
  sa.flags = (uint32_t)csp->csp_flags;
  if (csp->csp_mode == ESPGPU_CSP_MODE_AEAD) {
    // kernel form: raw first round, ror16 middle rounds, byte-swapped last round
    for (int i = 0; i < 4; ++i) sa.rk[i] = rk[i];
    for (int i = 4; i < 4 * nr; ++i) sa.rk[i] = ror16(rk[i]);
    for (int i = 0; i < 4; ++i) sa.rk[4 * nr + i] = bswap(rk[4 * nr + i]);
    uint8_t zero[16] = {0}, h[16];
    hc::aes_encrypt_block(rk, nr, zero, h);       // H = E_K(0^128), gmac.c:56-60
    std::vector<uint8_t> tabs(kGhTableBytes);
    hc::ghash_tables(h, tabs.data());
    HIPCHK(c, hipMemcpy(c->d_gtab + (size_t)slot * kGhTableBytes, tabs.data(), kGhTableBytes, hipMemcpyHostToDevice));
  } else {
    const bool auth = csp->csp_mode == ESPGPU_CSP_MODE_ETA || digest;
    const int aalg = auth ? csp->csp_auth_alg : 0;
    const bool sha256 = aalg == ESPGPU_CRYPTO_SHA2_256_HMAC;
    const bool wide = aalg == ESPGPU_CRYPTO_SHA2_384_HMAC || aalg == ESPGPU_CRYPTO_SHA2_512_HMAC;
    sa.calg = (uint32_t)csp->csp_cipher_alg;
    sa.aalg = (uint32_t)aalg;
    if (!null_cipher) {
      for (int i = 0; i < 4 * (nr + 1); ++i) sa.rk[i] = rk[i];
      uint32_t dk[60];
      hc::aes_expand_dec(key, csp->csp_cipher_klen, dk);
      for (int i = 0; i < 4 * (nr + 1); ++i) sa.dk[i] = dk[i];
    }
    const uint8_t *ak = (const uint8_t *)csp->csp_auth_key;
    if (!auth) {
    } else if (wide) {
      const bool is384 = aalg == ESPGPU_CRYPTO_SHA2_384_HMAC;
      hc::hmac_sha512_pad_state(ak, csp->csp_auth_klen, 0x36, is384, sa.ipad);
      hc::hmac_sha512_pad_state(ak, csp->csp_auth_klen, 0x5c, is384, sa.opad);
    } else if (sha256) {
      hc::hmac_sha256_pad_state(ak, csp->csp_auth_klen, 0x36, sa.ipad);
      hc::hmac_sha256_pad_state(ak, csp->csp_auth_klen, 0x5c, sa.opad);
    } else {
      hc::hmac_sha1_pad_state(ak, csp->csp_auth_klen, 0x36, sa.ipad);
      hc::hmac_sha1_pad_state(ak, csp->csp_auth_klen, 0x5c, sa.opad);
    }
  }
  HIPCHK(c, hipMemcpy(c->d_sas + slot, &sa, sizeof sa, hipMemcpyHostToDevice));
  Session &s = c->sessions[slot];
  s.used = true;
  s.mode = csp->csp_mode;
  s.flags = csp->csp_flags;
  s.mlen = (int)sa.mlen;
  s.klen = csp->csp_cipher_klen;
  const bool eta_kind = csp->csp_mode != ESPGPU_CSP_MODE_AEAD && !digest;
  s.ctr = eta_kind && csp->csp_cipher_alg == ESPGPU_CRYPTO_AES_ICM;
  s.null = eta_kind && null_cipher;
  s.whash = (eta_kind || digest) && (sa.aalg == ESPGPU_CRYPTO_SHA2_384_HMAC || sa.aalg == ESPGPU_CRYPTO_SHA2_512_HMAC);
  s.wide = s.whash || (eta_kind && (sa.aalg == 0 || null_cipher));
  if (eta_kind) {
    c->n_eta++;
    eta_count(c, s)++;
    c->n_whash += s.whash ? 1 : 0;
  } else if (digest) {
    c->n_dig++;
    c->n_dig_wide += s.whash ? 1 : 0;
  } else {
    c->n_gcm++;
  }
  *sid_out = slot;
  return 0;
}

int espgpu_session_room(espgpu_ctx *c) {
  if (!c) return ESPGPU_EINVAL;
  size_t room = c->cfg.max_sessions - c->sessions.size();
  for (const Session &s : c->sessions) room += s.used ? 0 : 1;
  return (int)std::min<size_t>(room, INT32_MAX);
}

void espgpu_freesession(espgpu_ctx *c, int32_t sid) {
  if (!c || sid < 0 || (size_t)sid >= c->sessions.size() || !c->sessions[sid].used) return;
  if (!c->failed) {
    // Requests already staged were accepted under this key: launch them now
    // (and the overflow behind them), then wait, so neither they nor flushed
    // batches see the slot reused.
    // (doorbell jobs have no stream to wait on: drain them)
    if (c->ovf.empty() && !c->door_ctl) espgpu_flush(c);
    else espgpu_drain(c);
  }
  if (!c->failed) {
    // the doorbell kernel keeps its current session's state (H^8 table in LDS);
    // stopped before the stream syncs, which could otherwise wait behind it
    // on a shared hardware queue
    door_stop(c);
    hipStreamSynchronize(c->stream);
    hipStreamSynchronize(c->s_out);
    for (auto &sl : c->slots) hipStreamSynchronize(sl.st);
    // and the ctx's last launch on any stream: a device-resident batch on the
    // caller's stream may still be reading this slot's keys
    if (c->launched) hipEventSynchronize(c->ev_last);
  }
  const Session &fs = c->sessions[sid];
  if (fs.mode == ESPGPU_CSP_MODE_DIGEST) {
    c->n_dig--;
    c->n_dig_wide -= fs.whash ? 1 : 0;
  } else if (fs.mode != ESPGPU_CSP_MODE_AEAD) {
    c->n_eta--;
    eta_count(c, fs)--;
    c->n_whash -= fs.whash ? 1 : 0;
  } else {
    c->n_gcm--;
  }
  c->sessions[sid] = Session();
  DevSA z;
  memset(&z, 0, sizeof z);
  if (!c->failed) hipMemcpy(c->d_sas + sid, &z, sizeof z, hipMemcpyHostToDevice);
}

}  // extern "C"
