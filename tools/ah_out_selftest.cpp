// CPU self-test of the outbound AH rules' reads and writes (f-stack_amd/csrc:
// ah_out.h's ah_encap_rule, ah_frame_rule and ah_sent_rule): headroom and
// packet together in a heap block of exactly ahsize + oh + len bytes and each
// save slot in a block of exactly hs bytes.  Built with the host compiler's
// -fsanitize=address,undefined, so a read or a write outside a block ends the
// run.  What the rules write is checked against plain restatements.  Run by
// tests/test_ah_out_selftest.py.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "ah_out.h"

using namespace espgpu;

namespace {

int fails = 0;
#define CHECK(c)                                                   \
  do {                                                             \
    if (!(c)) {                                                    \
      printf("FAIL line %d: %s\n", __LINE__, #c);                  \
      if (++fails > 20) exit(1);                                   \
    }                                                              \
  } while (0)

uint32_t rnd_state = 5200;
uint32_t rnd() {
  rnd_state = rnd_state * 1664525u + 1013904223u;
  return rnd_state >> 8;
}

void put16(uint8_t *p, uint32_t v) {
  p[0] = (uint8_t)(v >> 8);
  p[1] = (uint8_t)v;
}
uint32_t get16(const uint8_t *p) { return (uint32_t)p[0] << 8 | p[1]; }

uint32_t cksum(const uint8_t *h, uint32_t n) {
  uint32_t s = 0;
  for (uint32_t k = 0; k + 1 < n; k += 2) s += (uint32_t)h[k] << 8 | h[k + 1];
  while (s >> 16) s = (s & 0xffff) + (s >> 16);
  return ~s & 0xffff;
}

struct Heap {            // an exact-size heap block
  uint8_t *p;
  explicit Heap(size_t n) : p((uint8_t *)malloc(n ? n : 1)) {}
  ~Heap() { free(p); }
};

const uint32_t kMlens[4] = {12, 16, 24, 32};
const uint8_t kKeep[5] = {0x82, 0x85, 0x86, 0x94, 0x95};
const uint8_t kZero[4] = {0x83, 0x89, 0x44, 0x07};

long n_enc = 0, n_ref = 0, n_frm = 0, n_snt = 0;

// well-formed options over [20, skip): NOPs, kept and zeroed options, source
// routes of 4 bytes at least
void fill_options(uint8_t *h, uint32_t skip) {
  uint32_t off = 20;
  while (off < skip) {
    const uint32_t left = skip - off, r = rnd() % 10;
    if (left == 1 || r < 2) {
      h[off++] = 1;
      continue;
    }
    uint32_t ln = 2 + rnd() % (left - 1);
    h[off] = (r & 1) ? kKeep[rnd() % 5] : kZero[rnd() % 4];
    if ((h[off] == 0x83 || h[off] == 0x89) && ln < 4) {
      if (left < 4) {
        h[off] = 0x44;
      } else {
        ln = 4;
      }
    }
    h[off + 1] = (uint8_t)ln;
    for (uint32_t k = 2; k < ln; ++k) h[off + k] = (uint8_t)(1 + rnd() % 255);
    off += ln;
  }
}

// ah_massage_headers' IPv4 branch with out = 1, byte by byte
// (xform_ah.c:291-393); -1: refused
int massage4_out(uint8_t *h, uint32_t skip, bool keeptos) {
  if (!keeptos) h[1] = 0;
  h[8] = 0;
  h[10] = h[11] = 0;
  h[6] = h[7] = 0;
  for (uint32_t off = 20; off < skip;) {
    if (!(h[off] == 0 || h[off] == 1 || off + 1 < skip)) return -1;
    if (h[off] == 0) break;
    if (h[off] == 1) {
      ++off;
      continue;
    }
    const uint32_t count = h[off + 1];
    if (count < 2) return -1;
    if (off + count > skip) return -1;
    bool keep = false;
    for (uint8_t k : kKeep) keep |= h[off] == k;
    if (h[off] == 0x83 || h[off] == 0x89) {
      if (count < 4) return -1;
      memcpy(h + 16, h + off + count - 4, 4);
    }
    if (!keep) memset(h + off, 0, count);
    off += count;
  }
  return 0;
}

espgpu_encsa make_sa(bool af6, bool tunnel, bool keeptos) {
  espgpu_encsa e;
  memset(&e, 0, sizeof(e));
  e.flags = ESPGPU_ENC_AH | (af6 ? ESPGPU_ENC_AF6 : 0) | (tunnel ? ESPGPU_ENC_TUNNEL : 0) |
            (keeptos ? ESPGPU_ENC_AH_KEEPTOS : 0) | ESPGPU_ENC_ECN_NOCARE;
  e.ttl = (uint8_t)(1 + rnd() % 255);
  for (uint32_t k = 0; k < (af6 ? 16u : 4u); ++k) {
    e.src[k] = (uint8_t)(1 + rnd() % 254);
    e.dst[k] = (uint8_t)(1 + rnd() % 254);
  }
  e.src[0] = e.dst[0] = 0x20;
  return e;
}

// A cleartext packet of the family into blk + front: transport packets carry
// the SA's destination.
void make_packet(uint8_t *p, bool in6, uint32_t ihl, uint32_t len, const espgpu_encsa &e, bool transport) {
  for (uint32_t k = 0; k < len; ++k) p[k] = (uint8_t)rnd();
  if (in6) {
    p[0] = (uint8_t)(0x60 | (rnd() & 0xf));
    put16(p + 4, len - 40);
    p[8] = (rnd() & 1) ? 0xfe : 0x20;                  // a link-local source now and then
    if (p[8] == 0xfe) p[9] = (uint8_t)(0x80 | (rnd() & 0x3f));
    p[24] = 0x20;
    if (transport) memcpy(p + 24, e.dst, 16);
  } else {
    p[0] = (uint8_t)(0x40 | ihl);
    put16(p + 2, len);
    p[16] = 0x20;
    if (transport) memcpy(p + 16, e.dst, 4);
    fill_options(p, ihl * 4);
    put16(p + 10, 0);
    put16(p + 10, cksum(p, ihl * 4));
  }
}

// One packet of the given shape through the three rules.
void one_packet(bool af6, bool in6, uint32_t ihl, uint32_t mlen, bool tunnel, uint32_t q, bool keeptos) {
  const bool encap = tunnel || af6 != in6;
  const uint32_t skip = in6 ? 40 : ihl * 4, len = skip + q, ahsize = ah_hdrsiz(mlen, af6);
  const uint32_t oh = encap ? (af6 ? 40u : 20u) : 0u, front = ahsize + oh, hs = encap ? oh : skip;
  const espgpu_encsa e = make_sa(af6, tunnel, keeptos);
  Heap blk(front + len), slot(hs);
  for (uint32_t k = 0; k < front; ++k) blk.p[k] = (uint8_t)rnd();
  make_packet(blk.p + front, in6, ihl, len, e, !encap);
  std::vector<uint8_t> orig(blk.p, blk.p + front + len);
  memset(slot.p, 0xA5, hs);
  // one byte of headroom short: refused, nothing written
  {
    AhOutPlan pl;
    CHECK(ah_encap_rule(&e, mlen, blk.p + front, len, front - 1, 0x1234, slot.p, &pl) == ESPGPU_ENOBUFS);
    CHECK(memcmp(blk.p, orig.data(), front + len) == 0);
    for (uint32_t k = 0; k < hs; ++k) CHECK(slot.p[k] == 0xA5);
    ++n_ref;
  }
  AhOutPlan pl;
  CHECK(ah_encap_rule(&e, mlen, blk.p + front, len, front, 0x1234, slot.p, &pl) == 0);
  ++n_enc;
  CHECK(pl.ahsize == ahsize && pl.oh == oh && pl.total == front + len && pl.tunnel == encap);
  // the wire header
  std::vector<uint8_t> wire(hs);
  uint32_t nxt;
  if (encap) {
    nxt = in6 ? 41 : 4;
    if (af6) {
      const uint32_t tc = in6 ? (((uint32_t)orig[front] & 0xf) << 4 | orig[front + 1] >> 4) : orig[front + 1];
      wire[0] = (uint8_t)(0x60 | tc >> 4);
      wire[1] = (uint8_t)((tc & 0xf) << 4);
      put16(wire.data() + 4, front + len - 40);
      wire[6] = 51;
      wire[7] = e.ttl;
      memcpy(wire.data() + 8, e.src, 16);
      memcpy(wire.data() + 24, e.dst, 16);
    } else {
      wire[0] = 0x45;
      wire[1] = in6 ? (uint8_t)(((uint32_t)orig[front] & 0xf) << 4 | orig[front + 1] >> 4) : orig[front + 1];
      put16(wire.data() + 2, front + len);
      put16(wire.data() + 4, 0x1234);
      wire[8] = e.ttl;
      wire[9] = 51;
      memcpy(wire.data() + 12, e.src, 4);
      memcpy(wire.data() + 16, e.dst, 4);
      put16(wire.data() + 10, cksum(wire.data(), 20));
    }
  } else {
    memcpy(wire.data(), orig.data() + front, skip);
    if (in6) {
      nxt = wire[6];
      wire[6] = 51;
      put16(wire.data() + 4, front + len - 40);
    } else {
      nxt = wire[9];
      wire[9] = 51;
      put16(wire.data() + 2, front + len);
      put16(wire.data() + 10, 0);
      put16(wire.data() + 10, cksum(wire.data(), skip));
    }
  }
  CHECK(memcmp(slot.p, wire.data(), hs) == 0);
  // the hashed header
  std::vector<uint8_t> hashed(wire);
  if (af6) {
    hashed[0] = 0x60;
    hashed[1] = hashed[2] = hashed[3] = 0;
    hashed[7] = 0;
    for (uint32_t a : {8u, 24u})
      if (hashed[a] == 0xfe && (hashed[a + 1] & 0xc0) == 0x80) hashed[a + 2] = hashed[a + 3] = 0;
  } else {
    CHECK(massage4_out(hashed.data(), hs, keeptos) == 0);
  }
  CHECK(memcmp(blk.p, hashed.data(), hs) == 0);
  // the AH header: dword 0 and the padding written, SPI, sequence number and ICV field as they were
  CHECK(blk.p[hs] == nxt && blk.p[hs + 1] == (ahsize - 8) / 4 && blk.p[hs + 2] == 0 && blk.p[hs + 3] == 0);
  CHECK(memcmp(blk.p + hs + 4, orig.data() + hs + 4, 8 + mlen) == 0);
  for (uint32_t k = 12 + mlen; k < ahsize; ++k) CHECK(blk.p[hs + k] == 0);
  // behind it: the inner packet with its lengths fixed, or the payload
  if (encap) {
    std::vector<uint8_t> inner(orig.begin() + front, orig.end());
    if (!in6) {
      put16(inner.data() + 10, 0);
      put16(inner.data() + 10, cksum(inner.data(), skip));
    }
    CHECK(memcmp(blk.p + front, inner.data(), len) == 0);
  } else {
    CHECK(memcmp(blk.p + front + skip, orig.data() + front + skip, q) == 0);
  }
  // framing
  espgpu_outsa o;
  memset(&o, 0, sizeof(o));
  o.count = 0xfffffffdu;
  o.spi = 0xa1b2c3d4;
  uint32_t hi = 7;
  CHECK(ah_frame_rule(&o, blk.p, front + len, hs + 12, &hi) == 0 && hi == 0 && o.count == 0xfffffffeu);
  const uint8_t want8[8] = {0xa1, 0xb2, 0xc3, 0xd4, 0xff, 0xff, 0xff, 0xfe};
  CHECK(memcmp(blk.p + hs + 4, want8, 8) == 0);
  CHECK(ah_frame_rule(&o, blk.p, front + len, hs + 12, &hi) == 0 && o.count == 0xffffffffu);
  CHECK(ah_frame_rule(&o, blk.p, front + len, hs + 12, &hi) == ESPGPU_EACCES && o.count == 0xffffffffu);
  n_frm += 3;
  // the restore
  std::vector<uint8_t> mid(blk.p, blk.p + front + len);
  CHECK(ah_sent_rule(e.flags, blk.p, front + len, hs + 12, slot.p) == 0);
  ++n_snt;
  CHECK(memcmp(blk.p, wire.data(), hs) == 0);
  CHECK(memcmp(blk.p + hs, mid.data() + hs, front + len - hs) == 0);
  if (!af6) CHECK(cksum(blk.p, hs) == 0 && get16(blk.p + 2) == front + len);
}

// The option loop's refusals with the offending byte the last of the header,
// and the source routes shorter than 4 bytes: through the rule, in a block of
// exactly headroom and packet, and through the walk alone over a block that
// ends with the header.
void option_refusals() {
  for (uint32_t ihl = 6; ihl <= 15; ++ihl)
    for (uint32_t kind = 0; kind < 6; ++kind)
      for (uint32_t t = 0; t < 9; ++t) {
        const uint32_t skip = ihl * 4, len = skip + 9, front = 24;
        uint8_t type = t < 5 ? kKeep[t] : kZero[t - 5];
        if (kind >= 4) type = (t & 1) ? 0x83 : 0x89;
        const uint8_t tails[6][3] = {{type, 0, 0}, {type, 0, 0}, {type, 1, 0}, {type, 3, 0}, {type, 2, 0}, {type, 3, 9}};
        const uint32_t tl = kind == 0 ? 1 : kind == 5 ? 3 : 2;
        espgpu_encsa e = make_sa(false, false, false);
        Heap blk(front + len), slot(skip);
        for (uint32_t k = 0; k < front; ++k) blk.p[k] = (uint8_t)rnd();
        make_packet(blk.p + front, false, ihl, len, e, true);
        uint8_t *p = blk.p + front;
        fill_options(p, skip - tl);
        memcpy(p + skip - tl, tails[kind], tl);
        std::vector<uint8_t> orig(blk.p, blk.p + front + len);
        memset(slot.p, 0xA5, skip);
        AhOutPlan pl;
        CHECK(ah_encap_rule(&e, 12, p, len, front, 1, slot.p, &pl) == ESPGPU_EINVAL);
        ++n_ref;
        CHECK(memcmp(blk.p, orig.data(), front + len) == 0);
        for (uint32_t k = 0; k < skip; ++k) CHECK(slot.p[k] == 0xA5);
        Heap hd(skip);
        memcpy(hd.p, p, skip);
        uint64_t z = 0;
        bool sr = false;
        uint32_t d = 0;
        CHECK(ah_opt_walk<true>(hd.p, skip, &z, &sr, &d) == ESPGPU_EINVAL);
        // EOL or NOP in that last byte: accepted
        for (uint8_t last : {(uint8_t)0, (uint8_t)1}) {
          memcpy(blk.p, orig.data(), front + len);
          fill_options(p, skip - 1);
          p[skip - 1] = last;
          CHECK(ah_encap_rule(&e, 12, p, len, front, 1, slot.p, &pl) == 0);
          ++n_enc;
        }
      }
}

}  // namespace

int main() {
  for (int af6 = 0; af6 < 2; ++af6)
    for (int in6 = 0; in6 < 2; ++in6)
      for (uint32_t ihl = 5; ihl <= (in6 ? 5u : 15u); ++ihl)
        for (uint32_t mlen : kMlens)
          for (int tunnel = 0; tunnel < 2; ++tunnel)
            for (uint32_t q : {0u, 1u, 8u, 57u})
              one_packet(af6, in6, ihl, mlen, tunnel, q, (q ^ ihl) & 1);
  option_refusals();
  if (fails) {
    printf("FAILED %d checks\n", fails);
    return 1;
  }
  printf("OK %ld packets encapsulated, %ld refused, %ld numbered, %ld restored\n", n_enc, n_ref, n_frm, n_snt);
  return 0;
}
