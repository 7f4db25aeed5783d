// CPU self-test of the inbound AH rules' reads and writes (f-stack_amd/csrc:
// classify.h's AH branch, ah_in.h's ah_input_rule and ah_decap_rule), each
// packet in a heap block of exactly its own size and each save slot in a block
// of exactly skip bytes.  Built with the host compiler's
// -fsanitize=address,undefined, so a read or a write outside a block ends the
// run.  What the rules write is checked against plain restatements.  Run by
// tests/test_ah_in_selftest.py.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "ah_in.h"
#include "classify.h"

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

uint32_t rnd_state = 5100;
uint32_t rnd() {
  rnd_state = rnd_state * 1664525u + 1013904223u;
  return rnd_state >> 8;
}

void put16(uint8_t *p, uint32_t v) {
  p[0] = (uint8_t)(v >> 8);
  p[1] = (uint8_t)v;
}

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

long n_in = 0, n_dcp = 0, n_ref = 0, n_cls = 0;

// well-formed options over [20, skip): NOPs, kept and zeroed options
void fill_options(uint8_t *h, uint32_t skip) {
  uint32_t off = 20;
  while (off < skip) {
    const uint32_t left = skip - off, r = rnd() % 10;
    if (left == 1 || r < 2) {
      h[off++] = 1;
      continue;
    }
    const uint32_t ln = 2 + rnd() % (left - 1);
    h[off] = (r & 1) ? kKeep[rnd() % 5] : kZero[rnd() % 4];
    h[off + 1] = (uint8_t)ln;
    for (uint32_t k = 2; k < ln; ++k) h[off + k] = (uint8_t)(1 + rnd() % 255);
    off += ln;
  }
}

// ah_massage_headers' IPv4 branch, byte by byte (xform_ah.c:291-393); -1: refused
int massage4(uint8_t *h, uint32_t skip, bool keeptos) {
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
    if (!keep) memset(h + off, 0, count);
    off += count;
  }
  return 0;
}

// One packet of the given shape through both rules.  q payload bytes behind
// the AH header; the block holds exactly the packet.
void one_packet(bool af6, uint32_t ihl, uint32_t mlen, uint32_t q, uint32_t nxt, uint32_t mode, bool keeptos) {
  const uint32_t skip = af6 ? 40 : ihl * 4, ahsize = ah_hdrsiz(mlen, af6), len = skip + ahsize + q;
  const uint32_t flags = mode | (af6 ? ESPGPU_IN_AF6 : 0) | ESPGPU_IN_AH | (keeptos ? ESPGPU_IN_AH_KEEPTOS : 0);
  Heap pk(len), slot(skip);
  for (uint32_t k = 0; k < len; ++k) pk.p[k] = (uint8_t)rnd();
  if (af6) {
    pk.p[0] = (uint8_t)(0x60 | (rnd() & 0xf));
    put16(pk.p + 4, ahsize + q);
    pk.p[6] = 51;
    if (rnd() & 1) {                                   // a link-local source
      pk.p[8] = 0xfe;
      pk.p[9] = (uint8_t)(0x80 | (rnd() & 0x3f));
    } else {
      pk.p[8] = 0x20;
    }
    pk.p[24] = (rnd() & 3) ? 0x20 : 0xfe;
    if (pk.p[24] == 0xfe) pk.p[25] = 0x80;
  } else {
    pk.p[0] = (uint8_t)(0x40 | ihl);
    put16(pk.p + 2, len);
    pk.p[9] = 51;
    fill_options(pk.p, skip);
    put16(pk.p + 10, 0);
    put16(pk.p + 10, cksum(pk.p, skip));
  }
  pk.p[skip] = (uint8_t)nxt;
  pk.p[skip + 1] = (uint8_t)((ahsize - 8) / 4);
  std::vector<uint8_t> orig(pk.p, pk.p + len), want(orig);
  if (af6) {
    want[0] = 0x60;
    want[1] = want[2] = want[3] = 0;
    want[7] = 0;
    for (uint32_t a : {8u, 24u})
      if (want[a] == 0xfe && (want[a + 1] & 0xc0) == 0x80) want[a + 2] = want[a + 3] = 0;
  } else {
    CHECK(massage4(want.data(), skip, keeptos) == 0);
  }
  memset(slot.p, 0xA5, skip);
  CHECK(ah_input_rule(flags, mlen, pk.p, len, skip + 12, slot.p) == 0);
  ++n_in;
  CHECK(memcmp(pk.p, want.data(), len) == 0);
  CHECK(memcmp(slot.p, orig.data(), skip) == 0);
  // one byte short of the AH header: refused, nothing written
  {
    Heap sh(skip + ahsize - 1), s2(skip);
    memcpy(sh.p, orig.data(), skip + ahsize - 1);
    memset(s2.p, 0xA5, skip);
    CHECK(ah_input_rule(flags, mlen, sh.p, skip + ahsize - 1, skip + 12, s2.p) == ESPGPU_EACCES);
    CHECK(memcmp(sh.p, orig.data(), skip + ahsize - 1) == 0);
    for (uint32_t k = 0; k < skip; ++k) CHECK(s2.p[k] == 0xA5);
    ++n_ref;
  }
  // the decapsulation, in place
  DecapPlan pl;
  std::vector<uint8_t> before(pk.p, pk.p + len);
  const int st = ah_decap_rule(flags, mlen, pk.p, len, skip + 12, slot.p, &pl);
  ++n_dcp;
  const bool inner = (nxt == 4 || nxt == 41) && mode != ESPGPU_IN_TRANSPORT;
  int wst = 0;
  if (inner)
    wst = q < (nxt == 4 ? 20u : 40u) ? ESPGPU_EINVAL : 0;
  else if (!af6 && mode == ESPGPU_IN_TUNNEL)
    wst = ESPGPU_EPFNOSUPPORT;
  CHECK(st == wst);
  CHECK(memcmp(slot.p, orig.data(), skip) == 0);
  if (st != 0 || inner) {
    CHECK(memcmp(pk.p, before.data(), len) == 0);
    if (st == 0) CHECK(pl.off == skip + ahsize && pl.len == q && !pl.transport);
    return;
  }
  CHECK(pl.transport && pl.off == ahsize && pl.len == skip + q);
  std::vector<uint8_t> hdr(orig.begin(), orig.begin() + skip);
  if (af6) {
    hdr[6] = (uint8_t)nxt;
    put16(hdr.data() + 4, q);
  } else {
    hdr[9] = (uint8_t)nxt;
    put16(hdr.data() + 2, skip + q);
    put16(hdr.data() + 10, 0);
    put16(hdr.data() + 10, cksum(hdr.data(), skip));
  }
  CHECK(memcmp(pk.p + ahsize, hdr.data(), skip) == 0);
  CHECK(memcmp(pk.p, before.data(), ahsize) == 0);
  CHECK(memcmp(pk.p + ahsize + skip, before.data() + ahsize + skip, q) == 0);
}

// The option loop's refusals with the offending byte the last of the header:
// through the rule, in a block of exactly the packet, and through the walk
// alone over a block that ends with the header, so that a read one byte on
// (the option length the loop must not look for) is a read outside the block.
void option_refusals() {
  for (uint32_t ihl = 6; ihl <= 15; ++ihl)
    for (uint32_t kind = 0; kind < 4; ++kind)
      for (uint32_t t = 0; t < 9; ++t) {
        const uint32_t skip = ihl * 4, len = skip + 24;
        const uint8_t type = t < 5 ? kKeep[t] : kZero[t - 5];
        const uint8_t tails[4][2] = {{type, 0}, {type, 0}, {type, 1}, {type, 3}};
        const uint32_t tl = kind == 0 ? 1 : 2;
        Heap pk(len), slot(skip);
        for (uint32_t k = 0; k < len; ++k) pk.p[k] = (uint8_t)rnd();
        pk.p[0] = (uint8_t)(0x40 | ihl);
        fill_options(pk.p, skip - tl);
        memcpy(pk.p + skip - tl, tails[kind], tl);
        pk.p[skip + 1] = 4;
        std::vector<uint8_t> orig(pk.p, pk.p + len);
        memset(slot.p, 0xA5, skip);
        CHECK(ah_input_rule(ESPGPU_IN_AH, 12, pk.p, len, skip + 12, slot.p) == ESPGPU_EINVAL);
        ++n_ref;
        CHECK(memcmp(pk.p, orig.data(), len) == 0);
        for (uint32_t k = 0; k < skip; ++k) CHECK(slot.p[k] == 0xA5);
        // the walk alone over a block that ends with the header
        Heap hd(skip);
        memcpy(hd.p, orig.data(), skip);
        uint64_t z = 0;
        CHECK(ah_opt_walk<false>(hd.p, skip, &z) == ESPGPU_EINVAL);
        // EOL or NOP in that last byte: accepted
        for (uint8_t last : {(uint8_t)0, (uint8_t)1}) {
          memcpy(pk.p, orig.data(), len);
          fill_options(pk.p, skip - 1);
          pk.p[skip - 1] = last;
          CHECK(ah_input_rule(ESPGPU_IN_AH, 12, pk.p, len, skip + 12, slot.p) == 0);
          ++n_in;
        }
      }
}

// classification of AH packets in blocks of exactly their length
void classification() {
  espgpu_sad_entry sas[2];
  memset(sas, 0, sizeof(sas));
  sas[0].spi = 0x11223344;
  sas[0].sa = 3;
  sas[0].proto = 51;
  sas[0].af = 4;
  const uint8_t d4[4] = {10, 9, 8, 7};
  memcpy(sas[0].dst, d4, 4);
  sas[1].spi = 0x55667788;
  sas[1].sa = 4;
  sas[1].proto = 51;
  sas[1].af = 6;
  for (int k = 0; k < 16; ++k) sas[1].dst[k] = (uint8_t)(0x20 + k);
  std::vector<espgpu_sad_entry> table(8);
  CHECK(sad_build(sas, 2, table.data(), 8) == 0);
  const uint8_t spi4[4] = {0x11, 0x22, 0x33, 0x44}, spi6[4] = {0x55, 0x66, 0x77, 0x88};
  for (uint32_t plen = 0; plen <= 40; ++plen) {
    for (uint32_t ihl = 5; ihl <= 15; ++ihl) {
      const uint32_t total = ihl * 4 + plen;
      Heap h(total);
      for (uint32_t k = 0; k < total; ++k) h.p[k] = (uint8_t)rnd();
      h.p[0] = (uint8_t)(0x40 | ihl);
      put16(h.p + 2, total);
      put16(h.p + 6, 0);
      h.p[9] = 51;
      memcpy(h.p + 16, d4, 4);
      if (plen >= 8) memcpy(h.p + ihl * 4 + 4, spi4, 4);
      espgpu_desc d;
      const int st = esp_classify_rule(table.data(), 8, h.p, total, 100, ESPGPU_CLS_AH, &d);
      ++n_cls;
      CHECK(st == (plen < 12 ? ESPGPU_EINVAL : 0));
      if (st == 0) CHECK(d.off4 == 100 && d.len == total && d.sa == 3 && d.salt == ihl * 4 + 12 && d.esn_hi == 0);
      CHECK(esp_classify_rule(table.data(), 8, h.p, total, 100, 0, &d) == ESPGPU_ENOTSUP);
    }
    const uint32_t total = 40 + plen;
    Heap h(total);
    for (uint32_t k = 0; k < total; ++k) h.p[k] = (uint8_t)rnd();
    h.p[0] = 0x60;
    put16(h.p + 4, plen);
    h.p[6] = 51;
    memcpy(h.p + 24, sas[1].dst, 16);
    if (plen >= 8) memcpy(h.p + 44, spi6, 4);
    espgpu_desc d;
    const int st = esp_classify_rule(table.data(), 8, h.p, total, 100, ESPGPU_CLS_AH, &d);
    ++n_cls;
    CHECK(st == (plen == 0 ? ESPGPU_ENOTSUP : plen < 12 ? ESPGPU_EINVAL : 0));
    if (st == 0) CHECK(d.off4 == 100 && d.len == total && d.sa == 4 && d.salt == 52);
  }
}

}  // namespace

int main() {
  const uint32_t modes[3] = {0, ESPGPU_IN_TRANSPORT, ESPGPU_IN_TUNNEL};
  const uint32_t nxts[5] = {4, 41, 6, 17, 50};
  for (int af6 = 0; af6 < 2; ++af6)
    for (uint32_t ihl = 5; ihl <= (af6 ? 5u : 15u); ++ihl)
      for (uint32_t mlen : kMlens)
        for (uint32_t mode : modes)
          for (uint32_t nxt : nxts)
            for (uint32_t q : {0u, 1u, 19u, 20u, 39u, 40u, 57u})
              one_packet(af6, ihl, mlen, q, nxt, mode, (q ^ ihl) & 1);
  option_refusals();
  classification();
  if (fails) {
    printf("FAILED %d checks\n", fails);
    return 1;
  }
  printf("OK %ld packets massaged, %ld decapsulated, %ld refused, %ld classified\n", n_in, n_dcp, n_ref, n_cls);
  return 0;
}
