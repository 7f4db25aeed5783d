// CPU self-test of the inbound classification rule's reads (f-stack_amd/csrc/
// classify.h: esp_classify_rule, the function behind espgpu_esp_classify and
// cls_kernel): packets of every kind the rule tells apart, cut to every length
// 0 .. 80, each in a heap block of exactly that size, against SPI tables in
// heap blocks of exactly nslots entries (one of them a chain that wraps past
// the end).  Built with the host compiler's -fsanitize=address,undefined, so a
// read outside [pkt, pkt + len) or outside the table ends the run.  The result
// must also not depend on anything but those bytes: the same packet inside a
// larger block with other bytes around it classifies the same.
// Run by tests/test_classify_selftest.py.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

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

uint32_t rnd_state = 12345;
uint32_t rnd() {
  rnd_state = rnd_state * 1664525u + 1013904223u;
  return rnd_state >> 8;
}

void put16(uint8_t *p, uint32_t v) {
  p[0] = (uint8_t)(v >> 8);
  p[1] = (uint8_t)v;
}
void put32(uint8_t *p, uint32_t v) {
  put16(p, v >> 16);
  put16(p + 2, v);
}

void set_cksum(uint8_t *h, uint32_t hlen) {
  h[10] = h[11] = 0;
  uint32_t s = 0;
  for (uint32_t k = 0; k < hlen; k += 2) s += (uint32_t)h[k] << 8 | h[k + 1];
  while (s >> 16) s = (s & 0xffff) + (s >> 16);
  put16(h + 10, ~s & 0xffff);
}

// a 96-byte image of a packet; the tests cut it
struct Image {
  uint8_t b[96];
};

Image ipv4(uint32_t ihl, uint32_t ip_len, uint32_t off, uint8_t proto, const uint8_t dst[4], uint32_t spi) {
  Image im;
  for (auto &x : im.b) x = (uint8_t)rnd();
  im.b[0] = (uint8_t)(0x40 | ihl);
  put16(im.b + 2, ip_len);
  put16(im.b + 6, off);
  im.b[9] = proto;
  memcpy(im.b + 16, dst, 4);
  if (ihl >= 5) set_cksum(im.b, ihl * 4);
  if (ihl >= 5) put32(im.b + ihl * 4, spi);
  return im;
}

Image ipv6(uint32_t plen, uint8_t nxt, const uint8_t dst[16], uint32_t spi) {
  Image im;
  for (auto &x : im.b) x = (uint8_t)rnd();
  im.b[0] = 0x60;
  put16(im.b + 4, plen);
  im.b[6] = nxt;
  memcpy(im.b + 24, dst, 16);
  put32(im.b + 40, spi);
  return im;
}

struct Heap {            // an exact-size heap block
  uint8_t *p;
  explicit Heap(size_t n) : p((uint8_t *)malloc(n ? n : 1)) {}
  ~Heap() { free(p); }
};

int same(const espgpu_desc &a, const espgpu_desc &b) { return !memcmp(&a, &b, sizeof(a)); }

long runs = 0, accepted = 0;

void cut_and_run(const espgpu_sad_entry *table, uint32_t nslots, const Image &im) {
  for (uint32_t flags = 0; flags <= ESPGPU_CLS_IPCSUM; ++flags) {
    for (uint32_t len = 0; len <= 80; ++len) {
      Heap h(len);
      memcpy(h.p, im.b, len);
      espgpu_desc d1, d2;
      memset(&d1, 0xdd, sizeof(d1));
      memset(&d2, 0xee, sizeof(d2));
      const int s1 = esp_classify_rule(table, nslots, h.p, len, 1000, flags, &d1);
      // the same bytes at an odd address among other bytes
      Heap g(len + 13);
      memset(g.p, (int)(rnd() & 0xff), len + 13);
      memcpy(g.p + 5, im.b, len);
      const int s2 = esp_classify_rule(table, nslots, g.p + 5, len, 1000, flags, &d2);
      CHECK(s1 == s2 && same(d1, d2));
      CHECK(s1 == 0 || s1 == ESPGPU_EINVAL || s1 == ESPGPU_ENOTSUP || s1 == ESPGPU_ENOENT);
      if (s1) {
        CHECK(d1.off4 == 1000 && d1.len == 0 && d1.sa == 0xffff && d1.esn_hi == 0 && d1.salt == 0);
      } else {
        CHECK(d1.off4 > 1000 && d1.len >= 8 && (d1.off4 - 1000) * 4 + d1.len <= len && d1.esn_hi == 0);
        ++accepted;
      }
      if (len < 20) CHECK(s1 == ESPGPU_EINVAL);
      ++runs;
    }
  }
}

}  // namespace

int main() {
  // the SAs: a chain of SPIs with home slot 6 of 8 (wraps to 0, 1) and one elsewhere
  std::vector<espgpu_sad_entry> sas;
  std::vector<uint32_t> chain;
  for (uint32_t s = 0x100; chain.size() < 5; ++s)
    if ((key_u32hash(s) & 7) == 6) chain.push_back(s);
  const uint8_t d4[4] = {10, 1, 2, 3};
  uint8_t d6[16], ll[16];
  for (int k = 0; k < 16; ++k) d6[k] = (uint8_t)(0x20 + k);
  memcpy(ll, d6, 16);
  ll[0] = 0xfe;
  ll[1] = 0x80;
  for (uint32_t k = 0; k < 4; ++k) {
    espgpu_sad_entry e;
    memset(&e, 0, sizeof(e));
    e.spi = chain[k];
    e.sa = (uint16_t)(k + 1);
    e.proto = k == 3 ? 51 : 50;
    e.af = k & 1 ? 6 : 4;
    e.salt = 0x01020304u * (k + 1);
    memcpy(e.dst, k & 1 ? d6 : d4, k & 1 ? 16 : 4);
    sas.push_back(e);
  }
  const uint32_t spi4 = chain[0], spi6 = chain[1], spi4b = chain[2], spi_ah = chain[3], spi_miss = chain[4];

  for (uint32_t nslots : {8u, 16u, 1024u}) {
    Heap tb((size_t)nslots * sizeof(espgpu_sad_entry));
    espgpu_sad_entry *table = (espgpu_sad_entry *)tb.p;
    CHECK(sad_build(sas.data(), (uint32_t)sas.size(), table, nslots) == 0);
    if (nslots == 8) CHECK(table[6].spi == chain[0] && table[7].spi == chain[1] && table[0].spi == chain[2] &&
                           table[1].spi == chain[3] && table[2].spi == 0);
    std::vector<Image> ims;
    for (uint32_t ihl = 0; ihl <= 15; ++ihl)                       // every header length, right and wrong
      ims.push_back(ipv4(ihl, ihl * 4 + 16, 0, 50, d4, spi4));
    for (uint32_t ip_len : {0u, 19u, 20u, 24u, 27u, 28u, 29u, 44u, 60u, 80u, 81u, 1500u, 65535u})
      ims.push_back(ipv4(5, ip_len, 0, 50, d4, spi4b));
    for (uint32_t off : {0x2000u, 0x0001u, 0x1fffu, 0x4000u, 0x8000u})
      ims.push_back(ipv4(5, 44, off, 50, d4, spi4));
    for (uint32_t proto : {51u, 6u, 17u, 108u, 0u})
      ims.push_back(ipv4(6, 48, 0, (uint8_t)proto, d4, spi4));
    for (uint32_t spi : {0u, spi_miss, spi_ah, spi6, 0xffffffffu})   // lookups that fail, each its own way
      ims.push_back(ipv4(5, 44, 0, 50, d4, spi));
    ims.push_back(ipv4(5, 44, 0, 50, d6, spi4));                    // wrong destination
    for (uint32_t v : {0u, 1u, 5u, 7u, 15u}) {                      // versions
      Image im = ipv4(5, 44, 0, 50, d4, spi4);
      im.b[0] = (uint8_t)(v << 4 | 5);
      ims.push_back(im);
    }
    for (uint32_t plen : {0u, 1u, 7u, 8u, 9u, 12u, 24u, 39u, 40u, 41u, 1460u, 65535u})
      ims.push_back(ipv6(plen, 50, d6, spi6));
    for (uint32_t nxt : {0u, 43u, 44u, 51u, 60u, 17u})
      ims.push_back(ipv6(24, (uint8_t)nxt, d6, spi6));
    ims.push_back(ipv6(24, 50, ll, spi6));                          // link-local
    for (uint32_t spi : {0u, spi_miss, spi_ah, spi4})
      ims.push_back(ipv6(24, 50, d6, spi));
    {
      Image im = ipv6(24, 50, d6, spi6);                            // wrong in the last byte
      im.b[39] ^= 1;
      ims.push_back(im);
    }
    for (int k = 0; k < 200; ++k) {                                 // noise
      Image im;
      for (auto &x : im.b) x = (uint8_t)rnd();
      if (k & 1) im.b[0] = (uint8_t)((k & 2 ? 0x40 : 0x60) | (im.b[0] & 0xf));
      ims.push_back(im);
    }
    for (const Image &im : ims) cut_and_run(table, nslots, im);
  }
  // a table with no free slot: the probe is bounded by nslots
  {
    Heap tb(4 * sizeof(espgpu_sad_entry));
    espgpu_sad_entry *table = (espgpu_sad_entry *)tb.p;
    for (uint32_t k = 0; k < 4; ++k) table[k] = sas[k];
    cut_and_run(table, 4, ipv4(5, 44, 0, 50, d4, spi_miss));
    cut_and_run(table, 4, ipv4(5, 44, 0, 50, d4, spi4b));
  }
  CHECK(accepted > 100);
  if (fails) return 1;
  printf("OK %ld runs, %ld accepted\n", runs, accepted);
  return 0;
}
