// CPU self-test of the inbound decapsulation rule's reads and writes
// (f-stack_amd/csrc/decap.h: esp_decap_rule, the function behind
// espgpu_esp_decap and dcp_kernel): decrypted packets of every kind the rule
// tells apart, every ip_hl x hlen, each in a heap block of exactly skip + rlen
// bytes.  Built with the host compiler's -fsanitize=address,undefined, so a
// read or a write outside the packet ends the run.  The tunnel path must not
// touch the packet at all: it gets a block of one byte.  What the rule writes
// is checked against a plain restatement: the header moved by hlen with
// ip_len / ip_p / ip_sum (ip6_plen / ip6_nxt) set, nothing else changed.
// Run by tests/test_decap_selftest.py.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "decap.h"

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

uint32_t rnd_state = 54321;
uint32_t rnd() {
  rnd_state = rnd_state * 1664525u + 1013904223u;
  return rnd_state >> 8;
}

void put16(uint8_t *p, uint32_t v) {
  p[0] = (uint8_t)(v >> 8);
  p[1] = (uint8_t)v;
}

uint32_t cksum(const uint8_t *h, uint32_t hlen) {      // in_cksum: 0 for a header that is right
  uint32_t s = 0;
  for (uint32_t k = 0; k < hlen; k += 2) s += (uint32_t)h[k] << 8 | h[k + 1];
  while (s >> 16) s = (s & 0xffff) + (s >> 16);
  return ~s & 0xffff;
}

struct Heap {            // an exact-size heap block
  uint8_t *p;
  explicit Heap(size_t n) : p((uint8_t *)malloc(n ? n : 1)) {}
  ~Heap() { free(p); }
};

long runs = 0, accepted = 0, tunnels = 0;

// One packet: outer header of `skip` bytes (first byte `first`), a record of
// hlen + q + padlen + 2 + alen bytes whose trailer says padlen / nxt.
void run(uint32_t flags, uint32_t skip, uint8_t first, uint32_t ivlen, uint32_t alen, uint32_t q, uint32_t padlen,
         uint32_t nxt, uint32_t trflags) {
  const uint32_t hlen = 8 + ivlen, rlen = hlen + q + padlen + 2 + alen, total = skip + rlen;
  std::vector<uint8_t> img(total);
  for (auto &x : img) x = (uint8_t)rnd();
  img[0] = first;
  img[skip + hlen + q + padlen] = (uint8_t)padlen;
  img[skip + hlen + q + padlen + 1] = (uint8_t)nxt;
  const uint32_t trailer = nxt | padlen << 8 | ESPGPU_TR_VALID | trflags;
  // what the rule will decide, from the packet-free half alone (a one-byte block proves it is packet-free)
  DecapPlan plan;
  memset(&plan, 0, sizeof(plan));
  const int st0 = dcp_plan(flags, hlen, alen, skip, rlen, trailer, &plan);
  ++runs;
  if (st0 == 0 && !plan.transport) {
    Heap one(1);
    one.p[0] = 0xa5;
    DecapPlan p2;
    const int st = esp_decap_rule(flags, ivlen, alen, one.p, one.p, skip, rlen, trailer, &p2);
    CHECK(st == 0 && one.p[0] == 0xa5);
    CHECK(p2.off == skip + hlen && p2.len == q && p2.transport == 0);
    CHECK((nxt == 4 && q >= 20) || (nxt == 41 && q >= 40));
    ++tunnels;
    ++accepted;
    return;
  }
  Heap h(total);
  memcpy(h.p, img.data(), total);
  DecapPlan p;
  const int st = esp_decap_rule(flags, ivlen, alen, h.p, h.p, skip, rlen, trailer, &p);
  CHECK(st == 0 || st == ESPGPU_EINVAL || st == ESPGPU_ENODATA || st == ESPGPU_EPFNOSUPPORT);
  if (st0) CHECK(st == st0);
  if (st) {
    CHECK(!memcmp(h.p, img.data(), total));
    return;
  }
  ++accepted;
  CHECK(p.transport == 1 && p.off == hlen && p.len == skip + q);
  // the header, moved and fixed; everything else as it was
  std::vector<uint8_t> want = img;
  uint8_t *w = want.data() + hlen;
  memmove(w, img.data(), skip);
  if (flags & ESPGPU_IN_AF6) {
    put16(w + 4, q);
    w[6] = (uint8_t)nxt;
  } else {
    put16(w + 2, skip + q);
    w[9] = (uint8_t)nxt;
    put16(w + 10, 0);
    put16(w + 10, cksum(w, skip));
    CHECK(cksum(h.p + hlen, skip) == 0);
  }
  CHECK(!memcmp(h.p, want.data(), total));
  // out of place: the source is not written, the destination only in [hlen, hlen + skip)
  Heap src(skip), dst(total);
  memcpy(src.p, img.data(), skip);
  memset(dst.p, 0x3c, total);
  CHECK(esp_decap_rule(flags, ivlen, alen, src.p, dst.p, skip, rlen, trailer, &p) == 0);
  CHECK(!memcmp(src.p, img.data(), skip) && !memcmp(dst.p + hlen, want.data() + hlen, skip));
  for (uint32_t k = 0; k < total; ++k)
    if (k < hlen || k >= hlen + skip) CHECK(dst.p[k] == 0x3c);
}

}  // namespace

int main() {
  const uint32_t modes[3] = {0, ESPGPU_IN_TRANSPORT, ESPGPU_IN_TUNNEL};
  const uint32_t nxts[6] = {4, 41, 6, 17, 59, 50};
  for (uint32_t ivlen : {0u, 8u, 16u})
    for (uint32_t alen : {0u, 8u, 12u, 16u, 24u, 32u})
      for (uint32_t mode : modes)
        for (uint32_t nxt : nxts)
          for (uint32_t q : {0u, 19u, 20u, 39u, 40u, 41u, 100u}) {
            const uint32_t padlen = rnd() % 8;
            for (uint32_t ihl = 5; ihl <= 15; ++ihl)                 // every ip_hl x hlen
              run(mode, ihl * 4, (uint8_t)(0x40 | ihl), ivlen, alen, q, padlen, nxt, 0);
            run(mode | ESPGPU_IN_AF6, 40, 0x60 | (rnd() & 0xf), ivlen, alen, q, padlen, nxt, 0);
          }
  // refusals of every kind: the packet stays as it is
  for (uint32_t mode : modes)
    for (uint32_t af6 : {0u, (uint32_t)ESPGPU_IN_AF6}) {
      const uint32_t f = mode | af6, skip = af6 ? 40 : 24;
      const uint8_t first = af6 ? 0x60 : 0x46;
      for (uint32_t tr : {(uint32_t)ESPGPU_TR_BADLEN, (uint32_t)ESPGPU_TR_BADPAD, (uint32_t)ESPGPU_TR_NONE})
        for (uint32_t nxt : {4u, 6u}) {
          run(f, skip, first, 8, 16, 60, 3, nxt, tr);
          run(f | ESPGPU_IN_PAD_RAND, skip, first, 8, 16, 60, 3, nxt, tr);
        }
      run(f, skip, first ^ 0x30, 8, 16, 60, 3, 6, 0);                // version
      run(f, skip, first ^ 0x01, 8, 16, 60, 3, 6, 0);                // ip_hl (IPv6: flow bits, accepted)
      for (uint32_t bad : {16u, 64u, 44u, 22u, 0u}) run(f, bad, first, 8, 16, 60, 3, 6, 0);
      run(f | 0x10, skip, first, 8, 16, 60, 3, 6, 0);
      run(f | ESPGPU_IN_TRANSPORT | ESPGPU_IN_TUNNEL, skip, first, 8, 16, 60, 3, 6, 0);
      run(f, skip, first, 8, 16, 0, 0, 6, 0);                        // plen 2
      run(f, skip, first, 8, 16, 1, 0, 6, 0);                        // plen 3
    }
  // a record shorter than its header, ICV and trailer: plen < 2 is decided before anything is read
  for (uint32_t rlen : {0u, 8u, 31u, 32u, 33u}) {
    Heap one(1);
    DecapPlan p;
    CHECK(esp_decap_rule(ESPGPU_IN_TRANSPORT, 8, 16, one.p, one.p, 20, rlen, ESPGPU_TR_VALID | 6, &p) == ESPGPU_EINVAL);
  }
  CHECK(accepted > 1000 && tunnels > 100);
  if (fails) return 1;
  printf("OK %ld runs, %ld accepted, %ld tunnel\n", runs, accepted, tunnels);
  return 0;
}
