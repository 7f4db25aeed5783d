// CPU self-test of the NAT-T rules' reads and writes (f-stack_amd/csrc:
// classify.h's UDP branch, decap.h's and encap.h's header moves with the UDP
// header, natt.h's checksum fix), each packet in a heap block of exactly its
// own size (encapsulation: headroom + packet + tailroom).  Built with the host
// compiler's -fsanitize=address,undefined, so a read or a write outside the
// block ends the run.  What the rules write is checked against plain
// restatements.  Run by tests/test_natt_selftest.py.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "classify.h"
#include "decap.h"
#include "encap.h"
#include "natt.h"

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

uint32_t rnd_state = 4500;
uint32_t rnd() {
  rnd_state = rnd_state * 1664525u + 1013904223u;
  return rnd_state >> 8;
}

void put16(uint8_t *p, uint32_t v) {
  p[0] = (uint8_t)(v >> 8);
  p[1] = (uint8_t)v;
}
uint32_t get16(const uint8_t *p) { return (uint32_t)p[0] << 8 | p[1]; }

// the Internet checksum of n bytes (an odd last byte padded with zero) on top of `s`
uint32_t cksum(const uint8_t *h, uint32_t n, uint32_t s = 0) {
  for (uint32_t k = 0; k + 1 < n; k += 2) s += (uint32_t)h[k] << 8 | h[k + 1];
  if (n & 1) s += (uint32_t)h[n - 1] << 8;
  while (s >> 16) s = (s & 0xffff) + (s >> 16);
  return ~s & 0xffff;
}

struct Heap {            // an exact-size heap block
  uint8_t *p;
  explicit Heap(size_t n) : p((uint8_t *)malloc(n ? n : 1)) {}
  ~Heap() { free(p); }
};

void ip4(uint8_t *h, uint32_t ihl, uint32_t total, uint32_t proto) {
  for (uint32_t k = 0; k < ihl * 4; ++k) h[k] = (uint8_t)rnd();
  h[0] = (uint8_t)(0x40 | ihl);
  put16(h + 2, total);
  put16(h + 6, 0);
  h[9] = (uint8_t)proto;
  put16(h + 10, 0);
  put16(h + 10, cksum(h, ihl * 4));
}

long n_cls = 0, n_dcp = 0, n_enc = 0, n_sum = 0;

// ---- classification: a UDP-encapsulated packet in a block of exactly ip_len bytes ----
void classification() {
  espgpu_sad_entry sas[2];
  memset(sas, 0, sizeof(sas));
  sas[0].spi = 0x11223344;
  sas[0].sa = 3;
  sas[0].proto = 50;
  sas[0].af = 4;
  sas[0].salt = 0xabcdef01;
  sas[0].flags = ESPGPU_SAD_NATT;
  const uint8_t d0[8] = {10, 9, 8, 7, 0x04, 0x01, 0x11, 0x94};
  memcpy(sas[0].dst, d0, 8);
  sas[1] = sas[0];
  sas[1].spi = 0x55667788;
  sas[1].sa = 4;
  sas[1].flags = 0;
  memset(sas[1].dst + 4, 0, 4);
  std::vector<espgpu_sad_entry> table(8);
  CHECK(sad_build(sas, 2, table.data(), 8) == 0);
  const uint32_t flags = ESPGPU_CLS_NATT_PORT(4500);
  for (uint32_t ihl = 5; ihl <= 15; ++ihl)
    for (uint32_t plen = 0; plen <= 40; ++plen) {      // bytes behind the IP header
      const uint32_t total = ihl * 4 + plen;
      Heap h(total);
      ip4(h.p, ihl, total, 17);
      memcpy(h.p + 16, d0, 4);
      uint8_t *u = h.p + ihl * 4;
      for (uint32_t k = 0; k < plen; ++k) u[k] = (uint8_t)rnd();
      const uint8_t udp[12] = {0x04, 0x01, 0x11, 0x94, (uint8_t)(plen >> 8), (uint8_t)plen, 0, 0, 0x11, 0x22, 0x33, 0x44};
      memcpy(u, udp, plen < 12 ? plen : 12);
      espgpu_desc d;
      const int st = esp_classify_rule(table.data(), 8, h.p, total, 100, flags, &d);
      ++n_cls;
      const int want = plen < 8 ? ESPGPU_ENOTSUP : plen < 16 ? ESPGPU_ENOTSUP : (plen & 3) ? ESPGPU_EINVAL : 0;
      CHECK(st == want);
      if (st == 0) CHECK(d.off4 == 100 + ihl + 2 && d.len == plen - 8 && d.sa == 3 && d.salt == 0xabcdef01);
      if (st != 0) CHECK(d.off4 == 100 && d.len == 0 && d.sa == 0xffff);
      // the port off: the UDP header is not looked at
      CHECK(esp_classify_rule(table.data(), 8, h.p, total, 100, 0, &d) == ESPGPU_ENOTSUP);
      if (plen >= 16 && !(plen & 3)) {
        // a shorter uh_ulen: trimmed; a nonzero checksum, another source port, a plain SA: refused
        put16(u + 4, plen - 4);
        CHECK(esp_classify_rule(table.data(), 8, h.p, total, 100, flags, &d) == (plen - 4 < 16 ? ESPGPU_ENOTSUP : 0));
        put16(u + 4, plen);
        u[7] = 1;
        CHECK(esp_classify_rule(table.data(), 8, h.p, total, 100, flags, &d) == ESPGPU_ENOTSUP);
        u[7] = 0;
        u[1] ^= 1;
        CHECK(esp_classify_rule(table.data(), 8, h.p, total, 100, flags, &d) == ESPGPU_ENOENT);
        u[1] ^= 1;
        const uint8_t spi1[4] = {0x55, 0x66, 0x77, 0x88};
        memcpy(u + 8, spi1, 4);
        CHECK(esp_classify_rule(table.data(), 8, h.p, total, 100, flags, &d) == ESPGPU_ENOENT);
      }
    }
  // plain ESP for the NAT-T SA: the host's; for the plain SA: accepted
  Heap h(20 + 24);
  ip4(h.p, 5, 44, 50);
  memcpy(h.p + 16, d0, 4);
  const uint8_t spi0[4] = {0x11, 0x22, 0x33, 0x44}, spi1[4] = {0x55, 0x66, 0x77, 0x88};
  espgpu_desc d;
  memcpy(h.p + 20, spi0, 4);
  CHECK(esp_classify_rule(table.data(), 8, h.p, 44, 0, flags, &d) == ESPGPU_ENOTSUP);
  memcpy(h.p + 20, spi1, 4);
  CHECK(esp_classify_rule(table.data(), 8, h.p, 44, 0, flags, &d) == 0 && d.sa == 4);
}

// ---- decapsulation: IP header + UDP header + record, transport: the header moves by hlen + 8 ----
void decapsulation() {
  for (uint32_t ihl = 5; ihl <= 15; ++ihl)
    for (uint32_t ivlen : {0u, 8u, 16u})
      for (uint32_t nxt : {6u, 17u, 4u})
        for (uint32_t mode : {0u, (uint32_t)ESPGPU_IN_TRANSPORT, (uint32_t)ESPGPU_IN_TUNNEL}) {
          const uint32_t flags = mode | ESPGPU_IN_NATT, hl = ihl * 4, skip = hl + 8, hlen = 8 + ivlen, alen = 12;
          const uint32_t q = 24, padlen = rnd() % 6, rlen = hlen + q + padlen + 2 + alen, total = skip + rlen;
          std::vector<uint8_t> img(total);
          ip4(img.data(), ihl, total, 17);
          for (uint32_t k = hl; k < total; ++k) img[k] = (uint8_t)rnd();
          img[skip + hlen + q + padlen] = (uint8_t)padlen;
          img[skip + hlen + q + padlen + 1] = (uint8_t)nxt;
          const uint32_t trailer = nxt | padlen << 8 | ESPGPU_TR_VALID;
          DecapPlan plan;
          const int st0 = dcp_plan(flags, hlen, alen, skip, rlen, trailer, &plan);
          ++n_dcp;
          if (st0 == 0 && !plan.transport) {
            Heap one(1);
            DecapPlan p2;
            CHECK(esp_decap_rule(flags, ivlen, alen, one.p, one.p, skip, rlen, trailer, &p2) == 0);
            CHECK(p2.off == skip + hlen && p2.len == q && nxt == 4 && mode != ESPGPU_IN_TRANSPORT);
            continue;
          }
          Heap h(total);
          memcpy(h.p, img.data(), total);
          DecapPlan p;
          const int st = esp_decap_rule(flags, ivlen, alen, h.p, h.p, skip, rlen, trailer, &p);
          CHECK(st == st0);
          if (st) {
            CHECK(st == ESPGPU_EPFNOSUPPORT && mode == ESPGPU_IN_TUNNEL && !memcmp(h.p, img.data(), total));
            continue;
          }
          CHECK(p.transport == 1 && p.off == hlen + 8 && p.len == hl + q);
          std::vector<uint8_t> want = img;
          uint8_t *w = want.data() + hlen + 8;
          memmove(w, img.data(), hl);
          put16(w + 2, hl + q);
          w[9] = (uint8_t)nxt;
          put16(w + 10, 0);
          put16(w + 10, cksum(w, hl));
          CHECK(!memcmp(h.p, want.data(), total));
          // out of place: the source holds the IP header alone
          Heap src(hl), dst(total);
          memcpy(src.p, img.data(), hl);
          memset(dst.p, 0x3c, total);
          CHECK(esp_decap_rule(flags, ivlen, alen, src.p, dst.p, skip, rlen, trailer, &p) == 0);
          CHECK(!memcmp(dst.p + hlen + 8, want.data() + hlen + 8, hl));
          for (uint32_t k = 0; k < total; ++k)
            if (k < hlen + 8 || k >= hlen + 8 + hl) CHECK(dst.p[k] == 0x3c);
          // a header whose ip_hl is not skip - 8
          h.p[0] ^= 1;
          std::vector<uint8_t> keep(h.p, h.p + total);
          CHECK(esp_decap_rule(flags, ivlen, alen, h.p, h.p, skip, rlen, trailer, &p) == ESPGPU_EINVAL);
          CHECK(!memcmp(h.p, keep.data(), total));
        }
  Heap one(1);
  DecapPlan p;
  for (uint32_t skip : {20u, 24u, 72u, 30u})
    CHECK(esp_decap_rule(ESPGPU_IN_NATT, 8, 12, one.p, one.p, skip, 60, ESPGPU_TR_VALID | 6, &p) == ESPGPU_EINVAL);
  CHECK(esp_decap_rule(ESPGPU_IN_NATT | ESPGPU_IN_AF6, 8, 12, one.p, one.p, 40, 60, ESPGPU_TR_VALID | 6, &p) ==
        ESPGPU_EINVAL);
}

// ---- encapsulation: a block of exactly headroom + packet + tailroom ----
void encapsulation() {
  for (uint32_t tunnel : {0u, 1u})
    for (uint32_t ihl = 5; ihl <= 15; ++ihl)
      for (uint32_t ivlen : {0u, 8u, 16u})
        for (uint32_t plen : {0u, 1u, 37u}) {
          espgpu_encsa e;
          memset(&e, 0, sizeof(e));
          e.flags = ESPGPU_ENC_NATT | (tunnel ? ESPGPU_ENC_TUNNEL : 0);
          e.ttl = 61;
          const uint8_t src[4] = {192, 0, 2, 1}, dst[8] = {198, 51, 100, 7, 0x11, 0x94, 0x11, 0x95};
          memcpy(e.src, src, 4);
          memcpy(e.dst, dst, 8);
          const espgpu_eshape s = {ivlen, ivlen == 16 ? 16u : 4u, 12};
          const uint32_t hl = ihl * 4, len = hl + plen, hlen = 8 + ivlen, oh = tunnel ? 20 : 0;
          const uint32_t rlen = tunnel ? len : plen, padding = esp_padding(rlen, s.blks);
          const uint32_t headroom = hlen + oh + 8, tailroom = padding + s.alen;
          std::vector<uint8_t> img(headroom + len + tailroom);
          for (auto &x : img) x = (uint8_t)rnd();
          uint8_t *ip = img.data() + headroom;
          ip4(ip, ihl, len, 6);
          if (!tunnel) memcpy(ip + 16, dst, 4);
          Heap h(img.size());
          memcpy(h.p, img.data(), img.size());
          EncapOut o;
          ++n_enc;
          CHECK(esp_encap_rule(&e, s, h.p + headroom, len, headroom, tailroom, 0x7788, &o) == 0);
          const uint32_t total = (tunnel ? 20 : hl) + hlen + rlen + padding + s.alen + 8;
          CHECK(o.front == headroom && o.total == total && o.reclen == total - 8 - (tunnel ? 20 : hl));
          CHECK(o.frame == (rlen | (tunnel ? 4u : 6u) << 16));
          const uint8_t *w = h.p;                                  // the wire packet starts at the block's first byte
          const uint32_t whl = tunnel ? 20 : hl;
          CHECK(w[0] == (0x40 | whl / 4) && get16(w + 2) == total && w[9] == 17 && cksum(w, whl) == 0);
          CHECK(!memcmp(w + 12, tunnel ? src : ip + 12, 4) && !memcmp(w + 16, dst, 4));
          CHECK(get16(w + whl) == 0x1194 && get16(w + whl + 2) == 0x1195 && get16(w + whl + 4) == total - whl &&
                get16(w + whl + 6) == 0);
          // ESP header, IV, padding, trailer and ICV field are not written
          CHECK(!memcmp(w + whl + 8, img.data() + whl + 8, hlen));
          CHECK(!memcmp(h.p + headroom + len, img.data() + headroom + len, tailroom));
          if (!tunnel) CHECK(!memcmp(h.p + headroom + hl, ip + hl, plen));
          if (tunnel) CHECK(!memcmp(h.p + headroom + hl, ip + hl, plen) && get16(h.p + headroom + 2) == len);
          // one byte of headroom less: refused with nothing written (the block is one byte shorter too)
          Heap h2(img.size() - 1);
          memcpy(h2.p, img.data() + 1, img.size() - 1);
          CHECK(esp_encap_rule(&e, s, h2.p + headroom - 1, len, headroom - 1, tailroom, 0x7788, &o) == ESPGPU_ENOBUFS);
          CHECK(!memcmp(h2.p, img.data() + 1, img.size() - 1));
        }
}

// ---- the checksum fix: every segment length, the packet in a block of exactly its size ----
void one_sum(uint32_t proto, uint32_t ihl, uint32_t seglen, uint32_t policy, uint32_t delta) {
  const uint32_t hl = ihl * 4, total = hl + seglen, foff = proto == 6 ? 16 : 6;
  Heap h(total);
  ip4(h.p, ihl, total, proto);
  for (uint32_t k = hl; k < total; ++k) h.p[k] = (uint8_t)rnd();
  if (proto == 17 && seglen >= 6) put16(h.p + hl + 4, seglen);
  std::vector<uint8_t> img(h.p, h.p + total);
  const uint32_t cf = natt_cksum_rule(h.p, total, proto, policy, delta);
  ++n_sum;
  std::vector<uint8_t> want = img;
  uint32_t wcf = 0;
  if (seglen >= foff + 2) {
    uint8_t *f = want.data() + hl + foff;
    const uint32_t old = (uint32_t)f[0] | (uint32_t)f[1] << 8;            // as a little-endian host loads it
    if (policy == 0) {
      if (delta) {
        if (!(proto == 17 && old == 0)) {
          uint32_t v = old + delta;
          if (v > 65535) v -= 65535;
          f[0] = (uint8_t)v;
          f[1] = (uint8_t)(v >> 8);
        }
      } else if (proto == 17) {
        f[0] = f[1] = 0;
      } else {
        wcf = ESPGPU_NATT_CSUM_VALID;
      }
    } else {
      f[0] = f[1] = 0;
      uint8_t ph[12];
      memcpy(ph, img.data() + 12, 8);
      ph[8] = 0;
      ph[9] = (uint8_t)proto;
      put16(ph + 10, seglen);
      uint32_t s = 0;
      for (uint32_t k = 0; k < 12; k += 2) s += get16(ph + k);
      uint32_t c = cksum(want.data() + hl, seglen, s);
      if (proto == 17 && c == 0) c = 0xffff;
      put16(f, c);
    }
  }
  CHECK(cf == wcf);
  CHECK(!memcmp(h.p, want.data(), total));
}

void checksums() {
  for (uint32_t seglen = 0; seglen <= 530; ++seglen)
    for (uint32_t proto : {6u, 17u}) {
      const uint32_t ihl = 5 + rnd() % 11;
      one_sum(proto, ihl, seglen, 1, 0);
      one_sum(proto, ihl, seglen, 0, 1 + rnd() % 65535);
      one_sum(proto, ihl, seglen, 0, 0);
    }
  for (uint32_t proto : {6u, 17u}) one_sum(proto, 5, 65515, 1, 0);
  // other protocols, versions and header lengths: nothing is touched (a one-byte block where nothing is read)
  Heap one(1);
  one.p[0] = 0x45;
  CHECK(natt_cksum_rule(one.p, 1, 50, 1, 0) == 0 && natt_cksum_rule(one.p, 1, 4, 0, 5) == 0);
  CHECK(natt_cksum_rule(one.p, 1, 6, 1, 0) == 0 && one.p[0] == 0x45);
  Heap h(40);
  ip4(h.p, 5, 40, 6);
  h.p[0] = 0x65;
  std::vector<uint8_t> keep(h.p, h.p + 40);
  CHECK(natt_cksum_rule(h.p, 40, 6, 1, 0) == 0 && !memcmp(h.p, keep.data(), 40));
  h.p[0] = 0x4b;                                                       // ip_hl * 4 = 44 > len
  keep[0] = 0x4b;
  CHECK(natt_cksum_rule(h.p, 40, 6, 1, 0) == 0 && !memcmp(h.p, keep.data(), 40));
}

}  // namespace

int main() {
  classification();
  decapsulation();
  encapsulation();
  checksums();
  CHECK(n_cls > 400 && n_dcp > 250 && n_enc > 150 && n_sum > 3000);
  if (fails) return 1;
  printf("OK %ld classified, %ld decapsulated, %ld encapsulated, %ld checksums\n", n_cls, n_dcp, n_enc, n_sum);
  return 0;
}
