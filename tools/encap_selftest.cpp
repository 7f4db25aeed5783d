// CPU self-test of the outbound encapsulation rule's reads and writes
// (f-stack_amd/csrc/encap.h: esp_encap_rule, the function behind
// espgpu_esp_encap and enc_kernel): cleartext packets of every kind the rule
// tells apart -- SA family x packet family x mode x proxy, every ip_hl x hlen,
// every refusal -- each in a heap block of exactly headroom + len + tailroom
// bytes, with the rooms exactly what the packet needs.  Built with the host
// compiler's -fsanitize=address,undefined, so a read or a write outside the
// block ends the run.  What the rule writes is checked against a plain
// restatement: the moved or the new header with its fields set, the inner
// header's length and checksum in a tunnel, nothing else changed.
// Run by tests/test_encap_selftest.py.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "encap.h"

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

uint32_t rnd_state = 97531;
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

long runs = 0, accepted = 0, tunnels = 0, refused = 0;

espgpu_encsa make_sa(uint32_t flags) {
  espgpu_encsa e;
  memset(&e, 0, sizeof(e));
  e.flags = flags;
  e.ttl = (uint8_t)(1 + rnd() % 255);
  const uint32_t alen = flags & ESPGPU_ENC_AF6 ? 16 : 4;
  for (uint32_t k = 0; k < alen; ++k) {
    e.src[k] = (uint8_t)(1 + rnd() % 200);
    e.dst[k] = (uint8_t)(1 + rnd() % 200);
  }
  return e;
}

// A cleartext packet: version 4 with ihl dwords of header, or version 6.
std::vector<uint8_t> make_pkt(bool v6, uint32_t ihl, uint32_t plen, const uint8_t *dst) {
  const uint32_t skip = v6 ? 40 : ihl * 4;
  std::vector<uint8_t> p(skip + plen);
  for (auto &x : p) x = (uint8_t)rnd();
  p[0] = v6 ? (uint8_t)(0x60 | (rnd() & 0xf)) : (uint8_t)(0x40 | ihl);
  if (dst) memcpy(p.data() + (v6 ? 24 : 16), dst, v6 ? 16 : 4);
  return p;
}

// One packet with exactly the rooms it needs (`cut_head` / `cut_tail` bytes
// less, to be refused), in one exact-size block.
void run(const espgpu_encsa &e, const espgpu_eshape &s, const std::vector<uint8_t> &pkt, uint32_t cut_head,
         uint32_t cut_tail, int want) {
  const uint32_t len = (uint32_t)pkt.size(), hlen = 8 + s.ivlen;
  const bool af6 = e.flags & ESPGPU_ENC_AF6, v6 = len && (pkt[0] >> 4) == 6;
  const uint32_t skip = v6 ? 40 : len ? (pkt[0] & 0xfu) * 4 : 0;
  // the decision, restated
  bool tunnel = (e.flags & ESPGPU_ENC_TUNNEL) || af6 != v6;
  bool dst0 = true;
  for (uint32_t k = 0; k < (af6 ? 16u : 4u); ++k) dst0 = dst0 && e.dst[k] == 0;
  if (!tunnel && !dst0 && len >= skip) tunnel = memcmp(pkt.data() + (v6 ? 24 : 16), e.dst, v6 ? 16 : 4) != 0;
  const uint32_t oh = tunnel ? (af6 ? 40 : 20) : 0, rlen = tunnel ? len : len - skip;
  const uint32_t padding = esp_padding(rlen, s.blks);
  const uint32_t head = hlen + oh - cut_head, tail = padding + s.alen - cut_tail;
  Heap h((size_t)head + len + tail);
  std::vector<uint8_t> img((size_t)head + len + tail);
  for (auto &x : img) x = (uint8_t)rnd();
  if (len) memcpy(img.data() + head, pkt.data(), len);
  memcpy(h.p, img.data(), img.size());
  EncapOut o;
  memset(&o, 0xee, sizeof(o));
  const uint32_t ip_id = rnd() & 0xffff;
  const int st = esp_encap_rule(&e, s, h.p + head, len, head, tail, ip_id, &o);
  ++runs;
  CHECK(st == want);
  if (st) {
    ++refused;
    CHECK(!memcmp(h.p, img.data(), img.size()));
    return;
  }
  ++accepted;
  tunnels += tunnel;
  const uint32_t total = (tunnel ? oh : skip) + hlen + rlen + padding + s.alen;
  CHECK(o.front == hlen + oh && o.front == head && o.total == total && o.total == img.size());
  CHECK(o.reclen == total - (tunnel ? oh : skip) && (o.frame & 0xffff) == rlen);
  std::vector<uint8_t> w = img;
  uint8_t *ip = w.data();                              // the wire packet starts the block
  if (tunnel) {
    uint8_t *in = w.data() + head;
    uint32_t itos;
    bool idf = false;
    if (v6) {
      put16(in + 4, len - 40);
      itos = (uint32_t)(in[0] & 0xf) << 4 | in[1] >> 4;
    } else {
      put16(in + 2, len);
      put16(in + 10, 0);
      put16(in + 10, cksum(in, skip));
      itos = in[1];
      idf = in[6] & 0x40;
    }
    CHECK(o.frame >> 16 == (v6 ? 41u : 4u));
    uint32_t otos = itos;
    if (e.flags & ESPGPU_ENC_ECN_ALLOWED) {
      if ((itos & 3) == 3) otos &= ~1u;
    } else if (!(e.flags & ESPGPU_ENC_ECN_NOCARE)) {
      otos &= ~3u;
    }
    if (af6) {
      ip[0] = (uint8_t)(0x60 | otos >> 4);
      ip[1] = (uint8_t)(otos << 4);
      ip[2] = ip[3] = 0;
      put16(ip + 4, total - 40);
      ip[6] = 50;
      ip[7] = e.ttl;
      memcpy(ip + 8, e.src, 16);
      memcpy(ip + 24, e.dst, 16);
    } else {
      const bool setdf = v6 ? (e.flags & kEncDf) != 0
                            : (e.flags & ESPGPU_ENC_DF_SET) || ((e.flags & ESPGPU_ENC_DF_COPY) && idf);
      ip[0] = 0x45;
      ip[1] = (uint8_t)otos;
      put16(ip + 2, total);
      put16(ip + 4, (e.flags & ESPGPU_ENC_RFC6864) && setdf ? 0 : ip_id);
      put16(ip + 6, setdf ? 0x4000 : 0);
      ip[8] = e.ttl;
      ip[9] = 50;
      put16(ip + 10, 0);
      memcpy(ip + 12, e.src, 4);
      memcpy(ip + 16, e.dst, 4);
      put16(ip + 10, cksum(ip, 20));
      CHECK(cksum(h.p, 20) == 0);
    }
  } else {
    memmove(ip, img.data() + head, skip);
    if (v6) {
      CHECK(o.frame >> 16 == ip[6]);
      put16(ip + 4, total - 40);
      ip[6] = 50;
    } else {
      CHECK(o.frame >> 16 == ip[9]);
      put16(ip + 2, total);
      ip[9] = 50;
      put16(ip + 10, 0);
      put16(ip + 10, cksum(ip, skip));
      CHECK(cksum(h.p, skip) == 0);
    }
  }
  CHECK(!memcmp(h.p, w.data(), w.size()));
}

}  // namespace

int main() {
  const espgpu_eshape shapes[] = {{0, 4, 0}, {0, 4, 12}, {8, 4, 16}, {8, 16, 16}, {8, 4, 8}, {16, 16, 12},
                                  {16, 16, 32}, {16, 16, 0}, {8, 4, 24}};
  const uint32_t policies[] = {0, ESPGPU_ENC_DF_SET, ESPGPU_ENC_DF_COPY, ESPGPU_ENC_ECN_ALLOWED,
                               ESPGPU_ENC_ECN_NOCARE | ESPGPU_ENC_DF_COPY | ESPGPU_ENC_RFC6864,
                               ESPGPU_ENC_DF_SET | ESPGPU_ENC_RFC6864};
  for (const espgpu_eshape &s : shapes)
    for (uint32_t saf6 : {0u, (uint32_t)ESPGPU_ENC_AF6})
      for (uint32_t mode : {0u, (uint32_t)ESPGPU_ENC_TUNNEL})
        for (int v6 = 0; v6 < 2; ++v6)
          for (int proxy = 0; proxy < 3; ++proxy) {            // SA dst: the packet's, another, unspecified
            const uint32_t pol = policies[rnd() % 6];
            for (uint32_t ihl = 5; ihl <= (v6 ? 5u : 15u); ++ihl)
              for (uint32_t plen : {0u, 1u, 2u, 3u, 17u, 64u}) {
                espgpu_encsa e = make_sa(saf6 | mode | pol);
                if (proxy == 2) memset(e.dst, 0, 16);
                const bool same_af = (saf6 != 0) == (v6 != 0);
                const std::vector<uint8_t> p = make_pkt(v6, ihl, plen, proxy == 0 && same_af ? e.dst : nullptr);
                int want = 0;
                if (proxy == 2 && (saf6 || mode || !same_af)) want = ESPGPU_EINVAL;
                run(e, s, p, 0, 0, want);
              }
          }
  // refusals of every kind: the block stays as it is
  const espgpu_eshape s = {8, 4, 16};
  for (uint32_t saf6 : {0u, (uint32_t)ESPGPU_ENC_AF6})
    for (int v6 = 0; v6 < 2; ++v6) {
      const std::vector<uint8_t> p = make_pkt(v6, 7, 50, nullptr);
      espgpu_encsa e = make_sa(saf6 | ESPGPU_ENC_TUNNEL);
      run(e, s, p, 1, 0, ESPGPU_ENOBUFS);
      run(e, s, p, 0, 1, ESPGPU_ENOBUFS);
      for (uint32_t bad : {0x80u, (uint32_t)kEncDf, (uint32_t)kEncEcn, 0x80000000u}) {
        espgpu_encsa b = e;
        b.flags |= bad;
        run(b, s, p, 0, 0, ESPGPU_EINVAL);
      }
      for (uint32_t ver : {0u, 5u, 7u}) {
        std::vector<uint8_t> q = p;
        q[0] = (uint8_t)(ver << 4 | 5);
        run(e, s, q, 0, 0, ESPGPU_EAFNOSUPPORT);
      }
      for (uint32_t n : {0u, 1u, 19u}) run(e, s, std::vector<uint8_t>(p.begin(), p.begin() + n), 0, 0, ESPGPU_EINVAL);
      if (v6) run(e, s, std::vector<uint8_t>(p.begin(), p.begin() + 39), 0, 0, ESPGPU_EINVAL);
      if (!v6) {
        run(e, s, std::vector<uint8_t>(p.begin(), p.begin() + 27), 0, 0, ESPGPU_EINVAL);   // ip_hl * 4 > len
        std::vector<uint8_t> q = p;
        q[0] = 0x44;
        run(e, s, q, 0, 0, ESPGPU_EINVAL);
      }
      if (saf6) {
        espgpu_encsa b = e;
        b.src[0] = 0xfe;
        b.src[1] = 0x9a;
        run(b, s, p, 0, 0, ESPGPU_ENOTSUP);
        b = e;
        memset(b.src, 0, 16);
        run(b, s, p, 0, 0, ESPGPU_EINVAL);
      }
      // total at the limit: 65532 is the last this shape reaches, then EMSGSIZE
      const uint32_t oh = saf6 ? 40 : 20, skip = v6 ? 40 : 28;
      const uint32_t room = 65535 - oh - 8 - s.ivlen - s.alen, rl = room / 4 * 4 - 2;   // rlen + padding, padding 2
      run(e, s, make_pkt(v6, 7, rl - skip, nullptr), 0, 0, 0);
      run(e, s, make_pkt(v6, 7, rl - skip + 1, nullptr), 0, 0, ESPGPU_EMSGSIZE);
      run(e, s, make_pkt(v6, 7, 65536 - skip, nullptr), 0, 0, ESPGPU_EMSGSIZE);
    }
  CHECK(accepted > 5000 && tunnels > 2000 && accepted - tunnels > 500 && refused > 500);
  if (fails) return 1;
  printf("OK %ld runs, %ld accepted, %ld tunnel, %ld refused\n", runs, accepted, tunnels, refused);
  return 0;
}
