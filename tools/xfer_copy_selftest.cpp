// Host self-test of the staging copy (f-stack_amd/csrc/xfer_copy.h): the
// header is built for the CPU (ESPGPU_HOST_SHIM: __device__, __forceinline__,
// min, uint4 and v_alignbyte_b32 supplied here) and a call by nt threads is
// emulated by running t = 0 .. nt-1 one after the other -- equivalent, since
// every thread loads before it stores and source and destination never
// overlap.  Compared with memcpy over
//   source residue 0..15 x destination residue 0..15 (mod 16),
//   len 0..160 and 4092..4100,
//   nt in {1, 2, 3, 4, 8, 16, 32, 64, 256}  (stage_in gives a record 64 down
//                                            to 2 threads, the xfer kernel 256),
//   kU in {8, 16}:
// the destination span equals the source span, 32 guard bytes on each side
// of it are untouched, the source is unchanged.
//
// The source of every case is a heap block of its own that ends with the last
// dword that holds a byte of the span and, under AddressSanitizer, is poisoned
// up to the first such dword (in whole 8-byte shadow granules: a first dword
// at 4 mod 8 leaves the dword before it readable), so that a build with
// -fsanitize=address,undefined also checks the header's claim that no load
// touches a dword that holds no byte of the span.
//
// Prints OK and the number of combinations; -v lists every failing one.
// Built and run by tests/test_host_selftests.py.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#if defined(__SANITIZE_ADDRESS__)
#include <sanitizer/asan_interface.h>
#define POISON(p, n) ASAN_POISON_MEMORY_REGION((p), (n))
#define UNPOISON(p, n) ASAN_UNPOISON_MEMORY_REGION((p), (n))
#else
#define POISON(p, n) ((void)0)
#define UNPOISON(p, n) ((void)0)
#endif

struct uint4 {
  uint32_t x, y, z, w;
};
static inline uint32_t min(uint32_t a, uint32_t b) { return a < b ? a : b; }
// v_alignbyte_b32: the 64-bit hi:lo shifted right by 8 * sh bytes, low dword
static inline uint32_t host_alignbyte(uint32_t hi, uint32_t lo, uint32_t sh) {
  return (uint32_t)(((((uint64_t)hi) << 32) | lo) >> (8 * (sh & 3)));
}
#define ESPGPU_HOST_SHIM 1
#define __device__
#define __forceinline__ inline
#define __builtin_amdgcn_alignbyte(hi, lo, sh) host_alignbyte((hi), (lo), (sh))
#include "xfer_copy.h"

namespace {

constexpr uint32_t kGuard = 32;
constexpr uint8_t kFill = 0xC3;

uint32_t g_seed = 2463534242u;
inline uint8_t rnd() {
  g_seed ^= g_seed << 13;
  g_seed ^= g_seed >> 17;
  g_seed ^= g_seed << 5;
  const uint8_t v = (uint8_t)(g_seed >> 11);
  return v == kFill ? (uint8_t)(v ^ 1) : v;      // a byte that was not copied never looks copied
}

template <int kU>
bool one(uint32_t rs, uint32_t rd, uint32_t len, uint32_t nt, std::vector<uint8_t> &want) {
  // source: the dwords [first, last) relative to a 16-aligned base hold the span [rs, rs + len)
  const uint32_t first = rs & ~3u, last = len ? (rs + len + 3) & ~3u : first;
  void *raw = nullptr;
  if (posix_memalign(&raw, 16, last > 0 ? last : 1) != 0) abort();
  uint8_t *sbase = static_cast<uint8_t *>(raw);
  for (uint32_t i = first; i < last; ++i) sbase[i] = rnd();
  want.assign(sbase + first, sbase + last);
  if (len == 0) POISON(sbase, last > 0 ? last : 1);
  else POISON(sbase, first);
  // destination: guard | span at residue rd | guard, in a 16-aligned block
  void *draw = nullptr;
  static_assert(kGuard % 16 == 0, "the span's residue is rd");
  const uint32_t doff = kGuard + rd, dsize = doff + len + kGuard;
  if (posix_memalign(&draw, 16, dsize) != 0) abort();
  uint8_t *dbase = static_cast<uint8_t *>(draw);
  memset(dbase, kFill, dsize);
  for (uint32_t t = 0; t < nt; ++t)
    espgpu::xfer_copy<kU>((uint64_t)(uintptr_t)(sbase + rs), (uint64_t)(uintptr_t)(dbase + doff), len, t, nt);
  UNPOISON(sbase, last > 0 ? last : 1);
  bool ok = len == 0 || memcmp(dbase + doff, want.data() + (rs - first), len) == 0;
  for (uint32_t i = 0; i < dsize && ok; ++i)
    if ((i < doff || i >= doff + len) && dbase[i] != kFill) ok = false;
  ok = ok && (last == first || memcmp(sbase + first, want.data(), last - first) == 0);
  free(raw);
  free(draw);
  return ok;
}

}  // namespace

int main(int argc, char **argv) {
  const bool verbose = argc > 1 && strcmp(argv[1], "-v") == 0;
  std::vector<uint32_t> lens;
  for (uint32_t l = 0; l <= 160; ++l) lens.push_back(l);
  for (uint32_t l = 4092; l <= 4100; ++l) lens.push_back(l);
  const uint32_t nts[] = {1, 2, 3, 4, 8, 16, 32, 64, 256};
  std::vector<uint8_t> want;
  long checked = 0, bad = 0;
  for (int ku = 8; ku <= 16; ku += 8)
    for (uint32_t nt : nts)
      for (uint32_t len : lens)
        for (uint32_t rs = 0; rs < 16; ++rs)
          for (uint32_t rd = 0; rd < 16; ++rd) {
            const bool ok = ku == 8 ? one<8>(rs, rd, len, nt, want) : one<16>(rs, rd, len, nt, want);
            ++checked;
            if (!ok) {
              if (verbose || bad < 8)
                printf("FAIL %s kU %d nt %u len %u src %u dst %u\n", (rs | rd) == 0 ? "aligned" : "dword", ku, nt, len,
                       rs, rd);
              ++bad;
            }
          }
  if (bad) {
    printf("FAILED %ld of %ld combinations\n", bad, checked);
    return 1;
  }
  printf("OK %ld combinations\n", checked);
  return 0;
}
