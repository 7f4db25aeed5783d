// bounds_chk.h — the accessor layer of the bounds-checked build (`make
// checked`, -DESPGPU_BOUNDS, libespgpu_chk.so).  Never part of
// libespgpu.so: without ESPGPU_BOUNDS this header declares nothing.
//
// In the checked build every global-memory access that esp_gcm.hip and
// esp_ah.hip make through a record pointer (arena, out), a per-record array
// (desc, status, trailer, order), the chunk list or the SA table goes through
// chk_range / chk_index first (dev_prims.h routes ld16, st16, st8,
// st_partial, esp_ld4, esp_st4, esp_ld4w, esp_desc_ld16 and the esp_at_*
// helpers here).  An access that leaves its bounds is recorded in the report
// and NOT made: a load yields zeros, a store is dropped, a pointer into an
// array is redirected to its element 0.  esp_cbc.hip is not instrumented
// (DESIGN.md §4): its block is never set, so its accesses are made unchecked.
//
//  * byte ranges: an access of b bytes at ptr belongs to the armed buffer
//    (0 arena, 1 out) whose start is the nearest at or below ptr (so a stray
//    access that reaches the other buffer is judged by that buffer's bounds,
//    and an unarmed out is the arena); a read may end up to `pad` bytes past
//    the buffer's armed end, a write not past it.
//    An unarmed launch (lo[0] == 0) checks indices only.
//  * indices: < n for desc / status / trailer / order, < nsas for the SA
//    table, < nchunks (the planner's capacity) for the chunk list.
//
// The state is a per-file __device__ block (as g_opts / e_opts), set by the
// file's launcher once the launch's stream has drained (so launches of one
// file on different streams must not overlap); the report lives in device memory
// and is updated with vector atomics.  No LDS.  Out of scope (DESIGN.md
// §4): host-memory staging (xin / xout / hdesc / hstat, xfer.hip, the
// doorbell kernel), and the pointers that are not derived from a record: key
// schedules, tables, work queues, nchunks, ej0.
#pragma once
#ifdef ESPGPU_BOUNDS
#include <stdint.h>

namespace espgpu {

enum : uint32_t {
  CHK_READ = 0,      // byte range, load
  CHK_WRITE = 1,     // byte range, store
  CHK_DESC = 2,      // index kinds: the bound is n ...
  CHK_STATUS = 3,
  CHK_TRAILER = 4,
  CHK_ORDER = 5,
  CHK_CHUNKS = 6,    // ... the chunk capacity ...
  CHK_SAS = 7,       // ... nsas
};

constexpr uint32_t kChkKeep = 64;   // violations kept in full

struct ChkViolation {
  uint32_t site;     // file tag << 16 | __LINE__ (1 esp_gcm.hip, 3 esp_ah.hip)
  uint32_t kind;     // CHK_*
  uint32_t buf;      // byte ranges: 0 arena, 1 out
  uint32_t bytes;    // byte ranges: the access's size
  int64_t at;        // byte offset of the access from its buffer's start, or the index
  uint64_t bound;    // the buffer's armed bytes, or the index bound
  uint32_t block, lane;   // blockIdx.x, threadIdx.x
};

constexpr int64_t kChkNoMark = INT64_MIN;

struct ChkReport {
  uint32_t nviol;                // violations (all of them; the first kChkKeep are kept)
  uint32_t pad_;
  unsigned long long nchecked;   // checked accesses, per lane
  long long hw[2];               // per buffer: the largest access_end - armed end seen (reads inside the pad too)
  ChkViolation v[kChkKeep];
};

// What a launch checks against (a kernel parameter struct's `chk` field on
// the host side, the per-file __device__ block on the device).
struct ChkArm {
  uint64_t lo[2], hi[2];         // armed byte ranges [lo, hi): 0 arena, 1 out; lo[0] == 0: unarmed
  uint32_t pad;                  // bytes a read may end past hi
  uint32_t n, nsas, nchunks;     // index bounds
  ChkReport *rep;                // nullptr: nothing is checked
};

#ifdef __HIPCC__
namespace {

__device__ ChkArm g_chk;

__device__ __noinline__ void chk_note(uint32_t site, uint32_t kind, uint32_t buf, uint32_t bytes, int64_t at,
                                      uint64_t bound) {
  ChkReport *r = g_chk.rep;
  const uint32_t k = atomicAdd(&r->nviol, 1u);
  if (k < kChkKeep) {
    ChkViolation &v = r->v[k];
    v.site = site;
    v.kind = kind;
    v.buf = buf;
    v.bytes = bytes;
    v.at = at;
    v.bound = bound;
    v.block = blockIdx.x;
    v.lane = threadIdx.x;
  }
}

// true: the access may be made
__device__ __forceinline__ bool chk_range(const void *ptr, uint32_t bytes, bool write, uint32_t site) {
  ChkReport *r = g_chk.rep;
  if (!r) return true;
  atomicAdd(&r->nchecked, 1ull);
  if (!g_chk.lo[0]) return true;
  const uint64_t a = (uint64_t)(uintptr_t)ptr;
  const uint64_t l0 = g_chk.lo[0], l1 = g_chk.lo[1];
  const uint32_t b = (l1 && l1 != l0 && a >= l1 && (a < l0 || l1 > l0)) ? 1u : 0u;
  const int64_t over = (int64_t)(a + bytes) - (int64_t)g_chk.hi[b];
  if (a >= g_chk.lo[b]) {
    if (over > *(volatile long long *)&r->hw[b]) atomicMax(&r->hw[b], (long long)over);
    if (over <= (write ? 0 : (int64_t)g_chk.pad)) return true;
  }
  chk_note(site, write ? CHK_WRITE : CHK_READ, b, bytes, (int64_t)(a - g_chk.lo[b]), g_chk.hi[b] - g_chk.lo[b]);
  return false;
}

__device__ __forceinline__ bool chk_index(uint32_t kind, uint64_t i, uint32_t site) {
  if (!g_chk.rep) return true;
  atomicAdd(&g_chk.rep->nchecked, 1ull);
  const uint32_t bound = kind == CHK_SAS ? g_chk.nsas : (kind == CHK_CHUNKS ? g_chk.nchunks : g_chk.n);
  if (i < bound) return true;
  chk_note(site, kind, 0, 0, (int64_t)i, bound);
  return false;
}

}  // namespace

// The launcher's part: the block for the kernels about to be queued on st,
// written once st has drained (a synchronous copy: nothing depends on how the
// runtime stages a source on the stack).  One block per file: launches of one
// file must be serialised while the checker is read.
#define ESPGPU_CHK_SET(arm, st) \
  ((void)hipStreamSynchronize(st), (void)hipMemcpyToSymbol(HIP_SYMBOL(g_chk), &(arm), sizeof(ChkArm)))
#endif  // __HIPCC__

}  // namespace espgpu
#endif  // ESPGPU_BOUNDS
