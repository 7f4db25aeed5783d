// replay.hip — the ESP replay window for a device-resident batch: the
// pre-filter before crypto and the window update after it.  The predicates
// both share with the host rules are replay.h's; the grouping by SA that the
// update is built on is sa_group.hip's.
//
// The inbound sequence on a batch (include/espgpu.h, replay block):
//   1. espgpu_replay_check_batch  esp_input's ipsec_chkreplay (xform_esp.c:
//      329-340, ipsec.c:1248-1331) for every record in parallel, against the
//      windows as they stand when the batch starts; it supplies the ESN high
//      word for the AAD (:339, :372-402).  A replayed record gets status
//      ESPGPU_EACCES and descriptor len 0 (the decrypt kernels then drop it
//      as EINVAL without crypto work).
//   2. espgpu_decrypt_batch       ICV check, decrypt, trailer checks.
//   3. espgpu_replay_update_batch esp_input_cb's ipsec_updatereplay
//      (xform_esp.c:565-580, ipsec.c:1338-1436) for the records that
//      authenticated, with the result of applying espgpu_replay_update64 to
//      each SA's records one after another in arrival (index) order.  The
//      windows stay in HBM for the next batch's pre-filter.
//   4. espgpu_replay_merge        folds the EACCES of 1 and 3 into the status.
//
// The check is one lane per record: a 16-byte descriptor, the 4-byte sequence
// number from the record header and one bitmap word; integer compares only.
// An AH SA's window (ESPGPU_REPLAY_AH) has its number at desc.salt - 4 of the
// record, which is the whole packet (replay_seq_at).
//
// The update is sequential by definition; three facts make it parallel
// (DESIGN.md 3.4 has the arguments):
//   * the window top a record sees is max(T0, seq64 of the SA's earlier
//     taking-part records): an exclusive max-scan per SA in arrival order;
//   * inside the window the first record with a given seq64 wins, if its ring
//     bit in the initial bitmap is clear or its word lies above the initial
//     top's word (the advances have zeroed it by then);
//   * the final window is last = the SA's maximum, the ring words between the
//     initial and the final top zeroed, then the bit of every accepted record
//     that is less than a ring below the final top.
// So: a stable LSD radix sort of the records by SA (sa_group.hip: 8-bit digits,
// as many passes as the SA count needs), a segmented max-scan over the grouped
// positions (three kernels, kReplayScanBlock positions per workgroup), a hash
// table holding the first grouped position per (SA, seq64), the decisions
// (which read the initial bitmap), then clear and set as two more launches.
// Every step is a grid over records or over SAs, whatever the SA mix.
#include <hip/hip_runtime.h>

#include "dev_prims.h"
#include "espgpu_internal.h"
#include "replay.h"
#include "sa_group.h"

namespace espgpu {

namespace {

// ipsec_chkreplay (ipsec.c:1248-1331): true = permitted, *seqhigh set.
__device__ bool chkreplay(const espgpu_replay &r, const uint32_t *bitmap, uint32_t seq, uint32_t *seqhigh) {
  if (seq == 0 && r.last == 0) return false;
  const uint32_t window = r.wsize << 3;
  const uint32_t tl = (uint32_t)r.last, th = (uint32_t)(r.last >> 32);
  const uint32_t bl = tl - window + 1;
  // the high part stays when seq is in [bl, 2^32) with the window in one
  // subspace, or in [0, bl) with the window spanning two
  if ((tl >= window - 1 && seq >= bl) || (tl < window - 1 && seq < bl)) {
    *seqhigh = th;
    return !(seq <= tl && replay_seen(r, bitmap, seq));
  }
  // top of a non-ESN space reached: only SADB_X_EXT_CYCSEQ SAs go on
  if (tl == 0xffffffffu && !(r.flags & ESPGPU_REPLAY_ESN) && !(r.flags & ESPGPU_REPLAY_CYCSEQ))
    return false;
  if (tl < window - 1 && seq >= bl) {         // in the window, previous subspace
    if (th == 0) return false;
    *seqhigh = th - 1;
    return !replay_seen(r, bitmap, seq);
  }
  *seqhigh = th + 1;                           // wrapped into the next subspace
  return !(th + 1 == 0 && !(r.flags & ESPGPU_REPLAY_CYCSEQ));
}

// Where a record's sequence number lies and whether the record is long enough
// to hold it: byte 4 of an ESP record; of an AH record (a window with
// ESPGPU_REPLAY_AH; the record is the whole packet and salt the ICV field's
// offset) the dword before the ICV field, newah.ah_seq.
__device__ __forceinline__ bool replay_seq_at(const espgpu_replay &r, const espgpu_desc &d, uint32_t *at) {
  if (r.flags & ESPGPU_REPLAY_AH) {
    *at = d.salt - 4;
    return d.salt >= 12 && d.salt <= d.len;
  }
  *at = 4;
  return d.len >= 8;
}

__global__ __launch_bounds__(256) void replay_check_kernel(const uint8_t *arena, espgpu_desc *desc, uint32_t n,
                                                           const espgpu_replay *rp, uint32_t nrp,
                                                           const uint32_t *bitmap, uint8_t *rstatus) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const espgpu_desc d = desc[i];
  uint8_t st = 0;
  if (d.sa < nrp && d.len != 0) {
    const espgpu_replay r = rp[d.sa];
    uint32_t at;
    if (replay_seq_at(r, d, &at) && r.wsize != 0) {   // esp_input: replay != NULL && wsize != 0
      const uint32_t seq = bswap32(*reinterpret_cast<const uint32_t *>(arena + (size_t)d.off4 * 4 + at));
      uint32_t seqh = 0;
      if (!chkreplay(r, bitmap, seq, &seqh)) {
        st = ESPGPU_EACCES;
        desc[i].len = 0;
      } else if (r.flags & ESPGPU_REPLAY_ESN) {
        desc[i].esn_hi = seqh;
      }
    }
  }
  rstatus[i] = st;
}

__global__ __launch_bounds__(256) void replay_merge_kernel(uint8_t *status, const uint8_t *rstatus, uint32_t n) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n && rstatus[i]) status[i] = rstatus[i];
}

// ---- window update ------------------------------------------------------------

constexpr uint32_t kScanItems = kReplayScanBlock / 256;
constexpr uint32_t kEmpty = 0xffffffffu;           // free hash slot (no grouped position is 2^32 - 1)

// The workspace of one call, carved from the ctx's buffer (upd_carve).
struct UpdWs {
  uint64_t *sseq;          // [n] seq64 by grouped position (0 for records that take no part)
  uint64_t *top;           // [n] the window top each grouped position sees (M_i)
  uint64_t *agg_v, *car_v; // [scan blocks] segmented-scan aggregates and carries
  uint64_t *sa_top;        // [nsa] final top per SA (0: no record took part)
  GroupWs g;
  uint32_t *hash;          // [hcap] first grouped position per (SA, seq64)
  uint32_t *agg_f, *car_f; // [scan blocks] segment-head flags of the aggregates / carries
  uint64_t hcap;
  uint32_t scan_blocks;
};

struct UpdArgs {
  const uint8_t *arena;
  const espgpu_desc *desc;
  const uint8_t *status;
  espgpu_replay *rp;
  uint32_t *bitmap;
  uint8_t *ustatus;
  const uint32_t *skey, *order;   // the sorted buffers
  uint32_t n, nrp, nsa;           // nsa = group_no_key(nrp)
  UpdWs w;
};

__host__ __device__ inline uint64_t hash_cap(uint32_t n) {
  uint64_t c = 1024;
  while (c < 2 * (uint64_t)n) c <<= 1;
  return c;
}

// Which records take part, and under which SA.
__global__ __launch_bounds__(256) void upd_prep_kernel(UpdArgs a) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n) return;
  const espgpu_desc d = a.desc[i];
  uint32_t k = a.nsa;
  uint8_t u = 0;
  if (a.status[i] == 0 && d.sa < a.nrp && d.len != 0) {
    const espgpu_replay r = a.rp[d.sa];
    uint32_t at;
    if (replay_seq_at(r, d, &at) && r.wsize != 0) {
      if (replay_usable64(r)) k = d.sa;
      else u = ESPGPU_EINVAL;
    }
  }
  a.w.g.key[0][i] = k;
  a.w.g.idx[0][i] = i;
  a.ustatus[i] = u;
}

// Segmented max: f = a segment head lies in the range, v = the maximum since
// the last head (or over the whole range).  {0, 0} is the identity.
struct SegMax {
  uint32_t f;
  uint64_t v;
};
__device__ __forceinline__ SegMax seg_comb(SegMax a, SegMax b) {
  return SegMax{a.f | b.f, b.f ? b.v : (a.v > b.v ? a.v : b.v)};
}
__device__ __forceinline__ SegMax seg_shfl_up(SegMax x, uint32_t d) {
  SegMax y;
  y.f = __shfl_up(x.f, d);
  const uint32_t lo = __shfl_up((uint32_t)x.v, d), hi = __shfl_up((uint32_t)(x.v >> 32), d);
  y.v = ((uint64_t)hi << 32) | lo;
  return y;
}
// Exclusive scan of one SegMax per thread over a 256-thread workgroup.
__device__ SegMax block_excl(SegMax x, SegMax *total, SegMax *wt) {
  const uint32_t lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  SegMax inc = x;
  for (uint32_t d = 1; d < 64; d <<= 1) {
    const SegMax y = seg_shfl_up(inc, d);
    if (lane >= d) inc = seg_comb(y, inc);
  }
  SegMax ex = seg_shfl_up(inc, 1);
  if (lane == 0) ex = SegMax{0, 0};
  __syncthreads();                       // wt may still be read from the last use
  if (lane == 63) wt[wv] = inc;
  __syncthreads();
  SegMax pre{0, 0}, tot{0, 0};
  for (uint32_t k = 0; k < 4; ++k) {
    if (k < wv) pre = seg_comb(pre, wt[k]);
    tot = seg_comb(tot, wt[k]);
  }
  *total = tot;
  return seg_comb(pre, ex);
}

__device__ __forceinline__ uint64_t hash_slot(uint32_t key, uint64_t s, uint64_t mask) {
  uint64_t x = s * 0x9E3779B97F4A7C15ull + key;
  x ^= x >> 32;
  x *= 0xD6E8FEB86659FD93ull;
  x ^= x >> 29;
  return x & mask;
}

// The slot of (key, s) ends up holding the lowest grouped position inserted
// under it.  A slot's value only ever changes between positions of one
// (key, s), so comparing through the position it holds is stable.
__device__ void hash_insert(const UpdArgs &a, uint32_t key, uint64_t s, uint32_t p) {
  const uint64_t mask = a.w.hcap - 1;
  for (uint64_t h = hash_slot(key, s, mask);; h = (h + 1) & mask) {
    const uint32_t old = atomicCAS(&a.w.hash[h], kEmpty, p);
    if (old == kEmpty) return;
    if (a.skey[old] == key && a.w.sseq[old] == s) {
      atomicMin(&a.w.hash[h], p);
      return;
    }
  }
}
__device__ bool hash_first(const UpdArgs &a, uint32_t key, uint64_t s, uint32_t p) {
  const uint64_t mask = a.w.hcap - 1;
  for (uint64_t h = hash_slot(key, s, mask);; h = (h + 1) & mask) {
    const uint32_t cur = a.w.hash[h];
    if (cur == kEmpty) return true;      // (every record looked up was inserted)
    if (a.skey[cur] == key && a.w.sseq[cur] == s) return cur == p;
  }
}

// The per-SA exclusive max-scan over the grouped positions, in three kernels.
// FINAL = false: gather seq64 into sseq and write the workgroup's aggregate.
// FINAL = true: with the carries, write the top each position sees, enter the
// position in the hash table, and at an SA's last position its final top.
template <bool FINAL>
__global__ __launch_bounds__(256) void upd_scan_kernel(UpdArgs a) {
  __shared__ SegMax wt[4];
  const uint32_t tid = threadIdx.x, n = a.n;
  const uint64_t p0 = (uint64_t)blockIdx.x * kReplayScanBlock + (uint64_t)tid * kScanItems;
  uint32_t key[kScanItems], f[kScanItems];
  uint64_t s[kScanItems];
  uint32_t prev = (p0 > 0 && p0 - 1 < n) ? a.skey[p0 - 1] : 0xffffffffu;   // position 0 is a head
  SegMax agg{0, 0};
  for (uint32_t j = 0; j < kScanItems; ++j) {
    const uint64_t p = p0 + j;
    key[j] = a.nsa;
    f[j] = 0;
    s[j] = 0;
    if (p < n) {
      key[j] = a.skey[p];
      if (FINAL) {
        s[j] = a.w.sseq[p];
      } else {
        if (key[j] < a.nsa) {
          const espgpu_desc d = a.desc[a.order[p]];
          const uint32_t rflags = a.rp[key[j]].flags;
          const uint32_t at = (rflags & ESPGPU_REPLAY_AH) ? d.salt - 4 : 4u;
          const uint32_t seq = bswap32(*reinterpret_cast<const uint32_t *>(a.arena + (size_t)d.off4 * 4 + at));
          s[j] = (rflags & ESPGPU_REPLAY_ESN) ? ((uint64_t)d.esn_hi << 32) | seq : seq;
        }
        a.w.sseq[p] = s[j];
      }
      f[j] = key[j] != prev;
      prev = key[j];
    }
    agg = seg_comb(agg, SegMax{f[j], s[j]});
  }
  SegMax total;
  const SegMax ex = block_excl(agg, &total, wt);
  if (!FINAL) {
    if (tid == 0) {
      a.w.agg_f[blockIdx.x] = total.f;
      a.w.agg_v[blockIdx.x] = total.v;
    }
    return;
  }
  uint64_t run = seg_comb(SegMax{a.w.car_f[blockIdx.x], a.w.car_v[blockIdx.x]}, ex).v;
  for (uint32_t j = 0; j < kScanItems; ++j) {
    const uint64_t p = p0 + j;
    if (p >= n) break;
    if (f[j]) run = 0;
    if (key[j] < a.nsa) {
      const uint64_t t0 = a.rp[key[j]].last;
      const uint64_t m = run > t0 ? run : t0;
      a.w.top[p] = m;
      if (!(s[j] == 0 && m == 0)) hash_insert(a, key[j], s[j], (uint32_t)p);   // (that one is refused unmarked)
      const uint32_t next = p + 1 >= n ? 0xffffffffu : (j + 1 < kScanItems ? key[j + 1] : a.skey[p + 1]);
      if (next != key[j]) a.w.sa_top[key[j]] = s[j] > m ? s[j] : m;
    }
    if (s[j] > run) run = s[j];
  }
}

// The carries: an exclusive scan of the workgroup aggregates by one workgroup.
__global__ __launch_bounds__(256) void upd_scan_carry_kernel(UpdWs w) {
  __shared__ SegMax wt[4];
  SegMax carry{0, 0};
  for (uint32_t base = 0; base < w.scan_blocks; base += 256) {
    const uint32_t e = base + threadIdx.x;
    const SegMax x = e < w.scan_blocks ? SegMax{w.agg_f[e], w.agg_v[e]} : SegMax{0, 0};
    SegMax total;
    const SegMax pre = seg_comb(carry, block_excl(x, &total, wt));
    if (e < w.scan_blocks) {
      w.car_f[e] = pre.f;
      w.car_v[e] = pre.v;
    }
    carry = seg_comb(carry, total);
  }
}

// espgpu_replay_update64's verdict for every taking-part record, from the top
// it sees, the first-occurrence table and the bitmap as the batch found it.
__global__ __launch_bounds__(256) void upd_decide_kernel(UpdArgs a) {
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= a.n) return;
  const uint32_t key = a.skey[p];
  if (key >= a.nsa) return;
  const espgpu_replay r = a.rp[key];
  const uint64_t s = a.w.sseq[p], m = a.w.top[p], window = (uint64_t)r.wsize << 3;
  bool ok;
  if (s == 0 && m == 0) {
    ok = false;
  } else if (s > m) {
    ok = true;
  } else if (m - s < window) {
    const uint32_t word = a.bitmap[replay_word(r, s)];
    const bool stale = (s >> 5) > (r.last >> 5);      // zeroed by an advance before this record
    ok = (stale || !((word >> (s & 31)) & 1u)) && hash_first(a, key, s, p);
  } else {
    ok = false;
  }
  a.ustatus[a.order[p]] = ok ? 0 : ESPGPU_EACCES;
}

// One wave per SA: zero the ring words between the old and the new top, then
// move the top.
__global__ __launch_bounds__(256) void upd_clear_kernel(UpdArgs a) {
  const uint32_t sa = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (sa >= a.nsa) return;
  const uint64_t top = a.w.sa_top[sa];
  const espgpu_replay r = a.rp[sa];
  if (top <= r.last) return;
  const uint64_t cur = r.last >> 5, mask = r.bitmap_size - 1;
  uint64_t diff = (top >> 5) - cur;
  if (diff > r.bitmap_size) diff = r.bitmap_size;
  for (uint64_t k = lane; k < diff; k += 64) a.bitmap[r.bitmap_off + (uint32_t)((cur + 1 + k) & mask)] = 0;
  if (lane == 0) a.rp[sa].last = top;
}

// The bit of every accepted record that a later lap of the ring has not
// passed over.
__global__ __launch_bounds__(256) void upd_set_kernel(UpdArgs a) {
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= a.n) return;
  const uint32_t key = a.skey[p];
  if (key >= a.nsa || a.ustatus[a.order[p]] != 0) return;
  const espgpu_replay r = a.rp[key];
  const uint64_t s = a.w.sseq[p];
  if ((s >> 5) + r.bitmap_size > (a.w.sa_top[key] >> 5))
    atomicOr(&a.bitmap[replay_word(r, s)], 1u << (s & 31));
}

size_t upd_carve(uint8_t *base, uint32_t n, uint32_t nrp, UpdWs *w) {
  WsCarver c{base};
  w->hcap = hash_cap(n);
  w->scan_blocks = (uint32_t)(((uint64_t)n + kReplayScanBlock - 1) / kReplayScanBlock);
  w->sseq = c.take<uint64_t>(n);
  w->top = c.take<uint64_t>(n);
  w->agg_v = c.take<uint64_t>(w->scan_blocks);
  w->car_v = c.take<uint64_t>(w->scan_blocks);
  w->sa_top = c.take<uint64_t>(group_no_key(nrp));
  group_carve(c, n, &w->g);
  w->hash = c.take<uint32_t>(w->hcap);
  w->agg_f = c.take<uint32_t>(w->scan_blocks);
  w->car_f = c.take<uint32_t>(w->scan_blocks);
  return c.off;
}

}  // namespace

size_t replay_update_workspace_bytes(uint32_t n, uint32_t nrp) {
  UpdWs w;
  return upd_carve(nullptr, n, nrp, &w);
}

int launch_replay_update(const uint8_t *arena, const espgpu_desc *desc, uint32_t n, const uint8_t *status,
                         espgpu_replay *rp, uint32_t nrp, uint32_t *bitmap, uint8_t *ustatus, void *ws,
                         void *stream) {
  if (n == 0) return 0;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const dim3 blk(256), grid_n((n + 255) / 256);
  if (nrp == 0) return hipMemsetAsync(ustatus, 0, n, st) == hipSuccess ? 0 : -1;
  UpdArgs a{};
  a.arena = arena;
  a.desc = desc;
  a.status = status;
  a.rp = rp;
  a.bitmap = bitmap;
  a.ustatus = ustatus;
  a.n = n;
  a.nrp = nrp;
  a.nsa = group_no_key(nrp);
  upd_carve(static_cast<uint8_t *>(ws), n, nrp, &a.w);
  if (hipMemsetAsync(a.w.hash, 0xff, (size_t)a.w.hcap * 4, st) != hipSuccess ||
      hipMemsetAsync(a.w.sa_top, 0, (size_t)a.nsa * 8, st) != hipSuccess)
    return -1;
  hipLaunchKernelGGL(upd_prep_kernel, grid_n, blk, 0, st, a);
  const int cur = group_by_key(a.w.g, n, a.nsa, st);
  a.skey = a.w.g.key[cur];
  a.order = a.w.g.idx[cur];
  hipLaunchKernelGGL(upd_scan_kernel<false>, dim3(a.w.scan_blocks), blk, 0, st, a);
  hipLaunchKernelGGL(upd_scan_carry_kernel, dim3(1), blk, 0, st, a.w);
  hipLaunchKernelGGL(upd_scan_kernel<true>, dim3(a.w.scan_blocks), blk, 0, st, a);
  hipLaunchKernelGGL(upd_decide_kernel, grid_n, blk, 0, st, a);
  hipLaunchKernelGGL(upd_clear_kernel, dim3((a.nsa + 3) / 4), blk, 0, st, a);
  hipLaunchKernelGGL(upd_set_kernel, grid_n, blk, 0, st, a);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_replay_check(const uint8_t *arena, espgpu_desc *desc, uint32_t n, const espgpu_replay *rp,
                        uint32_t nrp, const uint32_t *bitmap, uint8_t *rstatus, void *stream) {
  if (n == 0) return 0;
  hipLaunchKernelGGL(replay_check_kernel, dim3((n + 255) / 256), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), arena, desc, n, rp, nrp, bitmap, rstatus);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_replay_merge(uint8_t *status, const uint8_t *rstatus, uint32_t n, void *stream) {
  if (n == 0) return 0;
  hipLaunchKernelGGL(replay_merge_kernel, dim3((n + 255) / 256), dim3(256), 0,
                     reinterpret_cast<hipStream_t>(stream), status, rstatus, n);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace espgpu
