// replay.hip — the ESP replay window for a device-resident batch: the
// pre-filter before crypto and the window update after it; and, over the
// same grouping by SA, the outbound framing before encrypt (at the end).
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
// So: a stable LSD radix sort of the records by SA (8-bit digits, as many
// passes as the SA count needs), a segmented max-scan over the grouped
// positions (three kernels, kReplayScanBlock positions per workgroup), a hash
// table holding the first grouped position per (SA, seq64), the decisions
// (which read the initial bitmap), then clear and set as two more launches.
// Every step is a grid over records or over SAs, whatever the SA mix.
#include <hip/hip_runtime.h>

#include "espgpu_internal.h"

namespace espgpu {

namespace {

__device__ __forceinline__ uint32_t be32(uint32_t x) { return __builtin_amdgcn_perm(x, x, 0x00010203u); }

// check_window (ipsec.c:1191-1201): bit (seq & 31) of word (seq >> 5) masked
// by the power-of-two bitmap size (IPSEC_REDUNDANT_BIT_SHIFTS, :1177-1180).
__device__ __forceinline__ bool seen(const espgpu_replay &r, const uint32_t *bitmap, uint32_t seq) {
  return (bitmap[r.bitmap_off + ((seq >> 5) & (r.bitmap_size - 1))] >> (seq & 31)) & 1u;
}

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
    return !(seq <= tl && seen(r, bitmap, seq));
  }
  // top of a non-ESN space reached: only SADB_X_EXT_CYCSEQ SAs go on
  if (tl == 0xffffffffu && !(r.flags & ESPGPU_REPLAY_ESN) && !(r.flags & ESPGPU_REPLAY_CYCSEQ))
    return false;
  if (tl < window - 1 && seq >= bl) {         // in the window, previous subspace
    if (th == 0) return false;
    *seqhigh = th - 1;
    return !seen(r, bitmap, seq);
  }
  *seqhigh = th + 1;                           // wrapped into the next subspace
  return !(th + 1 == 0 && !(r.flags & ESPGPU_REPLAY_CYCSEQ));
}

__global__ __launch_bounds__(256) void replay_check_kernel(const uint8_t *arena, espgpu_desc *desc, uint32_t n,
                                                           const espgpu_replay *rp, uint32_t nrp,
                                                           const uint32_t *bitmap, uint8_t *rstatus) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const espgpu_desc d = desc[i];
  uint8_t st = 0;
  if (d.sa < nrp && d.len >= 8) {
    const espgpu_replay r = rp[d.sa];
    if (r.wsize != 0) {                        // esp_input: replay != NULL && wsize != 0
      const uint32_t seq = be32(*reinterpret_cast<const uint32_t *>(arena + (size_t)d.off4 * 4 + 4));
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

constexpr uint32_t kSortItems = 8;                 // records per thread of a sort tile
constexpr uint32_t kSortTile = 256 * kSortItems;
constexpr uint32_t kScanItems = kReplayScanBlock / 256;
constexpr uint32_t kEmpty = 0xffffffffu;           // free hash slot (no grouped position is 2^32 - 1)

// The workspace of one call, carved from the ctx's buffer (replay_update_carve).
struct UpdWs {
  uint64_t *sseq;          // [n] seq64 by grouped position (0 for records that take no part)
  uint64_t *top;           // [n] the window top each grouped position sees (M_i)
  uint64_t *agg_v, *car_v; // [scan blocks] segmented-scan aggregates and carries
  uint64_t *sa_top;        // [nsa] final top per SA (0: no record took part)
  uint32_t *key[2], *idx[2];   // [n] sort buffers: SA (or nsa: takes no part), record index
  uint32_t *hash;          // [hcap] first grouped position per (SA, seq64)
  uint32_t *counts;        // [256][sort tiles] digit histograms, then their exclusive scan
  uint32_t *agg_f, *car_f; // [scan blocks] segment-head flags of the aggregates / carries
  uint64_t hcap;
  uint32_t sort_tiles, scan_blocks;
};

struct UpdArgs {
  const uint8_t *arena;
  const espgpu_desc *desc;
  const uint8_t *status;
  espgpu_replay *rp;
  uint32_t *bitmap;
  uint8_t *ustatus;
  const uint32_t *skey, *order;   // the sorted buffers
  uint32_t n, nrp, nsa;           // nsa = min(nrp, 65536): the key of a record that takes no part
  UpdWs w;
};

__host__ __device__ inline uint64_t hash_cap(uint32_t n) {
  uint64_t c = 1024;
  while (c < 2 * (uint64_t)n) c <<= 1;
  return c;
}

__device__ __forceinline__ bool window_usable(const espgpu_replay &r) {
  const uint32_t b = r.bitmap_size;
  return b != 0 && (b & (b - 1)) == 0 && (uint64_t)b * 32 >= (uint64_t)r.wsize * 8 + 32;
}

// Which records take part, and under which SA.
__global__ __launch_bounds__(256) void upd_prep_kernel(UpdArgs a) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n) return;
  const espgpu_desc d = a.desc[i];
  uint32_t k = a.nsa;
  uint8_t u = 0;
  if (a.status[i] == 0 && d.sa < a.nrp && d.len >= 8) {
    const espgpu_replay r = a.rp[d.sa];
    if (r.wsize != 0) {
      if (window_usable(r)) k = d.sa;
      else u = ESPGPU_EINVAL;
    }
  }
  a.w.key[0][i] = k;
  a.w.idx[0][i] = i;
  a.ustatus[i] = u;
}

// One stable radix pass: digit histogram per tile, ...
__global__ __launch_bounds__(256) void upd_hist_kernel(const uint32_t *key, uint32_t n, uint32_t shift,
                                                       uint32_t *counts, uint32_t tiles) {
  __shared__ uint32_t h[256];
  const uint32_t tid = threadIdx.x;
  h[tid] = 0;
  __syncthreads();
  const uint64_t base = (uint64_t)blockIdx.x * kSortTile;
  for (uint32_t k = 0; k < kSortItems; ++k) {
    const uint64_t e = base + k * 256 + tid;
    if (e < n) atomicAdd(&h[(key[e] >> shift) & 255u], 1u);
  }
  __syncthreads();
  counts[(size_t)tid * tiles + blockIdx.x] = h[tid];
}

__device__ __forceinline__ uint32_t wave_incl_add(uint32_t x, uint32_t lane) {
  for (uint32_t d = 1; d < 64; d <<= 1) {
    const uint32_t y = __shfl_up(x, d);
    if (lane >= d) x += y;
  }
  return x;
}

// ... exclusive scan of the [digit][tile] counts (one workgroup: 256 x the
// tile count is small beside n), ...
__global__ __launch_bounds__(256) void upd_scan_counts_kernel(uint32_t *c, uint64_t m) {
  __shared__ uint32_t wt[4];
  const uint32_t tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  uint32_t carry = 0;
  for (uint64_t base = 0; base < m; base += 2048) {
    const uint64_t e0 = base + (uint64_t)tid * 8;
    uint32_t x[8], sum = 0;
    for (uint32_t j = 0; j < 8; ++j) {
      x[j] = e0 + j < m ? c[e0 + j] : 0;
      sum += x[j];
    }
    const uint32_t incl = wave_incl_add(sum, lane);
    if (lane == 63) wt[wv] = incl;
    __syncthreads();
    uint32_t pre = carry, tot = 0;
    for (uint32_t k = 0; k < 4; ++k) {
      if (k < wv) pre += wt[k];
      tot += wt[k];
    }
    uint32_t ex = pre + incl - sum;
    for (uint32_t j = 0; j < 8; ++j)
      if (e0 + j < m) {
        c[e0 + j] = ex;
        ex += x[j];
      }
    carry += tot;
    __syncthreads();
  }
}

// ... and the scatter, which keeps the input order among equal digits: rounds
// in tile order, waves in order within a round, lanes ranked by ballot.
__global__ __launch_bounds__(256) void upd_scatter_kernel(const uint32_t *key_in, const uint32_t *idx_in,
                                                          uint32_t *key_out, uint32_t *idx_out, uint32_t n,
                                                          uint32_t shift, const uint32_t *counts, uint32_t tiles) {
  __shared__ uint32_t base[256];
  __shared__ uint32_t wc[4][256];
  const uint32_t tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  base[tid] = counts[(size_t)tid * tiles + blockIdx.x];
  for (uint32_t k = 0; k < 4; ++k) wc[k][tid] = 0;
  __syncthreads();
  const uint64_t tile0 = (uint64_t)blockIdx.x * kSortTile;
  for (uint32_t k = 0; k < kSortItems; ++k) {
    const uint64_t e = tile0 + k * 256 + tid;
    const bool valid = e < n;
    const uint32_t kv = valid ? key_in[e] : 0;
    const uint32_t d = (kv >> shift) & 255u;
    unsigned long long m = __ballot(valid);
    for (uint32_t bit = 0; bit < 8; ++bit) {
      const bool on = (d >> bit) & 1u;
      const unsigned long long b = __ballot(on);
      m &= on ? b : ~b;
    }
    const uint32_t rank = __popcll(m & ((1ull << lane) - 1));
    if (valid && rank == 0) wc[wv][d] = __popcll(m);
    __syncthreads();
    if (valid) {
      uint32_t pos = base[d] + rank;
      for (uint32_t q = 0; q < wv; ++q) pos += wc[q][d];
      key_out[pos] = kv;
      idx_out[pos] = idx_in[e];
    }
    __syncthreads();
    base[tid] += wc[0][tid] + wc[1][tid] + wc[2][tid] + wc[3][tid];
    for (uint32_t q = 0; q < 4; ++q) wc[q][tid] = 0;
    __syncthreads();
  }
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
          const uint32_t seq = be32(*reinterpret_cast<const uint32_t *>(a.arena + (size_t)d.off4 * 4 + 4));
          s[j] = (a.rp[key[j]].flags & ESPGPU_REPLAY_ESN) ? ((uint64_t)d.esn_hi << 32) | seq : seq;
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
    const uint32_t word = a.bitmap[r.bitmap_off + (uint32_t)((s >> 5) & (r.bitmap_size - 1))];
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
    atomicOr(&a.bitmap[r.bitmap_off + (uint32_t)((s >> 5) & (r.bitmap_size - 1))], 1u << (s & 31));
}

uint32_t upd_nsa(uint32_t nrp) { return nrp < 65536u ? nrp : 65536u; }

size_t upd_carve(uint8_t *base, uint32_t n, uint32_t nrp, UpdWs *w) {
  UpdWs t{};
  t.hcap = hash_cap(n);
  t.sort_tiles = (uint32_t)(((uint64_t)n + kSortTile - 1) / kSortTile);
  t.scan_blocks = (uint32_t)(((uint64_t)n + kReplayScanBlock - 1) / kReplayScanBlock);
  size_t off = 0;
  auto take = [&](size_t bytes) {
    uint8_t *p = base + off;
    off += (bytes + 255) & ~(size_t)255;
    return p;
  };
  t.sseq = (uint64_t *)take((size_t)n * 8);
  t.top = (uint64_t *)take((size_t)n * 8);
  t.agg_v = (uint64_t *)take((size_t)t.scan_blocks * 8);
  t.car_v = (uint64_t *)take((size_t)t.scan_blocks * 8);
  t.sa_top = (uint64_t *)take((size_t)upd_nsa(nrp) * 8);
  for (int k = 0; k < 2; ++k) {
    t.key[k] = (uint32_t *)take((size_t)n * 4);
    t.idx[k] = (uint32_t *)take((size_t)n * 4);
  }
  t.hash = (uint32_t *)take((size_t)t.hcap * 4);
  t.counts = (uint32_t *)take((size_t)t.sort_tiles * 256 * 4);
  t.agg_f = (uint32_t *)take((size_t)t.scan_blocks * 4);
  t.car_f = (uint32_t *)take((size_t)t.scan_blocks * 4);
  if (w) *w = t;
  return off;
}

// The stable grouping of n (key, index) pairs in key[0] / idx[0] by key: keys
// are 0 .. nsa, so as many 8-bit passes as nsa has digits.  Returns which of
// the two buffer pairs holds the result.
int group_by_key(uint32_t *const key[2], uint32_t *const idx[2], uint32_t *counts, uint32_t tiles, uint32_t n,
                 uint32_t nsa, hipStream_t st) {
  const dim3 blk(256);
  int cur = 0;
  for (uint32_t shift = 0; (nsa >> shift) != 0; shift += 8) {
    hipLaunchKernelGGL(upd_hist_kernel, dim3(tiles), blk, 0, st, key[cur], n, shift, counts, tiles);
    hipLaunchKernelGGL(upd_scan_counts_kernel, dim3(1), blk, 0, st, counts, (uint64_t)tiles * 256);
    hipLaunchKernelGGL(upd_scatter_kernel, dim3(tiles), blk, 0, st, key[cur], idx[cur], key[cur ^ 1],
                       idx[cur ^ 1], n, shift, counts, tiles);
    cur ^= 1;
  }
  return cur;
}

// ---- outbound framing ------------------------------------------------------------
// espgpu_esp_frame_batch (include/espgpu.h).  esp_output hands
// out an SA's sequence numbers and counter IVs one packet after another under
// the SA lock; here a record's number is its SA's counter plus its rank among
// that SA's taking-part records, and the rank is the record's position in
// the batch grouped by SA (the stable sort above keeps arrival order) minus
// the position of its SA's first record.  With room = esp_out_room(count0),
// the records of rank < room are accepted and get count0 + rank + 1 and
// cntr0 + rank; the SA ends at count0 + m, cntr0 + m, m = min(k, room).
// Five steps: validate, group, segment heads, frame (reads the counters),
// commit (writes them): every read of count / cntr precedes every write.
struct FrmWs {
  uint32_t *key[2], *idx[2];   // [n] sort buffers: SA (or nsa: takes no part), record index
  uint32_t *counts;            // [256][sort tiles]
  uint32_t *start;             // [nsa] grouped position of the SA's first record (SAs in the batch only)
  uint32_t sort_tiles;
};

struct FrmArgs {
  uint8_t *arena;
  espgpu_desc *desc;
  const uint32_t *frame;
  espgpu_outsa *out;
  const DevSA *sas;
  uint8_t *fstatus;
  const uint32_t *skey, *order;   // the sorted buffers
  uint32_t n, nout, nsa, nsas;    // nsa = min(nout, 65536): the key of a record that takes no part
  FrmWs w;
};

__device__ __forceinline__ bool frm_shape(const FrmArgs &a, uint32_t sa, uint32_t oflags, espgpu_eshape *s) {
  const DevSA &d = a.sas[sa];
  return esp_shape_of(d.mode, d.calg, d.mlen, oflags, s);
}

// Which records take part, and under which SA; the others are refused here.
__global__ __launch_bounds__(256) void frm_prep_kernel(FrmArgs a) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n) return;
  const espgpu_desc d = a.desc[i];
  const uint32_t rlen = a.frame[i] & 0xffffu;
  uint32_t k = a.nsa;
  if (d.sa < a.nout && d.sa < a.nsas) {
    espgpu_eshape s;
    if (frm_shape(a, d.sa, a.out[d.sa].flags, &s) &&
        8 + s.ivlen + rlen + esp_padding(rlen, s.blks) + s.alen == (uint32_t)d.len)
      k = d.sa;
  }
  a.w.key[0][i] = k;
  a.w.idx[0][i] = i;
  a.fstatus[i] = k == a.nsa ? ESPGPU_EINVAL : 0;
  if (k == a.nsa) a.desc[i].len = 0;
}

__global__ __launch_bounds__(256) void frm_heads_kernel(FrmArgs a) {
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= a.n) return;
  const uint32_t key = a.skey[p];
  if (key < a.nsa && (p == 0 || a.skey[p - 1] != key)) a.w.start[key] = p;
}

// One lane per grouped position: the record's number and IV from its rank,
// then the bytes esp_output writes.
__global__ __launch_bounds__(256) void frm_frame_kernel(FrmArgs a) {
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= a.n) return;
  const uint32_t key = a.skey[p];
  if (key >= a.nsa) return;
  const uint32_t i = a.order[p], rank = p - a.w.start[key];
  const espgpu_outsa o = a.out[key];
  if (rank >= esp_out_room(o.count, o.flags)) {       // the number space ended inside this batch
    a.fstatus[i] = ESPGPU_EINVAL;
    a.desc[i].len = 0;
    return;
  }
  espgpu_eshape s;
  if (!frm_shape(a, key, o.flags, &s)) return;        // (frm_prep_kernel accepted it)
  const uint64_t count = o.count + rank + 1;
  const uint32_t f = a.frame[i];
  esp_frame_write(a.arena + (size_t)a.desc[i].off4 * 4, s, o.flags, o.spi, count, o.cntr + rank, f & 0xffffu,
                  (uint8_t)(f >> 16));
  a.desc[i].esn_hi = (o.flags & ESPGPU_OUT_ESN) ? (uint32_t)(count >> 32) : 0u;
  if (s.ivlen == 8) a.desc[i].salt = o.salt;
}

// At the last grouped position of each SA: move its counters past what the
// framing kernel gave out.
__global__ __launch_bounds__(256) void frm_commit_kernel(FrmArgs a) {
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= a.n) return;
  const uint32_t key = a.skey[p];
  if (key >= a.nsa || (p + 1 < a.n && a.skey[p + 1] == key)) return;
  const espgpu_outsa o = a.out[key];
  const uint64_t k = (uint64_t)(p - a.w.start[key]) + 1, room = esp_out_room(o.count, o.flags);
  const uint64_t m = k < room ? k : room;
  espgpu_eshape s;
  if (m == 0 || !frm_shape(a, key, o.flags, &s)) return;
  a.out[key].count = o.count + m;
  if (s.ivlen == 8) a.out[key].cntr = o.cntr + m;
}

size_t frm_carve(uint8_t *base, uint32_t n, uint32_t nout, FrmWs *w) {
  FrmWs t{};
  t.sort_tiles = (uint32_t)(((uint64_t)n + kSortTile - 1) / kSortTile);
  size_t off = 0;
  auto take = [&](size_t bytes) {
    uint8_t *p = base + off;
    off += (bytes + 255) & ~(size_t)255;
    return p;
  };
  for (int k = 0; k < 2; ++k) {
    t.key[k] = (uint32_t *)take((size_t)n * 4);
    t.idx[k] = (uint32_t *)take((size_t)n * 4);
  }
  t.counts = (uint32_t *)take((size_t)t.sort_tiles * 256 * 4);
  t.start = (uint32_t *)take((size_t)upd_nsa(nout) * 4);
  if (w) *w = t;
  return off;
}

}  // namespace

size_t esp_frame_workspace_bytes(uint32_t n, uint32_t nout) { return frm_carve(nullptr, n, nout, nullptr); }

int launch_esp_frame(uint8_t *arena, espgpu_desc *desc, const uint32_t *frame, uint32_t n, espgpu_outsa *out,
                     uint32_t nout, const DevSA *sas, uint32_t nsas, uint8_t *fstatus, void *ws, void *stream) {
  if (n == 0) return 0;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const dim3 blk(256), grid_n((n + 255) / 256);
  FrmArgs a{};
  a.arena = arena;
  a.desc = desc;
  a.frame = frame;
  a.out = out;
  a.sas = sas;
  a.fstatus = fstatus;
  a.n = n;
  a.nout = nout;
  a.nsa = upd_nsa(nout);
  a.nsas = nsas;
  frm_carve(static_cast<uint8_t *>(ws), n, nout, &a.w);
  hipLaunchKernelGGL(frm_prep_kernel, grid_n, blk, 0, st, a);
  const int cur = group_by_key(a.w.key, a.w.idx, a.w.counts, a.w.sort_tiles, n, a.nsa, st);
  a.skey = a.w.key[cur];
  a.order = a.w.idx[cur];
  hipLaunchKernelGGL(frm_heads_kernel, grid_n, blk, 0, st, a);
  hipLaunchKernelGGL(frm_frame_kernel, grid_n, blk, 0, st, a);
  hipLaunchKernelGGL(frm_commit_kernel, grid_n, blk, 0, st, a);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

size_t replay_update_workspace_bytes(uint32_t n, uint32_t nrp) { return upd_carve(nullptr, n, nrp, nullptr); }

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
  a.nsa = upd_nsa(nrp);
  upd_carve(static_cast<uint8_t *>(ws), n, nrp, &a.w);
  if (hipMemsetAsync(a.w.hash, 0xff, (size_t)a.w.hcap * 4, st) != hipSuccess ||
      hipMemsetAsync(a.w.sa_top, 0, (size_t)a.nsa * 8, st) != hipSuccess)
    return -1;
  hipLaunchKernelGGL(upd_prep_kernel, grid_n, blk, 0, st, a);
  const int cur = group_by_key(a.w.key, a.w.idx, a.w.counts, a.w.sort_tiles, n, a.nsa, st);
  a.skey = a.w.key[cur];
  a.order = a.w.idx[cur];
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
