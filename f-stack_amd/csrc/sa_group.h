// sa_group.h — the stable grouping of a batch's records by SA (sa_group.hip),
// which the window update (replay.hip) and the outbound numbering (frame.hip,
// ah_out.hip) are built on, the carving of a stage's workspace, and the five
// numbering steps themselves over a protocol's rule.
#pragma once
#include <hip/hip_runtime.h>

#include <stddef.h>
#include <stdint.h>

#include "espgpu.h"

namespace espgpu {

constexpr uint32_t kSortItems = 8;                 // records per thread of a sort tile
constexpr uint32_t kSortTile = 256 * kSortItems;

// The key of a record that takes no part: one past the SA keys, which are 16
// bits in a descriptor.  Such records group behind every SA's.
inline uint32_t group_no_key(uint32_t nsa) { return nsa < 65536u ? nsa : 65536u; }

// Hands out a stage's workspace piece by piece, each 256-byte aligned.  Over
// base == nullptr it only measures: off is then the bytes the layout needs.
struct WsCarver {
  uint8_t *base;
  size_t off = 0;
  template <class T>
  T *take(size_t count) {
    T *p = reinterpret_cast<T *>(base + off);
    off += (count * sizeof(T) + 255) & ~(size_t)255;
    return p;
  }
};

struct GroupWs {
  uint32_t *key[2], *idx[2];   // [n] sort buffers: SA (or group_no_key: takes no part), record index
  uint32_t *counts;            // [256][sort tiles] digit histograms, then their exclusive scan
  uint32_t sort_tiles;
};

inline void group_carve(WsCarver &c, uint32_t n, GroupWs *g) {
  g->sort_tiles = (uint32_t)(((uint64_t)n + kSortTile - 1) / kSortTile);
  for (int k = 0; k < 2; ++k) {
    g->key[k] = c.take<uint32_t>(n);
    g->idx[k] = c.take<uint32_t>(n);
  }
  g->counts = c.take<uint32_t>((size_t)g->sort_tiles * 256);
}

// The stable grouping of the n (key, index) pairs in key[0] / idx[0] by key:
// keys are 0 .. nokey, so as many 8-bit passes as nokey has digits.  Returns
// which of the two buffer pairs holds the result.
int group_by_key(const GroupWs &g, uint32_t n, uint32_t nokey, hipStream_t st);

// start[key] = the grouped position of the first record of every key < nokey
// that occurs among the n sorted keys (n > 0); the other entries stay as they are.
void group_heads(const uint32_t *skey, uint32_t *start, uint32_t n, uint32_t nokey, hipStream_t st);

// ---- outbound numbering -------------------------------------------------------
// The reference hands out an SA's sequence numbers one packet after another
// under the SA lock; here a record's number is its SA's counter plus its rank
// among that SA's taking-part records, and the rank is the record's position in
// the batch grouped by SA (the stable sort keeps arrival order) minus the
// position of its SA's first record.  With room = Rule::room(SA), the records
// of rank < room are accepted; the SA moves on by m = min(k, room).  Five
// steps: prep (validate), group, segment heads, frame (reads the counters),
// commit (writes them): every read of a counter precedes every write.
//
// A Rule is a small struct passed to the kernels by value, with
//   static constexpr uint8_t kNoRoom     the status of a record the number space ended before
//   bool takes(d, i, o)                  does record i (descriptor d) take part under SA d.sa (o = out[d.sa])?
//   uint64_t room(o)                     numbers the SA may still give out
//   void write(desc_i, i, key, o, rank)  the record of rank `rank`: its bytes and descriptor fields
//   void commit(out_key, o, key, m)      the SA's counters past the m numbers given out
// all __device__ and const.  The segment heads need no rule: group_heads.

struct NumWs {
  GroupWs g;
  uint32_t *start;             // [nsa] grouped position of the SA's first record (SAs in the batch only)
};

inline size_t num_carve(uint8_t *base, uint32_t n, uint32_t nout, NumWs *w) {
  WsCarver c{base};
  group_carve(c, n, &w->g);
  w->start = c.take<uint32_t>(group_no_key(nout));
  return c.off;
}

inline size_t num_workspace_bytes(uint32_t n, uint32_t nout) {
  NumWs w;
  return num_carve(nullptr, n, nout, &w);
}

template <class Rule>
struct NumArgs {
  espgpu_desc *desc;
  espgpu_outsa *out;
  uint8_t *fstatus;
  Rule r;
  const uint32_t *skey, *order;   // the sorted buffers
  uint32_t n, nout, nsa;          // nsa = group_no_key(nout)
  NumWs w;
};

// Which records take part, and under which SA; the others are refused here.
template <class Rule>
__global__ __launch_bounds__(256) void num_prep_kernel(NumArgs<Rule> a) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n) return;
  const espgpu_desc d = a.desc[i];
  uint32_t k = a.nsa;
  if (d.sa < a.nout && a.r.takes(d, i, a.out + d.sa)) k = d.sa;
  a.w.g.key[0][i] = k;
  a.w.g.idx[0][i] = i;
  a.fstatus[i] = k == a.nsa ? ESPGPU_EINVAL : 0;
  if (k == a.nsa) a.desc[i].len = 0;
}

// One lane per grouped position: the record's number from its rank.
template <class Rule>
__global__ __launch_bounds__(256) void num_frame_kernel(NumArgs<Rule> a) {
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= a.n) return;
  const uint32_t key = a.skey[p];
  if (key >= a.nsa) return;
  const uint32_t i = a.order[p], rank = p - a.w.start[key];
  const espgpu_outsa o = a.out[key];
  if (rank >= a.r.room(o)) {                           // the number space ended inside this batch
    a.fstatus[i] = Rule::kNoRoom;
    a.desc[i].len = 0;
    return;
  }
  a.r.write(a.desc + i, i, key, o, rank);
}

// At the last grouped position of each SA: move its counters past what the
// framing kernel gave out.
template <class Rule>
__global__ __launch_bounds__(256) void num_commit_kernel(NumArgs<Rule> a) {
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= a.n) return;
  const uint32_t key = a.skey[p];
  if (key >= a.nsa || (p + 1 < a.n && a.skey[p + 1] == key)) return;
  const espgpu_outsa o = a.out[key];
  const uint64_t k = (uint64_t)(p - a.w.start[key]) + 1, room = a.r.room(o);
  const uint64_t m = k < room ? k : room;
  if (m == 0) return;
  a.r.commit(a.out + key, o, key, m);
}

template <class Rule>
int num_batch(const Rule &r, espgpu_desc *desc, uint32_t n, espgpu_outsa *out, uint32_t nout, uint8_t *fstatus,
              void *ws, hipStream_t st) {
  if (n == 0) return 0;
  const dim3 blk(256), grid_n((n + 255) / 256);
  NumArgs<Rule> a{};
  a.r = r;
  a.desc = desc;
  a.out = out;
  a.fstatus = fstatus;
  a.n = n;
  a.nout = nout;
  a.nsa = group_no_key(nout);
  num_carve(static_cast<uint8_t *>(ws), n, nout, &a.w);
  hipLaunchKernelGGL(num_prep_kernel<Rule>, grid_n, blk, 0, st, a);
  const int cur = group_by_key(a.w.g, n, a.nsa, st);
  a.skey = a.w.g.key[cur];
  a.order = a.w.g.idx[cur];
  group_heads(a.skey, a.w.start, n, a.nsa, st);
  hipLaunchKernelGGL(num_frame_kernel<Rule>, grid_n, blk, 0, st, a);
  hipLaunchKernelGGL(num_commit_kernel<Rule>, grid_n, blk, 0, st, a);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace espgpu
