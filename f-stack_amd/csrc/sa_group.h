// sa_group.h — the stable grouping of a batch's records by SA (sa_group.hip),
// which the window update (replay.hip) and the outbound framing (frame.hip)
// are built on, and the carving of a stage's workspace.
#pragma once
#include <hip/hip_runtime.h>

#include <stddef.h>
#include <stdint.h>

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

}  // namespace espgpu
