// sa_group.hip — a stable LSD radix sort of a batch's records by SA, 8-bit
// digits, kSortTile records per workgroup (sa_group.h; DESIGN.md 3.4 has the
// argument for the window update, 3.6 for the framing).  Three kernels per
// pass: digit histogram per tile, exclusive scan of the [digit][tile] counts,
// scatter.
#include "sa_group.h"

#include "dev_prims.h"

namespace espgpu {

namespace {

// One stable radix pass: digit histogram per tile, ...
__global__ __launch_bounds__(256) void grp_hist_kernel(const uint32_t *key, uint32_t n, uint32_t shift,
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

// ... exclusive scan of the [digit][tile] counts (one workgroup: 256 x the
// tile count is small beside n), ...
__global__ __launch_bounds__(256) void grp_scan_counts_kernel(uint32_t *c, uint64_t m) {
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
__global__ __launch_bounds__(256) void grp_scatter_kernel(const uint32_t *key_in, const uint32_t *idx_in,
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

// One lane per grouped position: where a key's segment starts.
__global__ __launch_bounds__(256) void grp_heads_kernel(const uint32_t *skey, uint32_t *start, uint32_t n,
                                                        uint32_t nokey) {
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= n) return;
  const uint32_t key = skey[p];
  if (key < nokey && (p == 0 || skey[p - 1] != key)) start[key] = p;
}

}  // namespace

void group_heads(const uint32_t *skey, uint32_t *start, uint32_t n, uint32_t nokey, hipStream_t st) {
  hipLaunchKernelGGL(grp_heads_kernel, dim3((n + 255) / 256), dim3(256), 0, st, skey, start, n, nokey);
}

int group_by_key(const GroupWs &g, uint32_t n, uint32_t nokey, hipStream_t st) {
  const dim3 blk(256), tiles(g.sort_tiles);
  int cur = 0;
  for (uint32_t shift = 0; (nokey >> shift) != 0; shift += 8) {
    hipLaunchKernelGGL(grp_hist_kernel, tiles, blk, 0, st, g.key[cur], n, shift, g.counts, g.sort_tiles);
    hipLaunchKernelGGL(grp_scan_counts_kernel, dim3(1), blk, 0, st, g.counts, (uint64_t)g.sort_tiles * 256);
    hipLaunchKernelGGL(grp_scatter_kernel, tiles, blk, 0, st, g.key[cur], g.idx[cur], g.key[cur ^ 1], g.idx[cur ^ 1],
                       n, shift, g.counts, g.sort_tiles);
    cur ^= 1;
  }
  return cur;
}

}  // namespace espgpu
