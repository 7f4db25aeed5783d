// frame.hip — the outbound framing of a device-resident batch before encrypt:
// espgpu_esp_frame_batch (include/espgpu.h); the rule of one
// record is frame.h's, shared with espgpu_esp_frame on the host.  esp_output hands
// out an SA's sequence numbers and counter IVs one packet after another under
// the SA lock; here a record's number is its SA's counter plus its rank among
// that SA's taking-part records, and the rank is the record's position in
// the batch grouped by SA (sa_group.hip's stable sort keeps arrival order) minus
// the position of its SA's first record.  With room = esp_out_room(count0),
// the records of rank < room are accepted and get count0 + rank + 1 and
// cntr0 + rank; the SA ends at count0 + m, cntr0 + m, m = min(k, room).
// Five steps: validate, group, segment heads, frame (reads the counters),
// commit (writes them): every read of count / cntr precedes every write.
#include <hip/hip_runtime.h>

#include "espgpu_internal.h"
#include "frame.h"
#include "sa_group.h"

namespace espgpu {

namespace {

struct FrmWs {
  GroupWs g;
  uint32_t *start;             // [nsa] grouped position of the SA's first record (SAs in the batch only)
};

struct FrmArgs {
  uint8_t *arena;
  espgpu_desc *desc;
  const uint32_t *frame;
  espgpu_outsa *out;
  const DevSA *sas;
  uint8_t *fstatus;
  const uint32_t *skey, *order;   // the sorted buffers
  uint32_t n, nout, nsa, nsas;    // nsa = group_no_key(nout)
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
  a.w.g.key[0][i] = k;
  a.w.g.idx[0][i] = i;
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
  WsCarver c{base};
  group_carve(c, n, &w->g);
  w->start = c.take<uint32_t>(group_no_key(nout));
  return c.off;
}

}  // namespace

size_t esp_frame_workspace_bytes(uint32_t n, uint32_t nout) {
  FrmWs w;
  return frm_carve(nullptr, n, nout, &w);
}

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
  a.nsa = group_no_key(nout);
  a.nsas = nsas;
  frm_carve(static_cast<uint8_t *>(ws), n, nout, &a.w);
  hipLaunchKernelGGL(frm_prep_kernel, grid_n, blk, 0, st, a);
  const int cur = group_by_key(a.w.g, n, a.nsa, st);
  a.skey = a.w.g.key[cur];
  a.order = a.w.g.idx[cur];
  hipLaunchKernelGGL(frm_heads_kernel, grid_n, blk, 0, st, a);
  hipLaunchKernelGGL(frm_frame_kernel, grid_n, blk, 0, st, a);
  hipLaunchKernelGGL(frm_commit_kernel, grid_n, blk, 0, st, a);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace espgpu
