// ah_out.hip — steps 1, 2 and 5 of the outbound AH sequence on a
// device-resident batch (include/espgpu.h, the outbound AH block): the
// transport-or-tunnel decision, ipsec_encap and ah_output's header work with
// ah_massage_headers (out = 1) in front of the digest kernel, ah_output's
// sequence numbers per SA in arrival order, and ah_output_cb's restore with
// key_sa_recordxfer behind it.  The rules are ah_out.h's, shared with
// espgpu_ah_encap, espgpu_ah_frame and espgpu_ah_sent on the host.
//
// aho_kernel: one lane per packet, no LDS, no workspace.  A lane reads its
// espgpu_pkt and SA id, the SA's policy and the session's mode and mlen (L2),
// the packet's first dword (and, in the proxy case, its destination), then the
// header: 5 dwords (IPv4 without options), 10 (IPv6) or up to 15.  The IPv4
// option loop is byte-serial and lane-dependent, so a wave runs it only if a
// ballot finds a lane whose packet header is longer than 20 bytes; the common
// wave takes the 10-dword instantiation of the rule, which has no loop in it.
// The loop reads the option bytes from the packet as it arrived and leaves a
// 40-bit mask of the bytes to zero and the source-route destination, which
// constant-index code applies to the registers: the header is never indexed by
// a variable.  The ballot stands where every lane of the wave reaches it, lanes
// past n included; no shuffle, no barrier.
//
// ahf_*: frame.hip's five steps (validate, group, segment heads, frame,
// commit) with ah_output's rule: every read of a counter precedes every write.
//
// ahs_kernel: one lane per record; a qualifying lane loads its 5-15 saved
// dwords into registers and stores them over the packet's.  The counters are
// aggregated as snt_kernel aggregates its own (encap.hip; a copy, because
// moving that code into a shared header changes the older kernels'
// instructions): per wave one add pair per distinct SA, per workgroup one where
// one SA has all of it.  Every lane of the wave stays on up to the barrier; the
// shuffles stand outside every lane-dependent branch.
#include <hip/hip_runtime.h>

#include "ah_out.h"
#include "dev_prims.h"
#include "espgpu_internal.h"
#include "sa_group.h"

namespace espgpu {

namespace {

struct AhoArgs {
  uint8_t *arena;
  const espgpu_pkt *pkt;
  const uint16_t *sa;
  const espgpu_encsa *enc;
  const DevSA *sas;
  uint8_t *hsave;
  espgpu_desc *desc;
  espgpu_pkt *opkt;
  uint8_t *estatus;
  uint32_t n, nenc, nsas, headroom, id0;
};

__global__ __launch_bounds__(256) void aho_kernel(AhoArgs a) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  bool go = false;
  int st = ESPGPU_EINVAL;
  uint32_t sa = 0, mlen = 0, len = 0, off4 = 0;
  uint8_t *pkt = nullptr;
  AhOutPlan pl = {};
  if (i < a.n) {
    const espgpu_pkt p = a.pkt[i];
    sa = a.sa[i];
    off4 = p.off4;
    len = p.len;
    if (sa < a.nenc && sa < a.nsas && a.sas[sa].mode == ESPGPU_CSP_MODE_DIGEST) {
      mlen = a.sas[sa].mlen;
      pkt = a.arena + (size_t)p.off4 * 4;
      st = ah_out_plan(&a.enc[sa], mlen, pkt, len, a.headroom, &pl);
      go = st == 0;
    }
  }
  const espgpu_encsa *const e = a.enc + (go ? sa : 0u);
  uint8_t *const slot = a.hsave + (size_t)i * kAhSaveSlot;
  const bool opts = go && !pl.in6 && pl.skip > 20;
  if (__ballot(opts)) {
    if (go) st = ah_out_build<15>(e, mlen, pkt, len, (a.id0 + i) & 0xffffu, pl, slot);
  } else {
    if (go) st = ah_out_build<10>(e, mlen, pkt, len, (a.id0 + i) & 0xffffu, pl, slot);
  }
  if (i < a.n) {
    espgpu_desc d = {off4, 0, 0xffff, 0, 0};
    espgpu_pkt r = {off4, 0};
    if (st == 0) {
      r.off4 = off4 - (pl.ahsize + pl.oh) / 4;
      r.len = pl.total;
      d.off4 = r.off4;
      d.len = (uint16_t)pl.total;
      d.sa = (uint16_t)sa;
      d.salt = (pl.tunnel ? pl.oh : pl.skip) + 12;
    }
    a.desc[i] = d;
    a.opkt[i] = r;
    a.estatus[i] = (uint8_t)st;
  }
}

// ---- step 2 ---------------------------------------------------------------------
struct AhfWs {
  GroupWs g;
  uint32_t *start;             // [nsa] grouped position of the SA's first record (SAs in the batch only)
};

struct AhfArgs {
  uint8_t *arena;
  espgpu_desc *desc;
  espgpu_outsa *out;
  const DevSA *sas;
  uint8_t *fstatus;
  const uint32_t *skey, *order;   // the sorted buffers
  uint32_t n, nout, nsa, nsas;    // nsa = group_no_key(nout)
  AhfWs w;
};

// Which records take part, and under which SA; the others are refused here.
__global__ __launch_bounds__(256) void ahf_prep_kernel(AhfArgs a) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n) return;
  const espgpu_desc d = a.desc[i];
  uint32_t k = a.nsa;
  if (d.sa < a.nout && d.sa < a.nsas && a.sas[d.sa].mode == ESPGPU_CSP_MODE_DIGEST && ah_frame_takes(d.len, d.salt))
    k = d.sa;
  a.w.g.key[0][i] = k;
  a.w.g.idx[0][i] = i;
  a.fstatus[i] = k == a.nsa ? ESPGPU_EINVAL : 0;
  if (k == a.nsa) a.desc[i].len = 0;
}

__global__ __launch_bounds__(256) void ahf_heads_kernel(AhfArgs a) {
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= a.n) return;
  const uint32_t key = a.skey[p];
  if (key < a.nsa && (p == 0 || a.skey[p - 1] != key)) a.w.start[key] = p;
}

// One lane per grouped position: the record's number from its rank.
__global__ __launch_bounds__(256) void ahf_frame_kernel(AhfArgs a) {
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= a.n) return;
  const uint32_t key = a.skey[p];
  if (key >= a.nsa) return;
  const uint32_t i = a.order[p], rank = p - a.w.start[key];
  const espgpu_outsa o = a.out[key];
  if (rank >= ah_out_room(o.count, o.flags)) {        // the number space ended inside this batch (xform_ah.c:949)
    a.fstatus[i] = ESPGPU_EACCES;
    a.desc[i].len = 0;
    return;
  }
  const uint64_t count = o.count + rank + 1;
  const espgpu_desc d = a.desc[i];
  ah_frame_write(a.arena + (size_t)d.off4 * 4, d.salt, o.spi, count);
  a.desc[i].esn_hi = (o.flags & ESPGPU_OUT_ESN) ? (uint32_t)(count >> 32) : 0u;
}

// At the last grouped position of each SA: move its counter past what the
// framing kernel gave out.
__global__ __launch_bounds__(256) void ahf_commit_kernel(AhfArgs a) {
  const uint32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= a.n) return;
  const uint32_t key = a.skey[p];
  if (key >= a.nsa || (p + 1 < a.n && a.skey[p + 1] == key)) return;
  const espgpu_outsa o = a.out[key];
  const uint64_t k = (uint64_t)(p - a.w.start[key]) + 1, room = ah_out_room(o.count, o.flags);
  const uint64_t m = k < room ? k : room;
  if (m == 0) return;
  a.out[key].count = o.count + m;
}

size_t ahf_carve(uint8_t *base, uint32_t n, uint32_t nout, AhfWs *w) {
  WsCarver c{base};
  group_carve(c, n, &w->g);
  w->start = c.take<uint32_t>(group_no_key(nout));
  return c.off;
}

// ---- step 5 ---------------------------------------------------------------------
struct AhsArgs {
  uint8_t *arena;
  const espgpu_pkt *opkt;
  const espgpu_desc *desc;
  const uint8_t *status;
  espgpu_encsa *enc;
  const DevSA *sas;
  const uint8_t *hsave;
  uint8_t *sstatus;
  uint32_t n, nenc, nsas;
};

constexpr uint32_t kAhsNone = 0xfffffffeu, kAhsMixed = 0xffffffffu;   // a wave's SA: no lane accepted; several SAs

__device__ __forceinline__ void ahs_book(espgpu_encsa *enc, uint32_t sa, uint32_t bytes, uint32_t count) {
  atomicAdd(reinterpret_cast<unsigned long long *>(&enc[sa].bytes), (unsigned long long)bytes);
  atomicAdd(reinterpret_cast<unsigned long long *>(&enc[sa].packets), (unsigned long long)count);
}

__global__ __launch_bounds__(256) void ahs_kernel(AhsArgs a) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x, lane = threadIdx.x & 63u;
  uint32_t sa = 0, booked = 0;
  bool accepted = false;
  if (i < a.n) {
    const espgpu_desc d = a.desc[i];
    int st = 0;
    if (a.status[i] == 0 && d.sa < a.nenc && d.sa < a.nsas && a.sas[d.sa].mode == ESPGPU_CSP_MODE_DIGEST) {
      const uint32_t ef = a.enc[d.sa].flags;
      if (ef & ESPGPU_ENC_AH) {
        const espgpu_pkt p = a.opkt[i];
        st = ah_sent_rule(ef, a.arena + (size_t)p.off4 * 4, p.len, d.salt, a.hsave + (size_t)i * kAhSaveSlot);
        if (st == 0) {
          sa = d.sa;
          booked = p.len;
          accepted = true;
        }
      }
    }
    a.sstatus[i] = (uint8_t)st;
  }
  // key_sa_recordxfer (ipsec_output.c:770), as snt_kernel's
  __shared__ uint32_t s_sa[4], s_bytes[4], s_count[4];
  const uint32_t wave = threadIdx.x >> 6;
  unsigned long long m = __ballot(accepted);
  const uint32_t lead = m ? (uint32_t)__ffsll((long long)m) - 1 : 0u;
  const uint32_t lsa = __shfl(sa, lead);
  const bool mine = accepted && sa == lsa;
  const unsigned long long mm = __ballot(mine);
  const uint32_t bytes = wave_sum(mine ? booked : 0u);         // 64 lanes of < 2^16 each
  const uint32_t count = (uint32_t)__popcll(mm);
  if (lane == 0) {
    s_sa[wave] = m == 0 ? kAhsNone : mm == m ? lsa : kAhsMixed;
    s_bytes[wave] = bytes;
    s_count[wave] = count;
  }
  __syncthreads();
  uint32_t wsa = kAhsNone, wbytes = 0, wcount = 0;
  bool one = true;
  for (uint32_t w = 0; w < 4; ++w) {
    const uint32_t v = s_sa[w];
    if (v == kAhsNone) continue;
    if (v == kAhsMixed || (wsa != kAhsNone && v != wsa)) one = false;
    wsa = v;
    wbytes += s_bytes[w];
    wcount += s_count[w];
  }
  if (one) {
    if (threadIdx.x == 0 && wsa != kAhsNone) ahs_book(a.enc, wsa, wbytes, wcount);
    return;
  }
  // otherwise per wave: the leading SA is summed already, then the loop over
  // the other distinct SAs among the accepted lanes (m is wave-uniform)
  if (m == 0) return;
  if (lane == lead) ahs_book(a.enc, lsa, bytes, count);
  m &= ~mm;
  while (m) {
    const uint32_t ld = (uint32_t)__ffsll((long long)m) - 1;
    const uint32_t nsa = __shfl(sa, ld);
    const bool hit = accepted && sa == nsa;
    const unsigned long long hm = __ballot(hit);
    const uint32_t b = wave_sum(hit ? booked : 0u);
    if (lane == ld) ahs_book(a.enc, nsa, b, (uint32_t)__popcll(hm));
    m &= ~hm;
  }
}

}  // namespace

int launch_ah_encap(uint8_t *arena, const espgpu_pkt *pkt, const uint16_t *sa, uint32_t n, const espgpu_encsa *enc,
                    uint32_t nenc, const DevSA *sas, uint32_t nsas, uint32_t headroom, uint32_t id0, uint8_t *hsave,
                    espgpu_desc *desc, espgpu_pkt *opkt, uint8_t *estatus, void *stream) {
  if (n == 0) return 0;
  const AhoArgs a = {arena, pkt, sa, enc, sas, hsave, desc, opkt, estatus, n, nenc, nsas, headroom, id0};
  hipLaunchKernelGGL(aho_kernel, dim3((n + 255) / 256), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), a);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

size_t ah_frame_workspace_bytes(uint32_t n, uint32_t nout) {
  AhfWs w;
  return ahf_carve(nullptr, n, nout, &w);
}

int launch_ah_frame(uint8_t *arena, espgpu_desc *desc, uint32_t n, espgpu_outsa *out, uint32_t nout,
                    const DevSA *sas, uint32_t nsas, uint8_t *fstatus, void *ws, void *stream) {
  if (n == 0) return 0;
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  const dim3 blk(256), grid_n((n + 255) / 256);
  AhfArgs a{};
  a.arena = arena;
  a.desc = desc;
  a.out = out;
  a.sas = sas;
  a.fstatus = fstatus;
  a.n = n;
  a.nout = nout;
  a.nsa = group_no_key(nout);
  a.nsas = nsas;
  ahf_carve(static_cast<uint8_t *>(ws), n, nout, &a.w);
  hipLaunchKernelGGL(ahf_prep_kernel, grid_n, blk, 0, st, a);
  const int cur = group_by_key(a.w.g, n, a.nsa, st);
  a.skey = a.w.g.key[cur];
  a.order = a.w.g.idx[cur];
  hipLaunchKernelGGL(ahf_heads_kernel, grid_n, blk, 0, st, a);
  hipLaunchKernelGGL(ahf_frame_kernel, grid_n, blk, 0, st, a);
  hipLaunchKernelGGL(ahf_commit_kernel, grid_n, blk, 0, st, a);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_ah_sent(uint8_t *arena, const espgpu_pkt *opkt, const espgpu_desc *desc, const uint8_t *status, uint32_t n,
                   espgpu_encsa *enc, uint32_t nenc, const DevSA *sas, uint32_t nsas, const uint8_t *hsave,
                   uint8_t *sstatus, void *stream) {
  if (n == 0) return 0;
  const AhsArgs a = {arena, opkt, desc, status, enc, sas, hsave, sstatus, n, nenc, nsas};
  hipLaunchKernelGGL(ahs_kernel, dim3((n + 255) / 256), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), a);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace espgpu
