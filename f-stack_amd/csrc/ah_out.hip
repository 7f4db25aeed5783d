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
// Step 2 is sa_group.h's five numbering steps (validate, group, segment heads,
// frame, commit), shared with frame.hip, over ah_output's rule: every read of
// a counter precedes every write.
//
// ahs_kernel: one lane per record; a qualifying lane loads its 5-15 saved
// dwords into registers and stores them over the packet's.  The counters are
// aggregated per wave and per workgroup before the 64-bit adds (sa_book.h,
// shared with the other directions' closing kernels): no lane returns before
// its barrier.
#include <hip/hip_runtime.h>

#include "ah_out.h"
#include "dev_prims.h"
#include "espgpu_internal.h"
#include "sa_book.h"
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
// ah_output's numbering rule for sa_group.h's steps.
struct AhfRule {
  uint8_t *arena;
  const DevSA *sas;
  uint32_t nsas;

  static constexpr uint8_t kNoRoom = ESPGPU_EACCES;    // xform_ah.c:949

  __device__ bool takes(const espgpu_desc &d, uint32_t, const espgpu_outsa *) const {
    return d.sa < nsas && sas[d.sa].mode == ESPGPU_CSP_MODE_DIGEST && ah_frame_takes(d.len, d.salt);
  }
  __device__ uint64_t room(const espgpu_outsa &o) const { return ah_out_room(o.count, o.flags); }
  __device__ void write(espgpu_desc *dp, uint32_t, uint32_t, const espgpu_outsa &o, uint32_t rank) const {
    const uint64_t count = o.count + rank + 1;
    const espgpu_desc d = *dp;
    ah_frame_write(arena + (size_t)d.off4 * 4, d.salt, o.spi, count);
    dp->esn_hi = (o.flags & ESPGPU_OUT_ESN) ? (uint32_t)(count >> 32) : 0u;
  }
  __device__ void commit(espgpu_outsa *dst, const espgpu_outsa &o, uint32_t, uint64_t m) const {
    dst->count = o.count + m;
  }
};

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

__global__ __launch_bounds__(256) void ahs_kernel(AhsArgs a) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
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
  sa_book_workgroup(a.enc, sa, booked, accepted);   // key_sa_recordxfer (ipsec_output.c:770)
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

size_t ah_frame_workspace_bytes(uint32_t n, uint32_t nout) { return num_workspace_bytes(n, nout); }

int launch_ah_frame(uint8_t *arena, espgpu_desc *desc, uint32_t n, espgpu_outsa *out, uint32_t nout,
                    const DevSA *sas, uint32_t nsas, uint8_t *fstatus, void *ws, void *stream) {
  const AhfRule r = {arena, sas, nsas};
  return num_batch(r, desc, n, out, nout, fstatus, ws, reinterpret_cast<hipStream_t>(stream));
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
