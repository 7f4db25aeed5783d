// encap.hip — the first and the last step of the outbound sequence on a
// device-resident batch (include/espgpu.h, the encapsulation block): from
// cleartext IP packets to the ESP-shaped records espgpu_esp_frame_batch takes,
// and the SAs' lifetime counters once the packets went through.
// ipsec4/6_perform_request's transport-or-tunnel decision, ipsec_encap's outer
// header, esp_output's m_makespace move, size check and protocol field,
// ipsec_process_done's length fields and key_sa_recordxfer, for every packet
// in parallel; the rule itself is encap.h's, shared with espgpu_esp_encap on
// the host.
//
// enc_kernel: one lane per packet, no LDS, no workspace.  A packet costs the
// dense arrays (its espgpu_pkt and SA id in; descriptor, frame word, espgpu_pkt
// and status byte out), its SA's 40 policy bytes and the session's mode / calg
// / mlen from L2, and its own header: 5-15 dwords loaded into registers, then
// either stored hlen bytes lower (transport) or two of them stored back and
// 5 or 10 new ones in front (tunnel).  The caller keeps the spans [pkt -
// headroom, pkt + len + tailroom) of one batch apart, so no lane writes what
// another reads.
//
// snt_kernel: one lane per record; the counters are aggregated per wave and
// per workgroup before the 64-bit adds (sa_book.h, shared with the other
// directions' closing kernels): no lane returns before its barrier.
#include <hip/hip_runtime.h>

#include "dev_prims.h"
#include "encap.h"
#include "espgpu_internal.h"
#include "frame.h"
#include "sa_book.h"

namespace espgpu {

namespace {

struct EncArgs {
  uint8_t *arena;
  const espgpu_pkt *pkt;
  const uint16_t *sa;
  const espgpu_encsa *enc;
  const espgpu_outsa *out;
  const DevSA *sas;
  espgpu_desc *desc;
  uint32_t *frame;
  espgpu_pkt *opkt;
  uint8_t *estatus;
  uint32_t n, nenc, nsas, headroom, tailroom, id0;
};

__global__ __launch_bounds__(256) void enc_kernel(EncArgs a) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n) return;
  const espgpu_pkt p = a.pkt[i];
  const uint32_t sa = a.sa[i];
  espgpu_desc d = {p.off4, 0, 0xffff, 0, 0};
  espgpu_pkt r = {p.off4, 0};
  int st = ESPGPU_EINVAL;
  espgpu_eshape s;
  if (sa < a.nenc && sa < a.nsas &&
      esp_shape_of(a.sas[sa].mode, a.sas[sa].calg, a.sas[sa].mlen, a.out[sa].flags, &s)) {
    EncapOut o;
    st = esp_encap_rule(&a.enc[sa], s, a.arena + (size_t)p.off4 * 4, p.len, a.headroom, a.tailroom,
                        (a.id0 + i) & 0xffffu, &o);
    if (st == 0) {
      r.off4 = p.off4 - o.front / 4;
      r.len = o.total;
      d.off4 = r.off4 + (o.total - o.reclen) / 4;      // behind the outer or the moved header
      d.len = (uint16_t)o.reclen;
      d.sa = (uint16_t)sa;
      a.frame[i] = o.frame;
    }
  }
  a.desc[i] = d;
  a.opkt[i] = r;
  a.estatus[i] = (uint8_t)st;
}

struct SntArgs {
  const espgpu_pkt *opkt;
  const espgpu_desc *desc;
  const uint8_t *status;
  espgpu_encsa *enc;
  uint32_t n, nenc;
};

__global__ __launch_bounds__(256) void snt_kernel(SntArgs a) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t sa = 0, booked = 0;
  bool accepted = false;
  if (i < a.n) {
    sa = a.desc[i].sa;
    accepted = a.status[i] == 0 && sa < a.nenc;
    booked = a.opkt[i].len;
    // key_sa_recordxfer runs before the UDP header exists (ipsec_output.c:770, :808)
    if (accepted && (a.enc[sa].flags & ESPGPU_ENC_NATT)) booked -= 8;
  }
  sa_book_workgroup(a.enc, sa, booked, accepted);   // key_sa_recordxfer (ipsec_output.c:770)
}

}  // namespace

int launch_esp_encap(uint8_t *arena, const espgpu_pkt *pkt, const uint16_t *sa, uint32_t n, const espgpu_encsa *enc,
                     const espgpu_outsa *out, uint32_t nenc, const DevSA *sas, uint32_t nsas, uint32_t headroom,
                     uint32_t tailroom, uint32_t id0, espgpu_desc *desc, uint32_t *frame, espgpu_pkt *opkt,
                     uint8_t *estatus, void *stream) {
  if (n == 0) return 0;
  const EncArgs a = {arena, pkt, sa, enc, out, sas, desc, frame, opkt, estatus, n, nenc, nsas, headroom, tailroom, id0};
  hipLaunchKernelGGL(enc_kernel, dim3((n + 255) / 256), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), a);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_esp_sent(const espgpu_pkt *opkt, const espgpu_desc *desc, const uint8_t *status, uint32_t n,
                    espgpu_encsa *enc, uint32_t nenc, void *stream) {
  if (n == 0) return 0;
  const SntArgs a = {opkt, desc, status, enc, n, nenc};
  hipLaunchKernelGGL(snt_kernel, dim3((n + 255) / 256), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), a);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace espgpu
