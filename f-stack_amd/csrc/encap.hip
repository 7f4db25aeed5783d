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
// snt_kernel: one lane per record; the counters are aggregated as dcp_kernel
// aggregates its own (decap.hip; kept as a copy here because moving that code
// into a shared header changed dcp_kernel's instructions).  Per wave: for each
// distinct SA among the accepted lanes (ballot, the first such lane's SA
// broadcast, the matching lanes' bytes summed across the wave) one lane issues
// one 64-bit add pair; a workgroup whose accepted records all belong to one SA
// adds once for its four waves, through 48 bytes of LDS.  All of it runs with
// every lane of the wave on: the conditions are ballots or workgroup-uniform,
// no lane returns before the barrier, and the shuffles stand outside every
// lane-dependent branch.
#include <hip/hip_runtime.h>

#include "dev_prims.h"
#include "encap.h"
#include "espgpu_internal.h"
#include "frame.h"

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

constexpr uint32_t kSntNone = 0xfffffffeu, kSntMixed = 0xffffffffu;   // a wave's SA: no lane accepted; several SAs

__device__ __forceinline__ void snt_book(espgpu_encsa *enc, uint32_t sa, uint32_t bytes, uint32_t count) {
  atomicAdd(reinterpret_cast<unsigned long long *>(&enc[sa].bytes), (unsigned long long)bytes);
  atomicAdd(reinterpret_cast<unsigned long long *>(&enc[sa].packets), (unsigned long long)count);
}

__global__ __launch_bounds__(256) void snt_kernel(SntArgs a) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x, lane = threadIdx.x & 63u;
  uint32_t sa = 0, booked = 0;
  bool accepted = false;
  if (i < a.n) {
    sa = a.desc[i].sa;
    accepted = a.status[i] == 0 && sa < a.nenc;
    booked = a.opkt[i].len;
    // key_sa_recordxfer runs before the UDP header exists (ipsec_output.c:770, :808)
    if (accepted && (a.enc[sa].flags & ESPGPU_ENC_NATT)) booked -= 8;
  }
  // key_sa_recordxfer (ipsec_output.c:770).  Each wave first sums its leading
  // SA (the SA of its first accepted lane); when that covers every accepted
  // lane of every wave of the workgroup, one lane adds for all 256 records.
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
    s_sa[wave] = m == 0 ? kSntNone : mm == m ? lsa : kSntMixed;
    s_bytes[wave] = bytes;
    s_count[wave] = count;
  }
  __syncthreads();
  uint32_t wsa = kSntNone, wbytes = 0, wcount = 0;
  bool one = true;
  for (uint32_t w = 0; w < 4; ++w) {
    const uint32_t v = s_sa[w];
    if (v == kSntNone) continue;
    if (v == kSntMixed || (wsa != kSntNone && v != wsa)) one = false;
    wsa = v;
    wbytes += s_bytes[w];
    wcount += s_count[w];
  }
  if (one) {
    if (threadIdx.x == 0 && wsa != kSntNone) snt_book(a.enc, wsa, wbytes, wcount);
    return;
  }
  // otherwise per wave: the leading SA is summed already, then the loop over
  // the other distinct SAs among the accepted lanes
  if (m == 0) return;
  if (lane == lead) snt_book(a.enc, lsa, bytes, count);
  m &= ~mm;
  while (m) {
    const uint32_t ld = (uint32_t)__ffsll((long long)m) - 1;
    const uint32_t nsa = __shfl(sa, ld);
    const bool hit = accepted && sa == nsa;
    const unsigned long long hm = __ballot(hit);
    const uint32_t b = wave_sum(hit ? booked : 0u);
    if (lane == ld) snt_book(a.enc, nsa, b, (uint32_t)__popcll(hm));
    m &= ~hm;
  }
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
