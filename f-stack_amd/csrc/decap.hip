// decap.hip — step 5 of the inbound sequence on a device-resident batch
// (include/espgpu.h, the decapsulation block): from decrypted records, their
// statuses and trailer words to the packets the stack takes next.
// esp_input_cb's trailer verdict and strip, ipsec4/6_common_input_cb's header
// fix and tunnel strip, and key_sa_recordxfer for every record in parallel;
// the rule itself is decap.h's, shared with espgpu_esp_decap on the host.
//
// One lane per packet, no LDS for the packet work, no workspace.  A record costs the dense arrays
// only: its espgpu_pkt, espgpu_desc, status byte and trailer word in, its
// espgpu_pkt and status byte out.  The SA's flags and the session's mode /
// calg / mlen come from L2.  A tunnel record never touches its packet; a
// transport record loads its 5-15 header dwords into registers and stores
// them hlen bytes further on.
//
// The SA counters are aggregated per wave: for each distinct SA among the
// accepted lanes (ballot, the first such lane's SA broadcast, the matching
// lanes' bytes summed across the wave) one lane issues one 64-bit add pair.
// Same-address adds serialise at about 13 ns each, so on top of that a
// workgroup whose accepted records all belong to one SA adds once for its four
// waves, through 48 bytes of LDS: a one-SA batch puts n / 256 adds on an
// address, not n (profiles/esp_decap_batch.txt).  All of it runs with every
// lane of the wave on: the conditions are ballots or workgroup-uniform, no
// lane returns before the barrier, and the shuffles stand outside every
// lane-dependent branch.
#include <hip/hip_runtime.h>

#include "decap.h"
#include "dev_prims.h"
#include "espgpu_internal.h"
#include "frame.h"

namespace espgpu {

namespace {

struct DcpArgs {
  const uint8_t *arena;
  uint8_t *out;
  const espgpu_pkt *pkt;
  const espgpu_desc *desc;
  const uint32_t *trailer;
  const uint8_t *status;
  espgpu_insa *in;
  const DevSA *sas;
  espgpu_pkt *ipkt;
  uint8_t *dstatus;
  uint32_t n, nin, nsas;
};

constexpr uint32_t kDcpNone = 0xfffffffeu, kDcpMixed = 0xffffffffu;   // a wave's SA: no lane accepted; several SAs

__device__ __forceinline__ void dcp_book(espgpu_insa *in, uint32_t sa, uint32_t bytes, uint32_t count) {
  atomicAdd(reinterpret_cast<unsigned long long *>(&in[sa].bytes), (unsigned long long)bytes);
  atomicAdd(reinterpret_cast<unsigned long long *>(&in[sa].packets), (unsigned long long)count);
}

__global__ __launch_bounds__(256) void dcp_kernel(DcpArgs a) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x, lane = threadIdx.x & 63u;
  uint32_t sa = 0, booked = 0;
  bool accepted = false;
  if (i < a.n) {
    const espgpu_pkt p = a.pkt[i];
    const espgpu_desc d = a.desc[i];
    const uint32_t tr = a.trailer[i];
    espgpu_pkt r = {p.off4, 0};
    int st = 0;
    if (a.status[i] == 0) {
      st = ESPGPU_EINVAL;
      espgpu_eshape s;
      if (d.sa < a.nin && d.sa < a.nsas &&
          esp_shape_of(a.sas[d.sa].mode, a.sas[d.sa].calg, a.sas[d.sa].mlen, 0, &s)) {
        // a descriptor that is not off4's own gives a skip the rule refuses
        // (up to 15 header dwords and a NAT-T SA's two UDP dwords)
        const uint32_t d4 = d.off4 - p.off4, skip = d4 < 18 ? d4 * 4 : ~0u;
        const size_t at = (size_t)p.off4 * 4;
        DecapPlan pl;
        st = esp_decap_rule(a.in[d.sa].flags, s.ivlen, s.alen, a.arena + at, a.out + at, skip, d.len, tr, &pl);
        if (st == 0) {
          r.off4 = p.off4 + pl.off / 4;
          r.len = pl.len;
          sa = d.sa;
          booked = pl.len;
          accepted = true;
        }
      }
    }
    a.ipkt[i] = r;
    a.dstatus[i] = (uint8_t)st;
  }
  // key_sa_recordxfer.  Each wave first sums its leading SA (the SA of its
  // first accepted lane); when that covers every accepted lane of every wave
  // of the workgroup, one lane adds for all 256 records.
  __shared__ uint32_t s_sa[4], s_bytes[4], s_count[4];
  const uint32_t wave = threadIdx.x >> 6;
  unsigned long long m = __ballot(accepted);
  const uint32_t lead = m ? (uint32_t)__ffsll((long long)m) - 1 : 0u;
  const uint32_t lsa = __shfl(sa, lead);
  const bool mine = accepted && sa == lsa;
  const unsigned long long mm = __ballot(mine);
  const uint32_t bytes = wave_sum(mine ? booked : 0u);         // 64 lanes of < 2^17 each
  const uint32_t count = (uint32_t)__popcll(mm);
  if (lane == 0) {
    s_sa[wave] = m == 0 ? kDcpNone : mm == m ? lsa : kDcpMixed;
    s_bytes[wave] = bytes;
    s_count[wave] = count;
  }
  __syncthreads();
  uint32_t wsa = kDcpNone, wbytes = 0, wcount = 0;
  bool one = true;
  for (uint32_t w = 0; w < 4; ++w) {
    const uint32_t v = s_sa[w];
    if (v == kDcpNone) continue;
    if (v == kDcpMixed || (wsa != kDcpNone && v != wsa)) one = false;
    wsa = v;
    wbytes += s_bytes[w];
    wcount += s_count[w];
  }
  if (one) {
    if (threadIdx.x == 0 && wsa != kDcpNone) dcp_book(a.in, wsa, wbytes, wcount);
    return;
  }
  // otherwise per wave: the leading SA is summed already, then the loop over
  // the other distinct SAs among the accepted lanes
  if (m == 0) return;
  if (lane == lead) dcp_book(a.in, lsa, bytes, count);
  m &= ~mm;
  while (m) {
    const uint32_t ld = (uint32_t)__ffsll((long long)m) - 1;
    const uint32_t nsa = __shfl(sa, ld);
    const bool hit = accepted && sa == nsa;
    const unsigned long long hm = __ballot(hit);
    const uint32_t b = wave_sum(hit ? booked : 0u);
    if (lane == ld) dcp_book(a.in, nsa, b, (uint32_t)__popcll(hm));
    m &= ~hm;
  }
}

}  // namespace

int launch_esp_decap(const uint8_t *arena, uint8_t *out, const espgpu_pkt *pkt, const espgpu_desc *desc,
                     const uint32_t *trailer, const uint8_t *status, uint32_t n, espgpu_insa *in, uint32_t nin,
                     const DevSA *sas, uint32_t nsas, espgpu_pkt *ipkt, uint8_t *dstatus, void *stream) {
  if (n == 0) return 0;
  const DcpArgs a = {arena, out, pkt, desc, trailer, status, in, sas, ipkt, dstatus, n, nin, nsas};
  hipLaunchKernelGGL(dcp_kernel, dim3((n + 255) / 256), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), a);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace espgpu
