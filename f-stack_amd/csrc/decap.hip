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
// The SA counters are aggregated per wave and per workgroup before the 64-bit
// adds (sa_book.h, shared with the AH decapsulation).
#include <hip/hip_runtime.h>

#include "decap.h"
#include "dev_prims.h"
#include "espgpu_internal.h"
#include "frame.h"
#include "sa_book.h"

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

__global__ __launch_bounds__(256) void dcp_kernel(DcpArgs a) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
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
  sa_book_workgroup(a.in, sa, booked, accepted);   // key_sa_recordxfer
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
