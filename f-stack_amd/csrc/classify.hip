// classify.hip — step 0 of the inbound sequence on a device-resident batch
// (include/espgpu.h, the classification block): from received packets in the
// arena to the espgpu_desc that the replay check, the decrypt kernels and the
// window update take.  ip_input's header sanity, ipsec_common_input's SPI
// lookup and esp_input's alignment checks for every packet in parallel; the
// rule itself is classify.h's, shared with espgpu_esp_classify on the host.
//
// One lane per packet, no LDS, no workspace.  A packet costs its 8-byte
// espgpu_pkt, five header dwords (IPv6: four more for the destination; IPv4
// options only under ESPGPU_CLS_IPCSUM), the SPI dword, and per probed slot
// one 16-byte load, plus the slot's dst half once the SPI matched.  At an
// MTU-sized stride every lane's header is a cache line of its own whatever
// the lane mapping, so the header loads go out together in one round and the
// SPI and the table follow; the table of a realistic SA set stays in L2.  The
// kernel reads the arena and the table and writes d_desc and d_cstatus.
#include <hip/hip_runtime.h>

#include "classify.h"
#include "espgpu_internal.h"

namespace espgpu {

namespace {

__global__ __launch_bounds__(256) void cls_kernel(const uint8_t *arena, const espgpu_pkt *pkt, uint32_t n,
                                                  const espgpu_sad_entry *table, uint32_t nslots, uint32_t flags,
                                                  espgpu_desc *desc, uint8_t *cstatus) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const espgpu_pkt p = pkt[i];
  espgpu_desc d;
  const int st = esp_classify_rule(table, nslots, arena + (size_t)p.off4 * 4, p.len, p.off4, flags, &d);
  desc[i] = d;
  cstatus[i] = (uint8_t)st;
}

}  // namespace

int launch_esp_classify(const uint8_t *arena, const espgpu_pkt *pkt, uint32_t n, const espgpu_sad_entry *table,
                        uint32_t nslots, uint32_t flags, espgpu_desc *desc, uint8_t *cstatus, void *stream) {
  if (n == 0) return 0;
  hipLaunchKernelGGL(cls_kernel, dim3((n + 255) / 256), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), arena,
                     pkt, n, table, nslots, flags, desc, cstatus);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace espgpu
