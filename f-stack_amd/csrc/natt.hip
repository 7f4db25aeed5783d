// natt.hip — step 5b of the inbound sequence on a device-resident batch
// (include/espgpu.h, the NAT-T block): udp_ipsec_adjust_cksum for every
// decapsulated transport packet of a NAT-T SA in parallel; the rule itself is
// natt.h's, shared with espgpu_esp_natt_cksum on the host.
//
// ntc_auto_kernel (policy 0): one lane per packet, no LDS, no workspace.  A
// packet costs the dense arrays (status bytes, espgpu_pkt, SA id, trailer
// word), its SA's flags and delta from L2, the IP header's first dword and
// the dword that holds the checksum field.
//
// ntc_sum_kernel (policy != 0) reads every byte of every taking-part packet's
// segment: a group of kNattLanes lanes per packet.  Per group step each lane
// loads four dwords, dword j of lane g at index step * 4 * L + j * L + g, so
// one load instruction of a group covers 4 * L contiguous bytes and a group
// step 16 * L (256 for L = 16); a wave works on 64 / L packets.  The segment
// starts 4-byte aligned (off4, ip_hl * 4), every load is an aligned dword that
// holds at least one byte of the span, and the last one is masked.  The loop's
// trip count depends on the packet, so nothing cross-lane stands inside it: a
// lane whose packet takes no part, or that is past n, runs it zero times and
// stays on, and the shuffles that add the group's sums stand behind it with
// every lane of the wave on (a shuffle read of a switched-off lane returns
// 0: DESIGN.md 3.2).  Lane 0 of the group then stores the field's dword.
// L = 16 was chosen unmeasured; the runs of tools/natt_bench.py since are in
// DESIGN.md 3.10.
#include <hip/hip_runtime.h>

#include "espgpu_internal.h"
#include "natt.h"

namespace espgpu {

namespace {

struct NtcArgs {
  uint8_t *out;
  const espgpu_pkt *ipkt;
  const espgpu_desc *desc;
  const uint32_t *trailer;
  const uint8_t *status;
  const uint8_t *dstatus;
  const espgpu_insa *in;
  uint8_t *cflags;
  uint32_t n, nin;
};

// Does packet i take part?  Then its bytes, length, protocol and SA delta.
__device__ __forceinline__ bool ntc_takes_part(const NtcArgs &a, uint32_t i, uint8_t **pkt, uint32_t *len,
                                               uint32_t *proto, uint32_t *delta) {
  if (a.status[i] != 0 || a.dstatus[i] != 0) return false;
  const uint32_t nxt = a.trailer[i] & 0xffu;
  if (nxt != 6 && nxt != 17) return false;             // ipsec_input.c:318; never a tunnel result
  const uint32_t sa = a.desc[i].sa;
  if (sa >= a.nin) return false;
  if (!(a.in[sa].flags & ESPGPU_IN_NATT)) return false;
  const espgpu_pkt p = a.ipkt[i];
  *pkt = a.out + (size_t)p.off4 * 4;
  *len = p.len;
  *proto = nxt;
  *delta = a.in[sa].natt_cksum;
  return true;
}

__global__ __launch_bounds__(256) void ntc_auto_kernel(NtcArgs a) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= a.n) return;
  uint8_t *pkt;
  uint32_t len, proto, delta, cf = 0;
  NattPlan p;
  if (ntc_takes_part(a, i, &pkt, &len, &proto, &delta) && natt_plan(pkt, len, proto, 0, &p))
    cf = natt_auto(pkt, p, delta);
  if (a.cflags) a.cflags[i] = (uint8_t)cf;
}

template <uint32_t L>
__global__ __launch_bounds__(256) void ntc_sum_kernel(NtcArgs a) {
  const uint32_t t = blockIdx.x * blockDim.x + threadIdx.x, i = t / L, g = t % L;
  uint8_t *pkt = nullptr;
  uint32_t len, proto, delta;
  NattPlan p;
  p.cklen = 0;
  p.ihl = 0;
  bool part = false;
  if (i < a.n) part = ntc_takes_part(a, i, &pkt, &len, &proto, &delta) && natt_plan(pkt, len, proto, 1, &p);
  const uint32_t nd = part ? (p.cklen + 3) / 4 : 0u;   // dwords with a byte of the span
  const uint8_t *seg = pkt + p.ihl;
  const uint32_t nfull = part ? p.cklen / 4 : 0u;      // dwords that lie in the span whole
  uint64_t acc = 0;
  uint32_t base = 0;
  // whole group steps: four whole dwords per lane, loaded without a condition so that they go out together
#pragma unroll 2
  for (; base + 4 * L <= nfull; base += 4 * L) {
    uint32_t w[4];
#pragma unroll
    for (uint32_t j = 0; j < 4; ++j) w[j] = mem_ld32(seg + 4 * (base + j * L + g));
    acc += (uint64_t)w[0] + w[1] + w[2] + w[3];
  }
  // the last step: at most 4 * L dwords are left (nd <= nfull + 1), the last of them masked
#pragma unroll
  for (uint32_t j = 0; j < 4; ++j) {
    const uint32_t k = base + j * L + g;
    if (k < nd) acc += natt_dword(seg, k, p.cklen);
  }
  // at most 2^14 dwords per lane: 18 bits after the fold, 22 after the group's sum
  acc = (acc & 0xffffffffu) + (acc >> 32);
  uint32_t s = (uint32_t)((acc & 0xffffu) + ((acc >> 16) & 0xffffu) + (acc >> 32));
  // every lane of the wave is on here; xor distances below L stay inside the group
#pragma unroll
  for (uint32_t d = L / 2; d > 0; d >>= 1) s += __shfl_xor(s, d);
  if (g == 0 && i < a.n) {
    if (part) natt_finish(pkt, p, s);
    if (a.cflags) a.cflags[i] = 0;
  }
}

}  // namespace

int launch_esp_natt_cksum(uint8_t *out, const espgpu_pkt *ipkt, const espgpu_desc *desc, const uint32_t *trailer,
                          const uint8_t *status, const uint8_t *dstatus, uint32_t n, const espgpu_insa *in,
                          uint32_t nin, uint32_t policy, uint32_t lanes, uint8_t *cflags, void *stream) {
  if (n == 0) return 0;
  const NtcArgs a = {out, ipkt, desc, trailer, status, dstatus, in, cflags, n, nin};
  hipStream_t st = reinterpret_cast<hipStream_t>(stream);
  if (policy == 0) {
    hipLaunchKernelGGL(ntc_auto_kernel, dim3((n + 255) / 256), dim3(256), 0, st, a);
  } else {
    const uint32_t L = lanes ? lanes : kNattLanes;
    const dim3 grid((uint32_t)(((uint64_t)n * L + 255) / 256));
    if (L == 8)
      hipLaunchKernelGGL(ntc_sum_kernel<8>, grid, dim3(256), 0, st, a);
    else if (L == 16)
      hipLaunchKernelGGL(ntc_sum_kernel<16>, grid, dim3(256), 0, st, a);
    else if (L == 32)
      hipLaunchKernelGGL(ntc_sum_kernel<32>, grid, dim3(256), 0, st, a);
    else
      return -1;
  }
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace espgpu
