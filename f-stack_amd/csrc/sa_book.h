// sa_book.h — key_sa_recordxfer for a workgroup of the kernels that close a
// direction (decap.hip dcp_kernel, ah_in.hip ahd_kernel, encap.hip snt_kernel,
// ah_out.hip ahs_kernel): every accepted lane's bytes and one packet into its
// SA's lifetime counters, espgpu_insa's inbound and espgpu_encsa's outbound.
//
// The counters are aggregated per wave: for each distinct SA among the
// accepted lanes (ballot, the first such lane's SA broadcast, the matching
// lanes' bytes summed across the wave) one lane issues one 64-bit add pair.
// Same-address adds serialise at about 13 ns each, so on top of that a
// workgroup whose accepted records all belong to one SA adds once for its four
// waves, through 48 bytes of LDS: a one-SA batch puts n / 256 adds on an
// address, not n (profiles/esp_decap_batch.txt).  All of it runs with every
// lane of the wave on: the conditions are ballots or workgroup-uniform, no
// lane returns before the barrier, and the shuffles stand outside every
// lane-dependent branch.
#pragma once
#include <hip/hip_runtime.h>

#include "dev_prims.h"
#include "espgpu.h"

namespace espgpu {

namespace {

constexpr uint32_t kBookNone = 0xfffffffeu, kBookMixed = 0xffffffffu;   // a wave's SA: no lane accepted; several SAs

template <class SA>
__device__ __forceinline__ void sa_book(SA *sas, uint32_t sa, uint32_t bytes, uint32_t count) {
  atomicAdd(reinterpret_cast<unsigned long long *>(&sas[sa].bytes), (unsigned long long)bytes);
  atomicAdd(reinterpret_cast<unsigned long long *>(&sas[sa].packets), (unsigned long long)count);
}

// Called by every thread of a 256-thread workgroup, as the last thing the
// kernel does: `accepted` lanes book `booked` bytes (< 2^17) into sas[sa].
// Each wave first sums its leading SA (the SA of its first accepted lane);
// when that covers every accepted lane of every wave of the workgroup, one
// lane adds for all 256 records.
template <class SA>
__device__ __forceinline__ void sa_book_workgroup(SA *sas, uint32_t sa, uint32_t booked, bool accepted) {
  __shared__ uint32_t s_sa[4], s_bytes[4], s_count[4];
  const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
  unsigned long long m = __ballot(accepted);
  const uint32_t lead = m ? (uint32_t)__ffsll((long long)m) - 1 : 0u;
  const uint32_t lsa = __shfl(sa, lead);
  const bool mine = accepted && sa == lsa;
  const unsigned long long mm = __ballot(mine);
  const uint32_t bytes = wave_sum(mine ? booked : 0u);         // 64 lanes of < 2^17 each
  const uint32_t count = (uint32_t)__popcll(mm);
  if (lane == 0) {
    s_sa[wave] = m == 0 ? kBookNone : mm == m ? lsa : kBookMixed;
    s_bytes[wave] = bytes;
    s_count[wave] = count;
  }
  __syncthreads();
  uint32_t wsa = kBookNone, wbytes = 0, wcount = 0;
  bool one = true;
  for (uint32_t w = 0; w < 4; ++w) {
    const uint32_t v = s_sa[w];
    if (v == kBookNone) continue;
    if (v == kBookMixed || (wsa != kBookNone && v != wsa)) one = false;
    wsa = v;
    wbytes += s_bytes[w];
    wcount += s_count[w];
  }
  if (one) {
    if (threadIdx.x == 0 && wsa != kBookNone) sa_book(sas, wsa, wbytes, wcount);
    return;
  }
  // otherwise per wave: the leading SA is summed already, then the loop over
  // the other distinct SAs among the accepted lanes (m is wave-uniform)
  if (m == 0) return;
  if (lane == lead) sa_book(sas, lsa, bytes, count);
  m &= ~mm;
  while (m) {
    const uint32_t ld = (uint32_t)__ffsll((long long)m) - 1;
    const uint32_t nsa = __shfl(sa, ld);
    const bool hit = accepted && sa == nsa;
    const unsigned long long hm = __ballot(hit);
    const uint32_t b = wave_sum(hit ? booked : 0u);
    if (lane == ld) sa_book(sas, nsa, b, (uint32_t)__popcll(hm));
    m &= ~hm;
  }
}

}  // namespace

}  // namespace espgpu
