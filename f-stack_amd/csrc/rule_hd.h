// rule_hd.h — what the rule headers (classify.h, decap.h, encap.h, frame.h, replay.h,
// ah_in.h, ah_out.h, natt.h, ip_hdr.h) share: the marker that makes one function serve the host entry point and the
// kernel, and a packet dword in memory order.  Plain C++ with no HIP header.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define ESPGPU_HD __host__ __device__
#else
#define ESPGPU_HD
#endif

namespace espgpu {

// A dword of the packet in memory order (byte k in bits 8k..8k+7).  The device
// accesses it whole: headers and records are 4-byte aligned there by off4.  The
// host goes byte by byte, from wherever the caller's buffer starts.
ESPGPU_HD inline uint32_t mem_ld32(const uint8_t *p) {
#ifdef __HIP_DEVICE_COMPILE__
  return *reinterpret_cast<const uint32_t *>(p);
#else
  return (uint32_t)p[0] | (uint32_t)p[1] << 8 | (uint32_t)p[2] << 16 | (uint32_t)p[3] << 24;
#endif
}
ESPGPU_HD inline void mem_st32(uint8_t *p, uint32_t v) {
#ifdef __HIP_DEVICE_COMPILE__
  *reinterpret_cast<uint32_t *>(p) = v;
#else
  p[0] = (uint8_t)v;
  p[1] = (uint8_t)(v >> 8);
  p[2] = (uint8_t)(v >> 16);
  p[3] = (uint8_t)(v >> 24);
#endif
}

}  // namespace espgpu
