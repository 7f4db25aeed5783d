// ah_in.hip — steps 1 and 6 of the inbound AH sequence on a device-resident
// batch (include/espgpu.h, the inbound AH block): ah_input's header-length
// checks and ah_massage_headers in front of the digest kernel, and
// ah_input_cb's restore and strip with ipsec4/6_common_input_cb and
// key_sa_recordxfer behind it, for every record in parallel.  The rules are
// ah_in.h's, shared with espgpu_ah_input and espgpu_ah_decap on the host.
//
// Both kernels: one lane per packet, no workspace.
//
// ahi_kernel reads a record's descriptor, its SA's flags and its session's
// mode and mlen (L2), the packet's first dword and the AH header's, then the
// header: 5 dwords (IPv4 without options), 10 (IPv6) or up to 15.  It stores
// them to the save slot as they came and massaged over the packet.  The IPv4
// option loop is byte-serial and lane-dependent, so a wave runs it only if a
// ballot finds a lane whose header is longer than 20 bytes; the common wave
// takes the 10-dword instantiation of the rule, which has no loop in it.  The
// loop reads the option bytes from the packet (they are in L1 by then: the
// header's dwords were just loaded) and leaves a 40-bit mask of the bytes to
// zero, which constant-index code applies to the registers: the header is
// never indexed by a variable, so neither path needs scratch.  No LDS, no
// barrier, no shuffle; the ballot stands where every lane of the wave reaches
// it, lanes past n included.
//
// ahd_kernel reads the descriptor, the status byte, the SA's flags, the
// session's mode and mlen and the AH header's first dword.  A tunnel record
// never touches its packet or its save slot; a transport record loads its
// 5-15 saved dwords into registers and stores them, fixed, ahsize bytes into
// the packet.  The counters go through sa_book.h, as dcp_kernel's: no lane
// returns before its barrier.
#include <hip/hip_runtime.h>

#include "ah_in.h"
#include "espgpu_internal.h"
#include "sa_book.h"

namespace espgpu {

namespace {

struct AhiArgs {
  uint8_t *arena;
  espgpu_desc *desc;
  const espgpu_insa *in;
  const DevSA *sas;
  uint8_t *hsave;
  uint8_t *astatus;
  uint32_t n, nin, nsas;
};

__global__ __launch_bounds__(256) void ahi_kernel(AhiArgs a) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  bool takes = false, go = false;
  uint32_t flags = 0, salt = 0;
  uint8_t *pkt = nullptr;
  int st = 0;
  if (i < a.n) {
    const espgpu_desc d = a.desc[i];
    if (d.len != 0 && d.sa < a.nin && d.sa < a.nsas && a.sas[d.sa].mode == ESPGPU_CSP_MODE_DIGEST) {
      takes = true;
      flags = a.in[d.sa].flags;
      salt = d.salt;
      pkt = a.arena + (size_t)d.off4 * 4;
      st = ah_in_plan(flags, a.sas[d.sa].mlen, pkt, d.len, salt);
      go = st == 0;
    }
  }
  // after the plan: skip is 20..60 (IPv4) or 40 (IPv6)
  const bool opts = go && !(flags & ESPGPU_IN_AF6) && salt > 32;
  uint8_t *const slot = a.hsave + (size_t)i * kAhSaveSlot;
  if (__ballot(opts)) {
    if (go) st = ah_in_massage<15>(flags, pkt, salt - 12, slot);
  } else {
    if (go) st = ah_in_massage<10>(flags, pkt, salt - 12, slot);
  }
  if (i < a.n) {
    if (takes && st) a.desc[i].len = 0;
    a.astatus[i] = (uint8_t)st;
  }
}

struct AhdArgs {
  uint8_t *arena;
  const espgpu_desc *desc;
  const uint8_t *status;
  espgpu_insa *in;
  const DevSA *sas;
  const uint8_t *hsave;
  espgpu_pkt *ipkt;
  uint8_t *dstatus;
  uint32_t n, nin, nsas;
};

__global__ __launch_bounds__(256) void ahd_kernel(AhdArgs a) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  uint32_t sa = 0, booked = 0;
  bool accepted = false;
  if (i < a.n) {
    const espgpu_desc d = a.desc[i];
    espgpu_pkt r = {d.off4, 0};
    int st = 0;
    bool write = true;
    if (a.status[i] == 0) {
      st = ESPGPU_EINVAL;
      const uint32_t mode = d.sa < a.nsas ? a.sas[d.sa].mode : 0u;
      if (mode == ESPGPU_CSP_MODE_DIGEST) {
        if (d.sa < a.nin && d.len != 0) {
          DecapPlan pl;
          st = ah_decap_rule(a.in[d.sa].flags, a.sas[d.sa].mlen, a.arena + (size_t)d.off4 * 4, d.len, d.salt,
                             a.hsave + (size_t)i * kAhSaveSlot, &pl);
          if (st == 0) {
            r.off4 = d.off4 + pl.off / 4;
            r.len = pl.len;
            sa = d.sa;
            booked = pl.len;
            accepted = true;
          }
        }
      } else if (mode != 0) {
        // an ESP session's record: espgpu_esp_decap_batch's
        st = 0;
        write = false;
      }
    }
    if (write) a.ipkt[i] = r;
    a.dstatus[i] = (uint8_t)st;
  }
  sa_book_workgroup(a.in, sa, booked, accepted);   // key_sa_recordxfer
}

}  // namespace

int launch_ah_input(uint8_t *arena, espgpu_desc *desc, uint32_t n, const espgpu_insa *in, uint32_t nin,
                    const DevSA *sas, uint32_t nsas, uint8_t *hsave, uint8_t *astatus, void *stream) {
  if (n == 0) return 0;
  const AhiArgs a = {arena, desc, in, sas, hsave, astatus, n, nin, nsas};
  hipLaunchKernelGGL(ahi_kernel, dim3((n + 255) / 256), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), a);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

int launch_ah_decap(uint8_t *arena, const espgpu_desc *desc, const uint8_t *status, uint32_t n, espgpu_insa *in,
                    uint32_t nin, const DevSA *sas, uint32_t nsas, const uint8_t *hsave, espgpu_pkt *ipkt,
                    uint8_t *dstatus, void *stream) {
  if (n == 0) return 0;
  const AhdArgs a = {arena, desc, status, in, sas, hsave, ipkt, dstatus, n, nin, nsas};
  hipLaunchKernelGGL(ahd_kernel, dim3((n + 255) / 256), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), a);
  return hipGetLastError() == hipSuccess ? 0 : -1;
}

}  // namespace espgpu
