// frame.hip — the outbound framing of a device-resident batch before encrypt:
// espgpu_esp_frame_batch (include/espgpu.h); the rule of one
// record is frame.h's, shared with espgpu_esp_frame on the host, and the five
// numbering steps are sa_group.h's, shared with the outbound AH (ah_out.hip).
// With room = esp_out_room(count0), the records of rank < room are accepted
// and get count0 + rank + 1 and cntr0 + rank; the SA ends at count0 + m,
// cntr0 + m, m = min(k, room).
#include <hip/hip_runtime.h>

#include "espgpu_internal.h"
#include "frame.h"
#include "sa_group.h"

namespace espgpu {

namespace {

// esp_output's numbering rule for sa_group.h's steps.
struct FrmRule {
  uint8_t *arena;
  const uint32_t *frame;
  const DevSA *sas;
  uint32_t nsas;

  static constexpr uint8_t kNoRoom = ESPGPU_EINVAL;

  __device__ bool shape(uint32_t sa, uint32_t oflags, espgpu_eshape *s) const {
    const DevSA &d = sas[sa];
    return esp_shape_of(d.mode, d.calg, d.mlen, oflags, s);
  }
  __device__ bool takes(const espgpu_desc &d, uint32_t i, const espgpu_outsa *o) const {
    const uint32_t rlen = frame[i] & 0xffffu;
    espgpu_eshape s;
    return d.sa < nsas && shape(d.sa, o->flags, &s) &&
           8 + s.ivlen + rlen + esp_padding(rlen, s.blks) + s.alen == (uint32_t)d.len;
  }
  __device__ uint64_t room(const espgpu_outsa &o) const { return esp_out_room(o.count, o.flags); }
  // the record's number and IV from its rank, then the bytes esp_output writes
  __device__ void write(espgpu_desc *d, uint32_t i, uint32_t key, const espgpu_outsa &o, uint32_t rank) const {
    espgpu_eshape s;
    if (!shape(key, o.flags, &s)) return;              // (takes() accepted it)
    const uint64_t count = o.count + rank + 1;
    const uint32_t f = frame[i];
    esp_frame_write(arena + (size_t)d->off4 * 4, s, o.flags, o.spi, count, o.cntr + rank, f & 0xffffu,
                    (uint8_t)(f >> 16));
    d->esn_hi = (o.flags & ESPGPU_OUT_ESN) ? (uint32_t)(count >> 32) : 0u;
    if (s.ivlen == 8) d->salt = o.salt;
  }
  __device__ void commit(espgpu_outsa *dst, const espgpu_outsa &o, uint32_t key, uint64_t m) const {
    espgpu_eshape s;
    if (!shape(key, o.flags, &s)) return;
    dst->count = o.count + m;
    if (s.ivlen == 8) dst->cntr = o.cntr + m;
  }
};

}  // namespace

size_t esp_frame_workspace_bytes(uint32_t n, uint32_t nout) { return num_workspace_bytes(n, nout); }

int launch_esp_frame(uint8_t *arena, espgpu_desc *desc, const uint32_t *frame, uint32_t n, espgpu_outsa *out,
                     uint32_t nout, const DevSA *sas, uint32_t nsas, uint8_t *fstatus, void *ws, void *stream) {
  const FrmRule r = {arena, frame, sas, nsas};
  return num_batch(r, desc, n, out, nout, fstatus, ws, reinterpret_cast<hipStream_t>(stream));
}

}  // namespace espgpu
