/* The host side of tools/frame_bench.py: espgpu_esp_frame per record in
 * arrival order on one core.  The records themselves stay on the device, so
 * each is framed in a scratch buffer and the bytes the rule wrote -- up to 16
 * of header and IV, up to 17 of padding and trailer -- are gathered into a
 * 40-byte slot per record for the copy up.  Returns the records refused. */
#include <string.h>

#include "espgpu.h"

#define SLOT 40

uint32_t
frame_walk(struct espgpu_outsa *out, uint32_t nout, const struct espgpu_eshape *shapes,
    struct espgpu_desc *desc, const uint32_t *frame, uint8_t *stage, uint8_t *fstatus, uint32_t n)
{
	static uint8_t rec[65536 + 64];
	uint32_t refused = 0;

	for (uint32_t i = 0; i < n; i++) {
		struct espgpu_desc *d = &desc[i];
		const uint32_t rlen = frame[i] & 0xffff;
		uint32_t hi = 0;
		int rc = ESPGPU_EINVAL;

		if (d->sa < nout)
			rc = espgpu_esp_frame(&out[d->sa], &shapes[d->sa], rec, d->len, rlen,
			    (uint8_t)(frame[i] >> 16), &hi);
		fstatus[i] = (uint8_t)rc;
		if (rc != 0) {
			d->len = 0;
			refused++;
			continue;
		}
		const struct espgpu_eshape *s = &shapes[d->sa];
		const uint32_t hlen = 8 + s->ivlen;

		d->esn_hi = hi;
		if (s->ivlen == 8)
			d->salt = out[d->sa].salt;
		memcpy(stage + (size_t)i * SLOT, rec, hlen < 16 ? hlen : 16);
		memcpy(stage + (size_t)i * SLOT + 16, rec + hlen + rlen, d->len - hlen - rlen - s->alen);
	}
	return refused;
}
