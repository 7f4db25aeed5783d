/* The host side of tools/decap_bench.py: espgpu_esp_decap per packet on one
 * core, with espgpu_esp_decap_batch's rules for who takes part.  The packets
 * themselves stay on the device; the host has each one's first HDR bytes (the
 * outer header and the ESP header and IV it moves over, at most 60 + 24
 * bytes; 64 for the 20-byte headers measured), its descriptor, status byte and
 * trailer word.  shapes[sa].blks == 0 marks a session the ctx does not hold.
 * Returns the packets accepted. */
#include "espgpu.h"

#define HDR 64

uint32_t
decap_walk(struct espgpu_insa *in, uint32_t nin, const struct espgpu_eshape *shapes, uint8_t *hdrs,
    const struct espgpu_pkt *pkt, const struct espgpu_desc *desc, const uint32_t *trailer,
    const uint8_t *status, uint32_t n, struct espgpu_pkt *ipkt, uint8_t *dstatus)
{
	uint32_t ok = 0;

	for (uint32_t i = 0; i < n; i++) {
		uint32_t sa = desc[i].sa, off = 0, len = 0;
		int rc = 0;

		if (status[i] == 0) {
			rc = ESPGPU_EINVAL;
			if (sa < nin && shapes[sa].blks != 0)
				rc = espgpu_esp_decap(&in[sa], &shapes[sa], hdrs + (size_t)i * HDR,
				    (desc[i].off4 - pkt[i].off4) * 4, desc[i].len, trailer[i], &off, &len);
			ok += rc == 0;
		}
		ipkt[i].off4 = pkt[i].off4 + off / 4;
		ipkt[i].len = len;
		dstatus[i] = (uint8_t)rc;
	}
	return ok;
}
