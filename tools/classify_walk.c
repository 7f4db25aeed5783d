/* The host side of tools/classify_bench.py: espgpu_esp_classify per packet
 * on one core.  The packets themselves stay on the device; the host has each
 * one's first HDR bytes (the rule reads the IP header and the SPI, at most 64
 * bytes of a packet, whatever its length).  Returns the packets accepted. */
#include "espgpu.h"

#define HDR 64

uint32_t
classify_walk(const struct espgpu_sad_entry *table, uint32_t nslots, const uint8_t *hdrs,
    const struct espgpu_pkt *pkt, uint32_t n, uint32_t flags, struct espgpu_desc *desc,
    uint8_t *cstatus)
{
	uint32_t ok = 0;

	for (uint32_t i = 0; i < n; i++) {
		int rc = espgpu_esp_classify(table, nslots, hdrs + (size_t)i * HDR, pkt[i].len,
		    pkt[i].off4, flags, &desc[i]);

		cstatus[i] = (uint8_t)rc;
		ok += rc == 0;
	}
	return ok;
}
