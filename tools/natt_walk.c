/* The host side of tools/natt_bench.py: espgpu_esp_natt_cksum per packet on
 * one core, with espgpu_esp_natt_cksum_batch's rules for who takes part.  The
 * recompute policy reads every segment byte, so the whole arena is on the
 * host here.  Returns the packets whose SA has ESPGPU_IN_NATT. */
#include "espgpu.h"

uint32_t
natt_walk(const struct espgpu_insa *in, uint32_t nin, uint8_t *arena, const struct espgpu_pkt *ipkt,
    const struct espgpu_desc *desc, const uint32_t *trailer, const uint8_t *status, const uint8_t *dstatus,
    uint32_t n, uint32_t policy, uint8_t *cflags)
{
	uint32_t took = 0;

	for (uint32_t i = 0; i < n; i++) {
		uint32_t sa = desc[i].sa;

		cflags[i] = 0;
		if (status[i] != 0 || dstatus[i] != 0 || sa >= nin)
			continue;
		took += (in[sa].flags & ESPGPU_IN_NATT) != 0;
		espgpu_esp_natt_cksum(&in[sa], arena + (size_t)ipkt[i].off4 * 4, ipkt[i].len, trailer[i], policy,
		    &cflags[i]);
	}
	return took;
}
