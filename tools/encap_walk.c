/* The host side of tools/encap_bench.py: espgpu_esp_encap and espgpu_esp_sent
 * per packet on one core, with the batch entries' rules for who takes part.
 * The packets themselves stay on the device; the host has of each one the
 * SPAN bytes that start `headroom` bytes before it (the room the headers go
 * into and the packet's own header, at most 64 + 60 bytes), its espgpu_pkt and
 * its SA id.  shapes[sa].blks == 0 marks a session the ctx does not hold.
 * encap_walk returns the packets accepted, sent_walk the packets booked. */
#include "espgpu.h"

#define SPAN 128

uint32_t
encap_walk(const struct espgpu_encsa *enc, uint32_t nenc, const struct espgpu_eshape *shapes, uint8_t *spans,
    const struct espgpu_pkt *pkt, const uint16_t *sa, uint32_t n, uint32_t headroom, uint32_t tailroom, uint32_t id0,
    struct espgpu_desc *desc, uint32_t *frame, struct espgpu_pkt *opkt, uint8_t *estatus)
{
	uint32_t ok = 0;

	for (uint32_t i = 0; i < n; i++) {
		uint32_t s = sa[i], front = 0, total = 0, reclen = 0, f = 0;
		int rc = ESPGPU_EINVAL;

		if (s < nenc && shapes[s].blks != 0)
			rc = espgpu_esp_encap(&enc[s], &shapes[s], spans + (size_t)i * SPAN + headroom, pkt[i].len,
			    headroom, tailroom, (uint16_t)(id0 + i), &front, &total, &reclen, &f);
		desc[i].esn_hi = desc[i].salt = 0;
		if (rc == 0) {
			opkt[i].off4 = pkt[i].off4 - front / 4;
			opkt[i].len = total;
			desc[i].off4 = opkt[i].off4 + (total - reclen) / 4;
			desc[i].len = (uint16_t)reclen;
			desc[i].sa = (uint16_t)s;
			frame[i] = f;
			ok++;
		} else {
			opkt[i].off4 = desc[i].off4 = pkt[i].off4;
			opkt[i].len = 0;
			desc[i].len = 0;
			desc[i].sa = 0xffff;
		}
		estatus[i] = (uint8_t)rc;
	}
	return ok;
}

uint32_t
sent_walk(struct espgpu_encsa *enc, uint32_t nenc, const struct espgpu_pkt *opkt, const struct espgpu_desc *desc,
    const uint8_t *status, uint32_t n)
{
	uint32_t ok = 0;

	for (uint32_t i = 0; i < n; i++)
		if (desc[i].sa < nenc) {
			espgpu_esp_sent(&enc[desc[i].sa], status[i], opkt[i].len);
			ok += status[i] == 0;
		}
	return ok;
}
