/* The host side of tools/ah_out_bench.py: espgpu_ah_encap, espgpu_ah_frame and
 * espgpu_ah_sent per packet on one core, with the batch stages' rules for who
 * takes part.  The packets themselves stay on the device; the host has the
 * first HDR bytes of each packet's span (the headroom the AH header opens into
 * and the IP header behind it; 64 for the 28 bytes of headroom and the 20-byte
 * headers measured), its espgpu_pkt, SA id, descriptor and status byte.  A
 * span starts `room` bytes before its cleartext packet, at a 4-byte offset
 * base4[i] of the arena.  mlens[sa] == 0 marks a session the ctx does not hold
 * as a DIGEST one.  Each returns the packets accepted. */
#include "espgpu.h"

#define HDR 64

uint32_t
ah_encap_walk(const struct espgpu_encsa *enc, uint32_t nenc, const uint32_t *mlens, uint8_t *hdrs,
    const struct espgpu_pkt *pkt, const uint16_t *sa, uint32_t n, uint32_t room, uint32_t id0, uint8_t *hsave,
    struct espgpu_desc *desc, struct espgpu_pkt *opkt, uint8_t *estatus)
{
	uint32_t ok = 0;

	for (uint32_t i = 0; i < n; i++) {
		uint32_t s = sa[i], front = 0, total = 0, salt = 0;
		int rc = ESPGPU_EINVAL;

		if (s < nenc && mlens[s] != 0)
			rc = espgpu_ah_encap(&enc[s], mlens[s], hdrs + (size_t)i * HDR + room, pkt[i].len, room,
			    (uint16_t)(id0 + i), hsave + (size_t)i * HDR, &front, &total, &salt);
		desc[i].off4 = opkt[i].off4 = pkt[i].off4 - front / 4;
		desc[i].len = (uint16_t)total;
		desc[i].sa = rc == 0 ? (uint16_t)s : 0xffff;
		desc[i].esn_hi = 0;
		desc[i].salt = salt;
		opkt[i].len = total;
		estatus[i] = (uint8_t)rc;
		ok += rc == 0;
	}
	return ok;
}

/* in index order, which is each SA's arrival order */
uint32_t
ah_frame_walk(struct espgpu_outsa *out, uint32_t nout, const uint32_t *mlens, uint8_t *hdrs,
    const uint32_t *base4, struct espgpu_desc *desc, uint32_t n, uint8_t *fstatus)
{
	uint32_t ok = 0;

	for (uint32_t i = 0; i < n; i++) {
		uint32_t s = desc[i].sa;
		int rc = ESPGPU_EINVAL;

		if (desc[i].len != 0 && s < nout && mlens[s] != 0)
			rc = espgpu_ah_frame(&out[s], hdrs + (size_t)i * HDR + (size_t)(desc[i].off4 - base4[i]) * 4,
			    desc[i].len, desc[i].salt, &desc[i].esn_hi);
		if (rc != 0)
			desc[i].len = 0;
		fstatus[i] = (uint8_t)rc;
		ok += rc == 0;
	}
	return ok;
}

uint32_t
ah_sent_walk(struct espgpu_encsa *enc, uint32_t nenc, const uint32_t *mlens, uint8_t *hdrs, const uint32_t *base4,
    const struct espgpu_pkt *opkt, const struct espgpu_desc *desc, const uint8_t *status, uint32_t n,
    const uint8_t *hsave, uint8_t *sstatus)
{
	uint32_t ok = 0;

	for (uint32_t i = 0; i < n; i++) {
		uint32_t s = desc[i].sa;
		int rc = 0;

		if (status[i] == 0 && s < nenc && mlens[s] != 0) {
			rc = espgpu_ah_sent(&enc[s], 0, hdrs + (size_t)i * HDR + (size_t)(opkt[i].off4 - base4[i]) * 4,
			    opkt[i].len, desc[i].salt, hsave + (size_t)i * HDR);
			ok += rc == 0;
		}
		sstatus[i] = (uint8_t)rc;
	}
	return ok;
}
