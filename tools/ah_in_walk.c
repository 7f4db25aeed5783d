/* The host side of tools/ah_in_bench.py: espgpu_ah_input and espgpu_ah_decap
 * per packet on one core, with the batch stages' rules for who takes part.
 * The packets themselves stay on the device; the host has each one's first
 * HDR bytes (the IP header and the AH header the restored header moves over;
 * 64 for the 20-byte headers and the 28-byte AH header measured), its
 * descriptor and its status byte.  mlens[sa] == 0 marks a session the ctx does
 * not hold as a DIGEST one.  Each returns the packets accepted. */
#include "espgpu.h"

#define HDR 64

uint32_t
ah_input_walk(const struct espgpu_insa *in, uint32_t nin, const uint32_t *mlens, uint8_t *hdrs,
    struct espgpu_desc *desc, uint32_t n, uint8_t *hsave, uint8_t *astatus)
{
	uint32_t ok = 0;

	for (uint32_t i = 0; i < n; i++) {
		uint32_t sa = desc[i].sa;
		int rc = 0;

		if (desc[i].len != 0 && sa < nin && mlens[sa] != 0) {
			rc = espgpu_ah_input(&in[sa], mlens[sa], hdrs + (size_t)i * HDR, desc[i].len,
			    desc[i].salt, hsave + (size_t)i * HDR);
			if (rc != 0)
				desc[i].len = 0;
			ok += rc == 0;
		}
		astatus[i] = (uint8_t)rc;
	}
	return ok;
}

uint32_t
ah_decap_walk(struct espgpu_insa *in, uint32_t nin, const uint32_t *mlens, uint8_t *hdrs,
    const struct espgpu_desc *desc, const uint8_t *status, uint32_t n, const uint8_t *hsave,
    struct espgpu_pkt *ipkt, uint8_t *dstatus)
{
	uint32_t ok = 0;

	for (uint32_t i = 0; i < n; i++) {
		uint32_t sa = desc[i].sa, off = 0, len = 0;
		int rc = 0;

		if (status[i] == 0) {
			rc = ESPGPU_EINVAL;
			if (desc[i].len != 0 && sa < nin && mlens[sa] != 0)
				rc = espgpu_ah_decap(&in[sa], mlens[sa], hdrs + (size_t)i * HDR, desc[i].len,
				    desc[i].salt, hsave + (size_t)i * HDR, &off, &len);
			ok += rc == 0;
		}
		ipkt[i].off4 = desc[i].off4 + off / 4;
		ipkt[i].len = len;
		dstatus[i] = (uint8_t)rc;
	}
	return ok;
}
