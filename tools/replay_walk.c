/* The host side of tools/replay_bench.py's comparison: the serial walk a
 * caller of the batch path needs without espgpu_replay_update_batch, i.e.
 * espgpu_replay_update for every authenticated record in arrival order on
 * one core.  Built by the bench into a shared object next to libespgpu.so. */
#include <stdint.h>

#include "espgpu.h"

uint32_t replay_walk(struct espgpu_replay *tab, uint32_t ntab, uint32_t *bitmap,
                     const struct espgpu_desc *desc, const uint32_t *seq, const uint8_t *status,
                     uint8_t *ustatus, uint32_t n)
{
	uint32_t refused = 0;
	for (uint32_t i = 0; i < n; i++) {
		ustatus[i] = 0;
		if (status[i] != 0 || desc[i].sa >= ntab || desc[i].len < 8)
			continue;
		ustatus[i] = (uint8_t)espgpu_replay_update(&tab[desc[i].sa], bitmap, seq[i]);
		refused += ustatus[i] != 0;
	}
	return refused;
}
