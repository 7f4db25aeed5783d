// replay.h — the replay window rules (include/espgpu.h, the replay block):
// what makes a window usable and where a sequence number's bit lies, for the
// host functions and the kernels (replay.hip) alike, and the two host update
// rules behind espgpu_replay_update / espgpu_replay_update64.
//
// Plain C++ with no HIP header, as classify.h and decap.h: the host side also
// builds with the host compiler alone.
#pragma once
#include <stdint.h>

#include "espgpu.h"
#include "rule_hd.h"

namespace espgpu {

// The window indexes the bitmap with bitmap_size - 1 as a mask: a power of
// two covering wsize * 8 bits (key.c:3346-3351 sizes it so).
ESPGPU_HD inline bool replay_params_ok(const espgpu_replay &r) {
  if (r.wsize == 0) return true;
  const uint32_t b = r.bitmap_size;
  return b != 0 && (b & (b - 1)) == 0 && (uint64_t)b * 32 >= (uint64_t)r.wsize * 8;
}

// Usable for the 64-bit rule (wsize != 0 is the caller's): also the redundant
// block (key.c:3343-3351), a ring of at least window + 32 bits, or two
// sequence numbers of one window span could share a bit.
ESPGPU_HD inline bool replay_usable64(const espgpu_replay &r) {
  const uint32_t b = r.bitmap_size;
  return b != 0 && (b & (b - 1)) == 0 && (uint64_t)b * 32 >= (uint64_t)r.wsize * 8 + 32;
}

// check_window (ipsec.c:1191-1201): bit (seq & 31) of word (seq >> 5) masked
// by the power-of-two bitmap size (IPSEC_REDUNDANT_BIT_SHIFTS, :1177-1180).
ESPGPU_HD inline uint32_t replay_word(const espgpu_replay &r, uint64_t seq) {
  return r.bitmap_off + (uint32_t)((seq >> 5) & (r.bitmap_size - 1));
}
ESPGPU_HD inline bool replay_seen(const espgpu_replay &r, const uint32_t *bitmap, uint64_t seq) {
  return (bitmap[replay_word(r, seq)] >> (seq & 31)) & 1u;
}

// The advance of the window top from r.last to s (advance_window,
// ipsec.c:1203-1220): the ring words the top moves past, at most the ring.
inline void replay_advance(const espgpu_replay &r, uint32_t *bitmap, uint64_t s) {
  const uint64_t cur = r.last >> 5, mask = r.bitmap_size - 1;
  uint64_t diff = (s >> 5) - cur;
  if (diff > r.bitmap_size) diff = r.bitmap_size;
  for (uint64_t k = 0; k < diff; ++k) bitmap[r.bitmap_off + (uint32_t)((cur + 1 + k) & mask)] = 0;
}

// espgpu_replay_update's rule: ipsec_updatereplay (ipsec.c:1338-1436) with
// the window helpers advance_window / set_window (:1203-1232): after
// authentication, in arrival order per SA.  wsize != 0.
inline int replay_update_rule(espgpu_replay *r, uint32_t *bitmap, uint32_t seq) {
  if (!replay_params_ok(*r)) return ESPGPU_EINVAL;
  if (seq == 0 && r->last == 0) return ESPGPU_EACCES;
  auto mark = [&](uint32_t s) { bitmap[replay_word(*r, s)] |= 1u << (s & 31); };
  auto move_top = [&](uint64_t s) {
    replay_advance(*r, bitmap, s);
    mark(seq);
    r->last = s;
  };
  const uint32_t window = r->wsize << 3;
  const uint32_t tl = (uint32_t)r->last, th = (uint32_t)(r->last >> 32);
  const uint32_t bl = tl - window + 1;
  if ((tl >= window - 1 && seq >= bl) || (tl < window - 1 && seq < bl)) {
    if (seq > tl) {
      move_top(((uint64_t)th << 32) | seq);
    } else {
      if (replay_seen(*r, bitmap, seq)) return ESPGPU_EACCES;
      mark(seq);
    }
    return 0;
  }
  if (!(r->flags & ESPGPU_REPLAY_ESN)) return ESPGPU_EACCES;
  if (tl < window - 1 && seq >= bl) {   // in the window, previous subspace
    if (th == 0 || replay_seen(*r, bitmap, seq)) return ESPGPU_EACCES;
    mark(seq);
    return 0;
  }
  if (th + 1 == 0) return ESPGPU_EACCES;   // the high part would wrap
  move_top(((uint64_t)(th + 1) << 32) | seq);
  return 0;
}

// espgpu_replay_update64's rule: the same update on the 64-bit sequence number
// the record was authenticated under (ESN: esn_hi << 32 | seq; else seq):
// nothing is inferred, so a record that has fallen below the window is
// refused, never taken for the next subspace.  The rule
// espgpu_replay_update_batch applies (replay.hip).  wsize != 0.
inline int replay_update64_rule(espgpu_replay *r, uint32_t *bitmap, uint64_t seq64) {
  if (!replay_usable64(*r)) return ESPGPU_EINVAL;
  const uint64_t window = (uint64_t)r->wsize << 3;
  const uint64_t s = (r->flags & ESPGPU_REPLAY_ESN) ? seq64 : (uint32_t)seq64, top = r->last;
  if (s == 0 && top == 0) return ESPGPU_EACCES;
  if (s > top) {
    replay_advance(*r, bitmap, s);
    r->last = s;
  } else if (top - s >= window || replay_seen(*r, bitmap, s)) {   // below the window, or a replay
    return ESPGPU_EACCES;
  }
  bitmap[replay_word(*r, s)] |= 1u << (s & 31);
  return 0;
}

}  // namespace espgpu
