"""espgpu_replay_update64: ipsec_updatereplay (freebsd/netipsec/ipsec.c:
1338-1436) restated on the 64-bit sequence number a record was authenticated
under (include/espgpu.h, replay block).  It is the rule the device-side batch
update applies, so it is pinned here on the host first:
  * against the oracle's ipsec_updatereplay step by step, window state
    included, over batches of records that passed ipsec_chkreplay against the
    window the batch started from (wherever the record is in the reference's
    domain; outside it, the one deliberate difference: EACCES, nothing moves);
  * directed edge cases and the unusable-parameter rows;
  * the three facts the kernels rest on (prefix maximum, first
    come wins, closed-form final window), as a plain Python model of the
    parallel form compared with the sequential run."""
import ctypes as C

import numpy as np
import pytest

import oracle as O

EACCES, EINVAL = 13, 22
GUARD = 0xDEADBEEF


def _windows():
    """(wsize bytes, flags, start `last`): the grid of test_replay.py."""
    out = []
    for wsize in (4, 8, 32, 128):
        w = wsize * 8
        for flags in (0, O.REPLAY_ESN, O.REPLAY_CYCSEQ):
            for last in (0, 5, w - 3, w + 1000, 0xFFFFFFFF - 10, (7 << 32) | 3, (7 << 32) | 0xFFFFFFF0):
                if last >> 32 and not flags & O.REPLAY_ESN:
                    continue
                out.append((wsize, flags, last))
    return out


def _seqs(rng, last, w, k):
    """32-bit sequence numbers around the window top, with repeats: in the
    window, just above it, below it, the top and its neighbour, zero, and
    now and then far above or anywhere."""
    tl = last & 0xFFFFFFFF
    out = []
    for _ in range(k):
        c = [tl - rng.integers(0, w), tl + rng.integers(1, 3 * w), tl - w - rng.integers(0, 64),
             tl, tl + 1, 0, tl - rng.integers(0, w), tl + rng.integers(1, w // 2 + 2),
             rng.integers(0, 2**32), tl + (1 << 31)]
        p = np.array([4, 4, 2, 1, 1, 1, 4, 4, 0.3, 0.3])
        out.append(int(c[rng.choice(len(c), p=p / p.sum())]) & 0xFFFFFFFF)
    for j in range(k // 3):                            # exact repeats, near and far
        out[int(rng.integers(0, k))] = out[int(rng.integers(0, k))]
    return out


def _lib():
    import espgpu
    return espgpu.lib()


def _u32p(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint32))


def _batch_against_oracle(wsize, flags, last, kinds):
    from espgpu._lib import Replay
    L = _lib()
    rng = np.random.default_rng(wsize * 7919 + flags * 31 + (last & 0xFFFF) + 1)
    w = wsize * 8
    start = O.Replay(wsize, last=last, flags=flags)
    for sn in _seqs(rng, last, w, 60):                 # a used window
        start.update(sn)
    last = start.last
    batch = []
    for sn in _seqs(rng, last, w, 300):
        ok, sh = start.check(sn)
        if ok:
            batch.append((sn, (sh << 32) | sn if flags & O.REPLAY_ESN else sn))
    assert len(batch) > 50
    ref = O.Replay(wsize, last=last, flags=flags)
    ref.bitmap[:] = start.bitmap
    nb = ref.bitmap.size
    assert nb * 32 >= w + 32                           # key.c's redundant block
    bitmap = np.full(nb + 6, GUARD, dtype=np.uint32)   # window at word 3, guards around
    bitmap[3:3 + nb] = start.bitmap
    rp = Replay(last, wsize, nb, 3, flags)
    for sn, s64 in batch:
        before = (rp.last, bitmap.copy())
        got = L.espgpu_replay_update64(C.byref(rp), _u32p(bitmap), s64)
        if flags & O.REPLAY_ESN and s64 + w <= ref.last:
            # fallen below the window since the check: the reference would
            # take it for the next subspace; here it is refused
            assert got == EACCES and rp.last == before[0] and np.array_equal(bitmap, before[1])
            kinds["esn_out_of_domain"] += 1
            continue
        old_last = ref.last
        want = ref.update(sn)
        assert (got == 0) == want and got in (0, EACCES), (sn, hex(s64), got, want)
        assert rp.last == ref.last
        assert np.array_equal(bitmap[3:3 + nb], ref.bitmap)
        assert (bitmap[:3] == GUARD).all() and (bitmap[3 + nb:] == GUARD).all()
        if want:
            kinds["advance" if ref.last != old_last else "in_window"] += 1
        elif s64 + w > old_last:
            kinds["duplicate"] += 1
        else:
            kinds["below"] += 1


def _kinds():
    return {"advance": 0, "in_window": 0, "duplicate": 0, "below": 0, "esn_out_of_domain": 0}


@pytest.mark.parametrize("wsize,flags,last", _windows())
def test_update64_matches_oracle_over_batches(wsize, flags, last):
    _batch_against_oracle(wsize, flags, last, _kinds())


def test_update64_grid_meets_every_kind():
    """Across the grid: accepted by advance, accepted in the window,
    duplicate, below the window and ESN out of the reference's domain all
    occur."""
    kinds = _kinds()
    for wsize, flags, last in _windows():
        _batch_against_oracle(wsize, flags, last, kinds)
    assert all(v > 0 for v in kinds.values()), kinds


def _fresh(wsize, last=0, flags=0, nb=None, off=2):
    from espgpu._lib import Replay
    ref = O.Replay(wsize, last=last, flags=flags)
    nb = ref.bitmap.size if nb is None else nb
    bitmap = np.full(max(nb, 1) + 2 * off, GUARD, dtype=np.uint32)
    bitmap[off:off + nb] = 0
    return Replay(last, wsize, nb, off, flags), bitmap


def test_update64_directed_cases():
    L = _lib()
    up = lambda rp, bm, s: L.espgpu_replay_update64(C.byref(rp), _u32p(bm), s)
    # sequence number 0 on an empty window; then 1 is fine, and 0 is inside the window
    rp, bm = _fresh(8)
    assert up(rp, bm, 0) == EACCES and rp.last == 0 and (bm[2:6] == 0).all()
    assert up(rp, bm, 1) == 0 and rp.last == 1 and bm[2] == 2
    assert up(rp, bm, 0) == 0 and bm[2] == 3 and up(rp, bm, 0) == EACCES
    # an advance larger than the ring zeroes every word, then sets one bit
    rp, bm = _fresh(4, last=40)                        # 2 words
    for s in (40, 39, 33, 12, 9):
        assert up(rp, bm, s) == 0
    assert bm[2] and bm[3]
    assert up(rp, bm, 40 + 1000) == 0 and rp.last == 1040
    want = np.zeros(2, dtype=np.uint32)
    want[(1040 >> 5) & 1] = 1 << (1040 & 31)
    assert np.array_equal(bm[2:4], want) and (bm[:2] == GUARD).all() and (bm[4:] == GUARD).all()
    # ESN across a 2^32 boundary, against the oracle
    rp, bm = _fresh(8, last=(2 << 32) | 0xFFFFFFF0, flags=O.REPLAY_ESN)
    ref = O.Replay(8, last=(2 << 32) | 0xFFFFFFF0, flags=O.REPLAY_ESN)
    for s64 in ((3 << 32) | 5, (2 << 32) | 0xFFFFFFF8, (2 << 32) | 0xFFFFFFF8, (3 << 32) | 5, (3 << 32) | 2,
                (2 << 32) | 0xFFFFFFC6):
        got = up(rp, bm, s64)
        assert (got == 0) == ref.update(s64 & 0xFFFFFFFF), hex(s64)
        assert rp.last == ref.last and np.array_equal(bm[2:2 + ref.bitmap.size], ref.bitmap)
    assert rp.last == (3 << 32) | 5
    # ... and the deliberate difference: (2, 0xFFFFFF00) is below the window
    # now; the reference would take its low word for a later sequence number
    keep = bm.copy()
    assert up(rp, bm, (2 << 32) | 0xFFFFFF00) == EACCES
    assert rp.last == (3 << 32) | 5 and np.array_equal(bm, keep)
    # a non-ESN window ignores the high word
    rp, bm = _fresh(8, last=100)
    assert up(rp, bm, (9 << 32) | 101) == 0 and rp.last == 101
    # wsize 0: no window
    rp, bm = _fresh(0, last=7, nb=0)
    assert up(rp, bm, 3) == 0 and rp.last == 7 and (bm == GUARD).all()


@pytest.mark.parametrize("wsize,bsize,ok", [
    (8, 0, False),         # no bitmap words
    (8, 3, False),         # not a power of two
    (8, 1, False),         # 64 window bits in one 32-bit word
    (8, 2, False),         # bitmap_size * 32 == W: no redundant block
    (8, 4, True),
    (128, 16, False),
    (128, 32, False),      # 1024 bits for a 1024-packet window: no redundant block
    (128, 64, True),
])
def test_update64_rejects_unusable_windows(wsize, bsize, ok):
    from espgpu._lib import Replay
    L = _lib()
    rp = Replay(100, wsize, bsize, 0, 0)
    bitmap = np.full(max(bsize, 1) + 4, 0xA5A5A5A5, dtype=np.uint32)
    got = L.espgpu_replay_update64(C.byref(rp), _u32p(bitmap), 101)
    if ok:
        assert got == 0 and rp.last == 101
    else:
        assert got == EINVAL and rp.last == 100 and (bitmap == 0xA5A5A5A5).all()


# ---- the parallel form ------------------------------------------------------

def parallel_update(last, wsize, nb, bitmap, seqs):
    """The batch update as the kernels compute it, for one SA: `bitmap` is the
    window's nb words, seqs the seq64 of its taking-part records in arrival
    order.  Returns (verdicts, last, bitmap)."""
    w, t0, init = wsize * 8, last, bitmap.copy()
    tops, m = [], t0
    for s in seqs:                                     # exclusive prefix maximum
        tops.append(m)
        m = max(m, s)
    first = {}
    for p, (s, top) in enumerate(zip(seqs, tops)):     # first occurrence per seq64
        if not (s == 0 and top == 0):
            first.setdefault(s, p)
    verdict = []
    for p, (s, top) in enumerate(zip(seqs, tops)):
        if s == 0 and top == 0:
            ok = False
        elif s > top:
            ok = True
        elif top - s < w:
            seen = (int(init[(s >> 5) & (nb - 1)]) >> (s & 31)) & 1
            ok = ((s >> 5) > (t0 >> 5) or not seen) and first[s] == p
        else:
            ok = False
        verdict.append(0 if ok else EACCES)
    out = init.copy()
    for k in range(min((m >> 5) - (t0 >> 5), nb)):
        out[((t0 >> 5) + 1 + k) & (nb - 1)] = 0
    for s, v in zip(seqs, verdict):
        if v == 0 and (s >> 5) + nb > (m >> 5):
            out[(s >> 5) & (nb - 1)] |= np.uint32(1 << (s & 31))
    return verdict, m, out


@pytest.mark.parametrize("wsize,flags,last", _windows())
def test_parallel_form_equals_sequential(wsize, flags, last):
    from espgpu._lib import Replay
    L = _lib()
    rng = np.random.default_rng(wsize * 31 + flags * 7 + (last & 0xFFF) + 5)
    w = wsize * 8
    start = O.Replay(wsize, last=last, flags=flags)
    for sn in _seqs(rng, last, w, 80):
        start.update(sn)
    last, nb = start.last, start.bitmap.size
    hi = last >> 32
    # any seq64, not only what a check would let through
    seqs = [((int(rng.integers(max(hi - 1, 0), hi + 2)) << 32) | sn) if flags & O.REPLAY_ESN else sn
            for sn in _seqs(rng, last, w, 400)]
    bitmap = start.bitmap.copy()
    rp = Replay(last, wsize, nb, 0, flags)
    want = [L.espgpu_replay_update64(C.byref(rp), _u32p(bitmap), s) for s in seqs]
    got, glast, gmap = parallel_update(last, wsize, nb, start.bitmap, seqs)
    assert got == want
    assert glast == rp.last and np.array_equal(gmap, bitmap)
