"""espgpu_replay_update_batch (replay.hip) in the value regimes that
test_replay_update_gpu.py leaves out: a second and a third radix pass, n on
the sort-tile / scan-block / workgroup / wave boundaries, a second round of
the carry kernel, a first-occurrence table at its densest, one long SA between
short ones, a workspace that grows between calls in flight, a caller's stream.

The reference and the comparison are that file's: _host_run (the host
espgpu_replay_update64 per taking-part record in index order) and _compare
(d_ustatus for every record, the whole table, every bitmap and guard word;
_device_run checks d_desc and d_status unmodified).

The batch generators are plain seeded functions, so the CPU test at the end
runs the reference over each of them, asserts the conditions that keep a GPU
comparison from passing vacuously (_conditions; the GPU tests assert them
too) and checks the Python model of the kernels' three facts
(test_replay_update64.parallel_update) on the same shapes."""
import functools

import numpy as np
import pytest

import oracle as O
from test_replay_update64 import _seqs, parallel_update
from test_replay_update_gpu import (EACCES, EINVAL, GUARD, SCAN_BLOCK, SORT_TILE, _compare, _device_run,
                                    _host_run, _records, _tables, _torch, drv)  # noqa: F401 (drv: fixture)

ESN = O.REPLAY_ESN
CARRY_ROUND = 256 * SCAN_BLOCK     # grouped positions per round of upd_scan_carry_kernel (256 aggregates)

PASS_NREPLAY = (255, 256, 257, 1024, 65535, 65536, 65537)      # 1, 2, 2, 2, 2, 3, 3 radix passes
BOUNDARY_N = (63, 64, 65, 255, 256, 257, SCAN_BLOCK - 1, SCAN_BLOCK, SCAN_BLOCK + 1,
              SORT_TILE - 1, SORT_TILE, SORT_TILE + 1, 2 * SORT_TILE)
FULL_LOAD_N = (512, SCAN_BLOCK, SORT_TILE, 2 * SORT_TILE)      # hash_cap(n) == 2n
FULL_LOAD_SEEDS = (0, 1, 2, 3)
CARRY_ROUNDS = (2, 3)               # rounds of the carry kernel's loop
REGROW_CALLS = ((0, 300, 3), (300, 5000, 300), (5300, 200, 300))   # (start, count, nreplay)


class Batch:
    """One table, one bitmap array and n records; the host result is computed
    once and handed out as it is (nothing here modifies it)."""

    def __init__(self, tab, words, sa, s64, status=None, length=None, calls=None, **info):
        self.tab, self.words = tab, words
        self.s64 = np.asarray(s64).astype(np.uint64)
        self.arena, self.desc = _records(np.asarray(sa).astype(np.uint16), self.s64, length)
        self.n = len(self.desc)
        self.status = np.zeros(self.n, dtype=np.uint8) if status is None else np.asarray(status, dtype=np.uint8)
        self.seq32 = (self.s64 & np.uint64(0xFFFFFFFF)).astype(np.uint32)
        self.calls = calls                         # None: one call over the whole table
        self.info = info
        self._want = None

    def want(self):
        if self._want is None:
            if self.calls is None:
                self._want = _host_run(self.tab, self.words, self.desc, self.seq32, self.status)
                self.per_call = None
            else:
                self._want, self.per_call = _host_run_calls(self, self.calls)
        return self._want


def _host_run_calls(b, calls):
    """_host_run per (start, count, nreplay) call, each on the windows the
    one before left: the sequential run over the concatenation, in which a
    record whose sa is not below its call's nreplay takes no part."""
    tab, words = b.tab.copy(), b.words
    ust = np.zeros(b.n, dtype=np.uint8)
    per_call = []
    for a, cnt, nrp in calls:
        u, t, words = _host_run(tab[:nrp], words, b.desc[a:a + cnt], b.seq32[a:a + cnt], b.status[a:a + cnt])
        per_call.append((int((t["last"] != tab["last"][:nrp]).sum()), int((u == EACCES).sum())))
        tab[:nrp] = t
        ust[a:a + cnt] = u
    return (ust, tab, words), per_call


# ---- windows ------------------------------------------------------------------

def _ring_words(wsize):
    """key_setsaval's bitmap size in words (as oracle.Replay): the smallest
    power of two >= wsize + 4 bytes; none for wsize 0."""
    wsize = np.asarray(wsize, dtype=np.int64)
    nb = np.ones_like(wsize)
    for _ in range(12):
        nb = np.where(nb < wsize + 4, nb * 2, nb)
    return np.where(wsize == 0, 0, np.maximum(nb // 4, 1))


def _window_arrays(rng, last, wsize, flags, nb=None, used=None, marks=3, gap=2):
    """_tables' layout (windows `gap` guard words apart in one array) from
    arrays, without a Python loop over the windows.  `used` windows start with
    the bit of `last` and of up to `marks` - 1 more sequence numbers of the
    window set, as after earlier batches."""
    from espgpu.batch import REPLAY_DTYPE
    last, wsize = np.asarray(last, dtype=np.uint64), np.asarray(wsize, dtype=np.int64)
    nb = _ring_words(wsize) if nb is None else np.asarray(nb, dtype=np.int64)
    nw = len(last)
    off = gap + np.concatenate([[0], np.cumsum(nb + gap)[:-1]]).astype(np.int64)
    tab = np.zeros(nw, dtype=REPLAY_DTYPE)
    tab["last"], tab["wsize"], tab["bitmap_size"], tab["bitmap_off"], tab["flags"] = last, wsize, nb, off, flags
    words = np.full(gap + int((nb + gap).sum()), GUARD, dtype=np.uint32)
    start = np.cumsum(nb) - nb
    words[np.repeat(off, nb) + np.arange(int(nb.sum())) - np.repeat(start, nb)] = 0
    if used is not None:
        li = last.astype(np.int64)
        can = np.asarray(used, dtype=bool) & (wsize > 0) & (nb > 0) & ((nb & (nb - 1)) == 0) & (li > 0)
        for k in range(marks):
            d = np.zeros(nw, dtype=np.int64) if k == 0 else (rng.random(nw) * wsize * 8).astype(np.int64)
            at = np.flatnonzero(can & (li >= d))
            s = li[at] - d[at]
            np.bitwise_or.at(words, off[at] + ((s >> 5) & (nb[at] - 1)), (1 << (s & 31)).astype(np.uint32))
    return tab, words


def _mixed_windows(rng, nw, wsizes, same_last=None):
    """nw windows: a third ESN, half of them used, tops on the small, the
    ordinary and the wrapping side (or all at `same_last`)."""
    wsize = rng.choice(wsizes, nw)
    flags = np.where(rng.random(nw) < 0.35, ESN, 0)
    kind = rng.integers(0, 5, nw)
    lo = np.select([kind == 0, kind == 1, kind == 2, kind == 3],
                   [0, 5, 0xFFFFFFFF - 10, 0xFFFFFFF0], rng.integers(100, 1 << 31, nw))
    last = np.where(flags == ESN, (7 << 32) | lo, lo) if same_last is None else np.full(nw, same_last)
    return last.astype(np.uint64), wsize, flags, rng.random(nw) < 0.5


def _draw(rng, tab, sa, n):
    """seq64 per record from _seqs around the top of its SA's window (the
    window's high word for an ESN SA)."""
    s64 = np.zeros(n, dtype=np.uint64)
    for s in np.unique(sa):
        if s >= len(tab):
            last, w, esn = 1000, 64, False
        else:
            last, w, esn = int(tab["last"][s]), max(int(tab["wsize"][s]), 1) * 8, bool(tab["flags"][s] & ESN)
        at = np.flatnonzero(sa == s)
        lo = np.array(_seqs(rng, last, w, at.size), dtype=np.uint64)
        s64[at] = lo | (np.uint64(last >> 32 << 32) if esn else np.uint64(0))
    return s64


def _sprinkle(rng, n, sa, nreplay, p_status=0.10, p_len=0.03, p_beyond=0.03):
    """Records that take no part: status != 0, len < 8, and (where 16 bits
    can hold one) an sa not below nreplay."""
    status = np.where(rng.random(n) < p_status, 80, 0).astype(np.uint8)
    length = np.where(rng.random(n) < p_len, 4, 16).astype(np.uint16)
    sa = sa.copy()
    if nreplay < 65536:
        at = np.flatnonzero(rng.random(n) < p_beyond)
        sa[at] = np.minimum(nreplay + rng.integers(0, 5, at.size), 65535)
    return status, length, sa


# ---- 1. table sizes around the pass boundaries -----------------------------

def _pass_sas(rng, nreplay):
    """About 64 SAs on which every radix pass matters: some that share the
    low byte and differ in the high one, some that differ only in the low
    byte, SA 0 and the last one a descriptor can name; four more have no
    window (wsize 0) or an unusable one."""
    top = min(nreplay, 65536) - 1
    c = 0x37
    sas = [0, top] + [256 * k for k in (1, 2) if 256 * k < nreplay]
    sas += [256 * k + c for k in (0, 1, 2, 3, 5, 0x80, 0xFE, 0xFF) if 256 * k + c < nreplay]
    base = 0x0400 if nreplay > 0x0500 else 0
    sas += [base + j for j in (0x01, 0x02, 0x36, 0x38, 0x7F, 0x80, 0xFE, 0xFF) if base + j < nreplay]
    sas = list(dict.fromkeys(sas))
    rest = [int(s) for s in rng.permutation(nreplay if nreplay < 65536 else 65536) if s not in sas]
    sas += rest[:64 - len(sas)]
    return sas, rest[64:66], rest[66:68]           # records go to these; wsize 0; unusable


def gen_pass_boundary(nreplay):
    rng = np.random.default_rng(1000 + nreplay)
    n = 2 * SORT_TILE + 1                          # three sort tiles, one record in the last
    sas, nowin, unusable = _pass_sas(rng, nreplay)
    last, wsize, flags, used = _mixed_windows(rng, nreplay, (4, 8))
    wsize[nowin] = 0
    wsize[rng.integers(0, nreplay, 5)] = 0         # ... and a few that no record names
    wsize[sas] = np.where(wsize[sas] == 0, 8, wsize[sas])
    nb = _ring_words(wsize)
    nb[unusable] = (2, 3)                          # no redundant block; not a power of two
    wsize[unusable] = 8
    tab, words = _window_arrays(rng, last, wsize, flags, nb=nb, used=used)
    sa = rng.choice(np.array(sas + nowin + unusable), n)
    s64 = _draw(rng, tab, sa, n)
    src = rng.integers(0, SORT_TILE - 48, 150)     # exact repeats more than a sort tile apart
    dst = src + SORT_TILE + 1 + rng.integers(0, 40, 150)
    sa[dst], s64[dst] = sa[src], s64[src]
    status, length, sa = _sprinkle(rng, n, sa, nreplay)
    return Batch(tab, words, sa, s64, status, length, sas=sas, nowin=nowin, unusable=unusable)


def gen_uniform_1024():
    """n = one sort tile + 1 over 1024 SAs drawn uniformly: one to three
    records per SA, so nearly every grouped position is a segment head; every
    window starts from the same `last`, so one seq64 occurs under many SAs."""
    rng = np.random.default_rng(77)
    nreplay, n = 1024, SORT_TILE + 1
    last, wsize, flags, used = _mixed_windows(rng, nreplay, (4, 8), same_last=5000)
    wsize[rng.integers(0, nreplay, 10)] = 0
    nb = _ring_words(wsize)
    bad = rng.integers(0, nreplay, 10)
    wsize[bad], nb[bad] = 8, 2
    tab, words = _window_arrays(rng, last, wsize, flags, nb=nb, used=used)
    sa = rng.integers(0, nreplay, n)
    s64 = np.array(_seqs(rng, 5000, 64, n), dtype=np.uint64)
    status, length, sa = _sprinkle(rng, n, sa, nreplay)
    return Batch(tab, words, sa, s64, status, length)


# ---- 2. n on the tile, block, workgroup and wave boundaries ---------------

def gen_boundary(n):
    """Three SAs (ESN, used, fresh), a wsize 0 entry, a few records that take
    no part, random arrival order."""
    rng = np.random.default_rng(2000 + n)
    tab, words = _window_arrays(rng, [(3 << 32) | 0xFFFFFF00, 5000, 0, 9], [32, 8, 4, 0], [ESN, 0, 0, 0],
                                used=[False, True, False, False], marks=12)
    sa = rng.integers(0, 3, n)
    sa[rng.random(n) < 0.02] = 3                   # no window
    s64 = _draw(rng, tab, sa, n)
    status, length, sa = _sprinkle(rng, n, sa, 4, p_status=0.05, p_len=0.02, p_beyond=0.02)
    # the record in the tail (of a wave, a workgroup, a scan block, a sort
    # tile at n = boundary + 1) takes part and repeats the first of its SA:
    # lost, or grouped ahead of it, it is not refused
    sa[0] = sa[n - 1] = n % 3
    s64[n - 1] = s64[0] = _draw(rng, tab, sa[:1], 1)[0]
    status[[0, n - 1]], length[[0, n - 1]] = 0, 16
    return Batch(tab, words, sa, s64, status, length)


def gen_full_load(n, seed):
    """Every record takes part and most (SA, seq64) pairs are distinct, so
    the first-occurrence table of 2n slots is as full as it gets.  Two
    1024-packet windows; the sequence numbers ascend from below the top with a
    shuffle narrower than the window, so most records arrive inside it and are
    looked up; about a tenth are exact repeats of an earlier record."""
    rng = np.random.default_rng(3000 + 16 * n + seed)
    lasts = [(2 << 32) | 0xFFFFFE00, 70000]        # the ESN top crosses 2^32 inside the batch
    tab, words = _window_arrays(rng, lasts, [128, 128], [ESN, 0], used=[True, True], marks=200)
    sa = rng.integers(0, 2, n)
    s64 = np.zeros(n, dtype=np.int64)
    for k in (0, 1):
        at = np.flatnonzero(sa == k)
        s = lasts[k] - 100 + np.arange(at.size, dtype=np.int64)
        for a in range(0, at.size, 700):
            s[a:a + 700] = s[a:a + 700][rng.permutation(s[a:a + 700].size)]
        s64[at] = s
    for src in rng.integers(0, n - 1, n // 10):
        dst = int(rng.integers(src + 1, n))
        sa[dst], s64[dst] = sa[src], s64[src]
    return Batch(tab, words, sa, s64)


# ---- 3. a second (and a third) round of the carry kernel ------------------

def gen_carry_round(rounds):
    """(rounds - 1) * 256 + 2 scan blocks, the last one partial, so the carry
    loop's last round has two live entries.  SA 0 (ESN, 1024 packets) owns all
    but 500 records: ascending from below its top across 2^32, shuffled in
    runs wider than the window, with exact repeats on both sides of every
    multiple of CARRY_ROUND (SA 0 sorts first: grouped position = rank among
    its records).  SA 1's records are scattered through the arrival order; its
    segment head lies in the last carry round, and its window starts far below
    SA 0's numbers.  rounds = 2 is the smallest batch with a second round.
    Only with a third does a carry have to be folded and not just handed on,
    and only if an earlier round holds the maximum: see below."""
    rng = np.random.default_rng(5 + rounds)
    n, n1 = (rounds - 1) * CARRY_ROUND + SCAN_BLOCK + 1, 500
    n0 = n - n1
    t0 = (5 << 32) | (0xFFFFFFFF - 150000)
    s0 = t0 - 200 + np.arange(n0, dtype=np.int64)
    for a in range(0, n0, 1500):
        s0[a:a + 1500] = s0[a:a + 1500][rng.permutation(s0[a:a + 1500].size)]
    repeats = [(SCAN_BLOCK - 2, SCAN_BLOCK)]
    for B in range(CARRY_ROUND, n0, CARRY_ROUND):
        repeats += [(B - 900, B - 890), (B - 5, B + 3), (B - 1, B), (B + 7, B + 9),
                    (B - SCAN_BLOCK - 1, B - SCAN_BLOCK)]
    for src, dst in repeats:
        s0[dst] = s0[src]
    if rounds > 2:
        # one record late in the first round lies above all of the second and
        # just above the start of the third: what the third round's blocks
        # see is the first round's maximum, not the second's
        s0[CARRY_ROUND - 3000] = t0 - 200 + 2 * CARRY_ROUND + 1400
    tab, words = _window_arrays(rng, [t0, 1000], [128, 32], [ESN, ESN], used=[True, True], marks=200)
    sa = np.zeros(n, dtype=np.int64)
    sa[rng.choice(n, n1, replace=False)] = 1
    s64 = np.zeros(n, dtype=np.int64)
    s64[sa == 0] = s0
    s1 = np.array(_seqs(rng, 1000, 256, n1), dtype=np.int64)
    s64[sa == 1] = np.where(s1 > 1 << 20, 1100, s1)   # (no jump to the far end of the 32-bit space)
    return Batch(tab, words, sa, s64, repeat_dst=[d for _, d in repeats], t0=t0)


# ---- 4. one long SA between short ones -------------------------------------

def gen_long_sa():
    """40 SAs; SA 20 holds 3500 records (its segment covers whole scan blocks
    with no head inside, between short segments on both sides), the others 64
    each."""
    rng = np.random.default_rng(11)
    nw = 40
    last, wsize, flags, used = _mixed_windows(rng, nw, (4, 8, 32, 128))
    tab, words = _window_arrays(rng, last, wsize, flags, used=used, marks=20)
    sa = rng.permutation(np.concatenate([np.full(3500, 20), np.repeat(np.delete(np.arange(nw), 20), 64)]))
    n = sa.size
    s64 = _draw(rng, tab, sa, n)
    status, length, sa = _sprinkle(rng, n, sa, nw, p_status=0.05, p_len=0.01, p_beyond=0.01)
    return Batch(tab, words, sa, s64, status, length)


# ---- 5. workspace growth between unsynchronised calls ----------------------

def gen_regrow():
    """Three calls' records over one table of 300 windows: 300 records
    against its first 3 entries (sa 3 .. 5 take no part there), 5000 against
    all of it, 200 again.  Every call draws on SAs 0 to 2, each a little
    higher than the one before, so every call moves tops."""
    rng = np.random.default_rng(31)
    nw = 300
    last, wsize, flags, used = _mixed_windows(rng, nw, (4, 8, 32))
    last[:3], wsize[:3], flags[:3] = [(7 << 32) | 4000, 5000, 0], [32, 8, 4], [ESN, 0, 0]
    tab, words = _window_arrays(rng, last, wsize, flags, used=used, marks=8)
    sa, s64 = [], []
    for k, (a, cnt, nrp) in enumerate(REGROW_CALLS):
        s = np.where(rng.random(cnt) < (0.3 if k == 1 else 0.8), rng.integers(0, 3, cnt),
                     rng.integers(0, 6 if k == 0 else nw, cnt))
        t = tab.copy()
        t["last"][:3] += np.uint64(100 * k)        # the later calls aim above the earlier ones
        sa.append(s)
        s64.append(_draw(rng, t, s, cnt))
    sa, s64 = np.concatenate(sa), np.concatenate(s64)
    status = np.where(rng.random(sa.size) < 0.05, 80, 0)
    return Batch(tab, words, sa, s64, status, calls=REGROW_CALLS)


# ---- the cases, and what the reference must show on each --------------------

@functools.lru_cache(maxsize=None)
def _case(kind, *args):
    return {"pass": gen_pass_boundary, "uniform": gen_uniform_1024, "boundary": gen_boundary,
            "full": gen_full_load, "carry": gen_carry_round, "long": gen_long_sa, "regrow": gen_regrow}[kind](*args)


CASES = ([("pass", r) for r in PASS_NREPLAY] + [("uniform",)] + [("boundary", n) for n in BOUNDARY_N]
         + [("full", n, s) for n in FULL_LOAD_N for s in FULL_LOAD_SEEDS] + [("carry", r) for r in CARRY_ROUNDS] + [("long",), ("regrow",)])


def _case_id(c):
    return "-".join(str(x) for x in c)


def _taking_part(b):
    """The records upd_prep_kernel gives an SA key (per call, where the calls
    differ in nreplay)."""
    sa = b.desc["sa"].astype(np.int64)
    nrp = np.full(b.n, len(b.tab))
    for a, cnt, r in (b.calls or ()):
        nrp[a:a + cnt] = r
    t = b.tab[np.minimum(sa, len(b.tab) - 1)]
    nb, wsize = t["bitmap_size"].astype(np.int64), t["wsize"].astype(np.int64)
    usable = (nb != 0) & ((nb & (nb - 1)) == 0) & (nb * 32 >= wsize * 8 + 32)
    return (b.status == 0) & (sa < nrp) & (b.desc["len"] >= 8) & (wsize != 0) & usable


def _seq_eff(b):
    """The number the rule works on: seq64 for an ESN SA, its low word else."""
    sa = np.minimum(b.desc["sa"].astype(np.int64), len(b.tab) - 1)
    return np.where(b.tab["flags"][sa] & ESN, b.s64, b.s64 & np.uint64(0xFFFFFFFF))


def _walk(b):
    """Per record: takes part; arrives inside the window (s <= top and
    top - s < window, top = the prefix maximum of the model); repeats an
    earlier taking-part record of its SA."""
    took, s, sa = _taking_part(b), _seq_eff(b), b.desc["sa"]
    inwin, repeat = np.zeros(b.n, dtype=bool), np.zeros(b.n, dtype=bool)
    top, seen = {}, set()
    for i in np.flatnonzero(took):
        k, si = int(sa[i]), int(s[i])
        t = top.get(k, int(b.tab["last"][k]))
        inwin[i] = si <= t and t - si < int(b.tab["wsize"][k]) * 8
        repeat[i] = (k, si) in seen
        seen.add((k, si))
        top[k] = max(t, si)
    return took, inwin, repeat


def _model_check(b, want):
    """parallel_update (the kernels' three facts in Python) per SA against
    the host rule: verdicts, final top, final window words."""
    took, s, sa = _taking_part(b), _seq_eff(b), b.desc["sa"]
    for k in np.unique(sa[took]):
        at = np.flatnonzero(took & (sa == k))
        t = b.tab[k]
        off, nb = int(t["bitmap_off"]), int(t["bitmap_size"])
        v, last, bm = parallel_update(int(t["last"]), int(t["wsize"]), nb, b.words[off:off + nb],
                                      [int(x) for x in s[at]])
        assert v == list(want[0][at]), k
        assert last == want[1]["last"][k] and np.array_equal(bm, want[2][off:off + nb]), k


def _conditions(case, b, want):
    """What keeps a comparison with `want` from passing vacuously.  These
    are conditions on the reference alone."""
    kind = case[0]
    ust = want[0]
    took = _taking_part(b)
    assert (ust[took] == 0).any() and (ust == EACCES).any()
    assert not ust[~took & (ust != EINVAL)].any()
    if kind in ("pass", "uniform", "boundary", "long"):
        assert (~took).sum() >= 1 and (b.status != 0).any()
    if kind == "boundary":
        assert took[0] and took[-1] and ust[-1] == EACCES and b.desc["sa"][0] == b.desc["sa"][-1]
    if kind == "pass":
        nreplay, sa = case[1], b.desc["sa"]
        assert (ust == EINVAL).any() and (sa[took] == 0).any() and (sa[took] == min(nreplay, 65536) - 1).any()
        if nreplay < 65536:
            assert (sa >= nreplay).any()
        _, _, repeat = _walk(b)
        both = [k for k in np.unique(sa[took])
                if (ust[took & (sa == k)] == 0).any() and (repeat & (sa == k) & (ust == EACCES)).any()]
        far = np.flatnonzero(repeat & (ust == EACCES))
        assert both and far.size > 100
        if nreplay > 256:                          # below that no two SAs differ in the high byte
            low = [k & 0xFF for k in both]
            assert any(low.count(x) >= 2 for x in set(low)), both
    if kind == "full":
        assert took.all()
        _, inwin, repeat = _walk(b)
        assert inwin.sum() * 5 >= b.n and repeat.sum() * 20 >= b.n
        assert np.unique(np.stack([b.desc["sa"].astype(np.uint64), b.s64]), axis=1).shape[1] * 10 >= 8 * b.n
    if kind == "carry":
        sa = b.desc["sa"]
        rank = np.cumsum(sa == 0) - 1                # grouped position of SA 0's records
        refused = rank[(sa == 0) & (ust == EACCES)]
        for B in range(CARRY_ROUND, b.n - 500, CARRY_ROUND):
            assert ((refused >= B - CARRY_ROUND) & (refused < B)).sum() > 50 and (refused >= B).sum() > 5
        at0 = np.flatnonzero(sa == 0)
        if case[1] > 2:
            # third-round records refused under the true top that the second
            # round's maximum alone would let in
            s0 = _seq_eff(b)[at0].astype(np.int64)
            r2, jump = 2 * CARRY_ROUND, s0[CARRY_ROUND - 3000]
            assert jump > s0[CARRY_ROUND:].max() - 2000 and jump == s0[:r2 + 300].max()
            m1 = np.maximum.accumulate(s0[CARRY_ROUND:])[r2 - CARRY_ROUND - 1:-1]
            assert ((jump - s0[r2:] >= 1024) & (m1 - s0[r2:] < 1024) & (ust[at0[r2:]] == EACCES)).sum() > 50
        for d in b.info["repeat_dst"]:
            assert ust[at0[d]] == EACCES
        assert (ust[sa == 1] == 0).sum() > 10         # under SA 0's maximum every one of them would be refused
        assert want[1]["last"][0] >> 32 == 6 and want[1]["last"][1] < 1 << 32
    if kind == "regrow":
        b.want()
        assert all(adv >= 1 and ref >= 1 for adv, ref in b.per_call), b.per_call
        a, cnt, nrp = b.calls[0]
        assert (b.desc["sa"][a:a + cnt] >= nrp).any()


# ---- GPU ---------------------------------------------------------------------

def _check(drv, case, **kw):
    b = _case(*case)
    want = b.want()
    _conditions(case, b, want)
    got = _device_run(drv, b.tab, b.words, b.arena, b.desc, b.status, **kw)
    _compare(got, want, n_guard_words=2 * (len(b.tab) + 1))


@pytest.mark.gpu
@pytest.mark.parametrize("nreplay", PASS_NREPLAY)
def test_update_pass_boundaries(drv, nreplay):
    """One, two and three radix passes: three sort tiles (the last of one
    record) over about 64 SAs chosen so that every digit orders some of them,
    with repeats more than a tile apart and the sentinel key mixed in."""
    _check(drv, ("pass", nreplay))


@pytest.mark.gpu
def test_update_heads_everywhere(drv):
    _check(drv, ("uniform",))


@pytest.mark.gpu
@pytest.mark.parametrize("n", BOUNDARY_N)
def test_update_n_on_boundaries(drv, n):
    _check(drv, ("boundary", n))


@pytest.mark.gpu
@pytest.mark.parametrize("seed", FULL_LOAD_SEEDS)
@pytest.mark.parametrize("n", FULL_LOAD_N)
def test_update_full_first_occurrence_table(drv, n, seed):
    _check(drv, ("full", n, seed))


@pytest.mark.gpu
@pytest.mark.parametrize("rounds", CARRY_ROUNDS)
def test_update_carry_rounds(drv, rounds):
    _check(drv, ("carry", rounds))


@pytest.mark.gpu
def test_update_long_sa_between_short_ones(drv):
    _check(drv, ("long",))


@pytest.mark.gpu
def test_update_workspace_grows_between_calls():
    """A driver of its own (the module's has seen larger batches): the
    workspace is freed and reallocated for the second call while the first may
    still run, and the third is carved from the larger buffer."""
    _torch()
    from espgpu.opencrypto import GpuCryptoDriver
    d = GpuCryptoDriver(max_sessions=64, batch_records=1024, batch_bytes=1 << 20, nbatches=1)
    try:
        _check(d, ("regrow",), calls=[tuple(c) for c in REGROW_CALLS])
    finally:
        d.close()


@pytest.mark.gpu
def test_update_on_a_callers_stream(drv):
    torch = _torch()
    _check(drv, ("boundary", 2 * SORT_TILE), stream=torch.cuda.Stream())


# ---- CPU: the generators, the reference on them, the model -----------------

def test_window_arrays_lay_out_as_tables():
    rng = np.random.default_rng(1)
    last, wsize, flags, _ = _mixed_windows(rng, 50, (0, 4, 8, 32, 128))
    tab, words = _window_arrays(rng, last, wsize, flags)
    wins = [(int(l), int(w), int(_ring_words(w)), int(f), None) for l, w, f in zip(last, wsize, flags)]
    tab2, words2 = _tables(wins)
    assert np.array_equal(tab, tab2) and np.array_equal(words, words2)
    for w in (4, 8, 32, 128):
        assert _ring_words(w) == O.Replay(w).bitmap.size
    # used windows: the top's bit and nothing outside the window or the ring
    tab, words = _window_arrays(rng, last, wsize, flags, used=np.ones(50, dtype=bool), marks=6)
    assert np.array_equal(words == GUARD, words2 == GUARD)
    for t in tab[(tab["wsize"] > 0) & (tab["last"] > 0)]:
        ring = words[t["bitmap_off"]:t["bitmap_off"] + t["bitmap_size"]]
        s = int(t["last"])
        assert (int(ring[(s >> 5) & (t["bitmap_size"] - 1)]) >> (s & 31)) & 1
        assert 1 <= sum(bin(int(x)).count("1") for x in ring) <= 6


@pytest.mark.parametrize("case", CASES, ids=_case_id)
def test_reference_on_generated_batches(case):
    b = _case(*case)
    want = b.want()
    _conditions(case, b, want)
    assert len(b.arena) >= 16 * b.n and (b.desc["off4"] * 4 + 16 <= len(b.arena)).all()
    if case[0] != "carry":                         # 264 000 and 526 000 records through the Python model: left out for time
        _model_check(b, want)
