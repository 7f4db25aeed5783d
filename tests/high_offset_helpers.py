"""Where in the arena a record lies (test_high_offsets.py on the CPU,
test_high_offsets_gpu.py and test_esp_natt_gpu.py on the GPU).

espgpu_desc.off4 and espgpu_pkt.off4 count 4-byte units: a batch addresses an
arena of 16 GiB, and a kernel has to form a record's pointer in 64 bits.  One
that multiplies in 32 bits, or casts a byte offset to int on the way, is right
for every arena below 2 GiB and wrong above.  A Place puts an existing small
layout at a high offset of a large device allocation, so that its records lie
on both sides of such a boundary and some across it:

  allocation  [0, ALLOC)  ALLOC = 2^31 + 2^32 + 2^23 bytes, filled with PATTERN
  arena ptr   allocation + GUARD (2^31): the pointer the library is given
  boundary B  2^31 ("sign") or 2^32 ("wrap"), measured from the arena pointer
  base        (B - cut) & ~127, the layout's byte 0 (its alignment classes
              modulo 128 survive); every off4 grows by base / 4
  window      [base, base + size) of the arena: the only bytes ever uploaded,
              downloaded or compared with a reference

The safety condition.  Every byte offset x that a record of a placed layout
touches (its bytes and the REACH bytes a kernel may read past it) has its
truncation x mod 2^32 and the sign extension of that 32-bit value inside the
allocation when added to the arena pointer: the first needs ALLOC - GUARD >=
2^32, the second GUARD >= 2^31.  A kernel that drops or mis-extends the high
bits of an offset therefore reads and writes mapped memory of the test's own
and gives a wrong answer; it cannot fault.  Place.check_safe asserts it record
by record instead of trusting this paragraph.

After a case everything outside the window, in the arena's allocation and in
the second one that serves as `out`, must still hold PATTERN (Arenas.finish:
compared on the device, chunk by chunk, the first differing offset reported
as seen from the arena pointer), and the window is set back to PATTERN."""
import numpy as np

GUARD = 1 << 31
ALLOC = (1 << 31) + (1 << 32) + (1 << 23)
SPAN = ALLOC - GUARD                         # bytes behind the arena pointer
BOUNDARIES = {"sign": 1 << 31, "wrap": 1 << 32}
PATTERN = 0x3C                               # neither check's OUT_FILL (0xA5) nor 0x00 / 0xEE / 0xFF
REACH = 16                                   # include/espgpu.h: readable bytes behind a record
CROSS_LEN = 512                              # a record at least this long crosses the boundary
CHUNK = 1 << 28

# packed output past 4 GiB: slot i at i * PACKED_STRIDE from the start of the
# second allocation (no guard in front: PACKED_N slots need 2^32 + 19.7 MB, more
# than lies behind the arena pointer).  A slot offset taken mod 2^32 stays
# inside the allocation; a sign-extended one would not, and the one place that
# forms the address (esp_gcm.hip do_group, `p.out + (size_t)di * p.out_stride`)
# multiplies unsigned in 64 bits.
PACKED_STRIDE = 65536
PACKED_HIGH = 300
PACKED_N = 65536 + PACKED_HIGH
PACKED_PAYLOAD = 12


def pick_cut(offs, lens, min_len=CROSS_LEN):
    """The layout's byte that comes to lie (at most 127 bytes below) the
    boundary: min_len / 2 bytes into the record of at least min_len bytes
    that starts nearest to the median record, so that about half of the
    records lie on each side."""
    offs, lens = np.asarray(offs, dtype=np.int64), np.asarray(lens, dtype=np.int64)
    long = np.nonzero(lens >= min_len)[0]
    assert len(long), "no record of %d bytes or more to lay across the boundary" % min_len
    mid = np.median(offs)
    i = long[np.argmin(np.abs(offs[long] - mid))]
    return int(offs[i]) + min_len // 2


class Place:
    """A layout of `size` bytes with records at byte offsets offs, lens bytes
    long, placed so that its byte `cut` lies at boundary B (a name of
    BOUNDARIES) or at most 127 bytes below it."""

    def __init__(self, boundary, size, offs, lens, cut=None, min_len=CROSS_LEN):
        self.name = boundary
        self.B = BOUNDARIES[boundary]
        self.size = int(size)
        self.offs = np.asarray(offs, dtype=np.int64)
        self.lens = np.asarray(lens, dtype=np.int64)
        self.min_len = min_len
        self.cut = pick_cut(self.offs, self.lens, min_len) if cut is None else int(cut)
        self.base = (self.B - self.cut) & ~127
        self.base4 = self.base // 4
        assert 0 <= self.base and self.base + self.size + REACH <= SPAN, "the window leaves the allocation"

    # -- relocation --------------------------------------------------------
    def relocate(self, recs):
        """A copy of a structured array with an off4 field (espgpu_desc or
        espgpu_pkt), every off4 base / 4 larger."""
        out = np.array(recs, copy=True)
        wide = out["off4"].astype(np.int64) + self.base4
        assert (wide < 1 << 32).all(), "a relocated off4 does not fit 32 bits"
        out["off4"] = wide.astype(np.uint32)
        return out

    def back(self, off4):
        """Offsets the device wrote (descriptors and packet lists of a later
        stage), as the same layout at base 0 would have them."""
        return (np.asarray(off4).astype(np.int64) - self.base4).astype(np.int64)

    # -- what the CPU test asserts -------------------------------------------
    def sides(self):
        """-> (records wholly below B, records across it, records wholly at or
        above it), as index arrays."""
        lo, hi = self.base + self.offs, self.base + self.offs + self.lens
        return np.nonzero(hi <= self.B)[0], np.nonzero((lo < self.B) & (hi > self.B))[0], np.nonzero(lo >= self.B)[0]

    def check_geometry(self, quarter=True):
        below, across, above = self.sides()
        n = len(self.offs)
        assert self.base % 128 == 0 and 0 <= self.B - self.cut - self.base < 128
        assert any(self.lens[i] >= self.min_len for i in across), \
            "%s: no record of %d bytes or more across the boundary" % (self.name, self.min_len)
        if quarter:
            assert 4 * len(below) >= n and 4 * len(above) >= n, "%s: %d records below, %d above, of %d" % (
                self.name, len(below), len(above), n)
        return len(below), len(across), len(above)

    def check_safe(self):
        """The safety condition, for every record's first and last touched
        byte (and so, both maps being monotonic between at most two breaks
        that are checked too, for every byte between)."""
        lo = self.base + self.offs
        hi = lo + np.maximum(self.lens, 1) + REACH - 1
        # (a kernel that truncates a record's start and walks on from there in
        # 64 bits stays inside too: what lies behind 2^32 is longer than a record)
        assert (hi - lo < SPAN - (1 << 32)).all()
        xs = [lo, hi]
        for brk in (1 << 31, 1 << 32):       # where truncation or sign extension jumps
            inside = (lo < brk) & (hi >= brk)
            xs += [np.where(inside, brk - 1, lo), np.where(inside, brk, lo)]
        for x in xs:
            assert (x >= 0).all() and (x < SPAN).all(), "a record's own bytes leave the allocation"
            t = x & 0xFFFFFFFF
            s = np.where(t >= 1 << 31, t - (1 << 32), t)
            for name, y in (("truncated", t), ("sign-extended", s)):
                ok = (GUARD + y >= 0) & (GUARD + y < ALLOC)
                assert ok.all(), "%s offset %d of byte %d leaves the allocation" % (
                    name, int(y[~ok][0]), int(x[~ok][0]))


def place_for_batch(b, boundary):
    """sweep_helpers.Batch"""
    return Place(boundary, len(b.plain), b.descs["off4"].astype(np.int64) * 4, b.descs["len"])


def place_for_layout(lay, boundary):
    """ah_sweep_helpers.Layout"""
    return Place(boundary, len(lay.arena), lay.off, lay.L)


def place_for_packets(arena, rec, boundary, head=72, tail=49):
    """The stage loop's cleartext packets (encap_helpers.layout: rec is the
    espgpu_pkt list, each packet with head writable bytes in front and tail
    behind).  A record here is a packet with its room, all of which the stage
    kernels may write; one of at least 256 + head + tail bytes crosses the
    boundary."""
    offs = rec["off4"].astype(np.int64) * 4 - head
    return Place(boundary, len(arena), offs, rec["len"].astype(np.int64) + head + tail, min_len=256 + head + tail)


# the layouts of test_high_offsets_gpu.py, by case name
def _layouts():
    import ah_sweep_helpers as A
    import sweep_helpers as S
    gcm = {"gcm-" + f: (lambda f=f: S.gcm_mixed(f)) for f in ("e-random", "a-aligned")}
    eta = {"eta-h-random-" + k: (lambda k=k: S.eta_mixed("h-random", k)) for k in S.MIXED_KINDS}
    eta["eta-interleaved"] = S.eta_interleaved
    return gcm, eta, {"ah-random": A.random_mix, "ah-hashes": A.hashes}


GCM_LAYOUTS, ETA_LAYOUTS, AH_LAYOUTS = _layouts()


# ---------------------------------------------------------------------------
# the device side

class Arenas:
    """The two allocations, made and filled once (a module-scoped fixture) and
    released with release()."""

    def __init__(self):
        import torch
        self.torch = torch
        self.bufs = []
        try:
            for _ in range(2):
                self.bufs.append(torch.empty(ALLOC, dtype=torch.uint8, device="cuda"))
        except RuntimeError as e:            # torch.OutOfMemoryError is one
            self.bufs = []
            torch.cuda.empty_cache()
            raise AssertionError("two device allocations of %d bytes (%.2f GiB) each are needed: %s" % (
                ALLOC, ALLOC / 2.0**30, str(e).splitlines()[0]))
        for t in self.bufs:
            t.fill_(PATTERN)
        torch.cuda.synchronize()

    def release(self):
        self.bufs = []
        self.torch.cuda.empty_cache()

    def arena(self):
        """The tensor whose data_ptr() is the arena pointer."""
        return self.bufs[0][GUARD:]

    def out(self):
        return self.bufs[1][GUARD:]

    def out_from_start(self):
        return self.bufs[1]

    def first_stray(self, t, skip=None):
        """The first index of t outside skip = (lo, hi) that does not hold
        PATTERN, or None; such bytes are set back to PATTERN."""
        torch = self.torch
        n = t.numel()
        spans = [(0, n)] if skip is None else [(0, max(skip[0], 0)), (min(skip[1], n), n)]
        pieces = [(a, min(a + CHUNK, hi)) for lo, hi in spans if hi > lo for a in range(lo, hi, CHUNK)]
        flags = torch.stack([(t[a:b] != PATTERN).any() for a, b in pieces]).cpu().numpy()
        first = None
        for (a, b), f in zip(pieces, flags):
            if f:
                if first is None:
                    first = a + int(torch.nonzero(t[a:b] != PATTERN)[0, 0])
                t[a:b].fill_(PATTERN)
        return first


class Placed:
    """A Place on the Arenas: what sweep_helpers.check, ah_sweep_helpers.check
    and the end-to-end loop take as their placement."""

    def __init__(self, arenas, place):
        self.arenas, self.place = arenas, place
        self.base, self.base4, self.size = place.base, place.base4, place.size
        self.relocate, self.back = place.relocate, place.back

    def load(self, src):
        """src (numpy uint8, the layout's arena) uploaded into the window.
        -> (the tensor to hand to the library, the window's view)"""
        torch = self.arenas.torch
        assert len(src) == self.size
        arena = self.arenas.arena()
        win = arena[self.base:self.base + self.size]
        win.copy_(torch.from_numpy(np.array(src)))
        return arena, win

    def out(self, fill):
        """-> (`out` for the library, its window's view, prefilled)"""
        out = self.arenas.out()
        win = out[self.base:self.base + self.size]
        win.fill_(fill)
        return out, win

    def finish(self):
        """Everything outside the window holds PATTERN in both allocations;
        the window is set back.  Offsets in the message are as seen from the
        arena pointer (negative: inside the guard)."""
        self.arenas.torch.cuda.synchronize()
        lo, hi = GUARD + self.base, GUARD + self.base + self.size
        stray = [self.arenas.first_stray(t, (lo, hi)) for t in self.arenas.bufs]
        for t in self.arenas.bufs:
            t[lo:hi].fill_(PATTERN)
        for name, at in zip(("the arena's", "out's"), stray):
            if at is not None:
                x = at - GUARD
                raise AssertionError(
                    "%s allocation was written outside the window [%#x, %#x): first at %#x from the arena pointer "
                    "(the window's byte %d, were that byte's offset taken mod 2^32)" % (
                        name, self.base, self.base + self.size, x, (x - self.base) & 0xFFFFFFFF))
