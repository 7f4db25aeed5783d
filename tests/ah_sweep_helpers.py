"""Shared by the AH digest sweeps (test_ah_sweep.py on the CPU,
test_ah_sweep_gpu.py on the GPU): the length sets, the sessions, the batch
layouts and the comparison with oracle.hmac (AhSA.icv_hole / AhSA.icv).

esp_ah.hip's digest kernels choose their code from a record's byte length
(the ESN word and the 0x80 byte start at any byte of a dword; the padding
needs a block more past a residue that the ESN word moves), from where the
ICV field lies against the record's whole hash blocks and its tail, and from
the other records of the wave (the block loop runs to the wave's longest
message, the loads go quad by quad, both hashes of a width share a wave).
The layouts rest on how a caller-grouped batch maps records to waves: 64
consecutive descriptors are one unit.  They arrange by that and do not
assert it.

What a layout is made of is told here in the message's own terms (SHA
padding, byte offsets), never in the kernel's: total_blocks and field_class
know nothing of msg_word or nfull."""
import functools
import math

import numpy as np

from ah_helpers import BLOCK, DESC, AhSA

EINVAL, EBADMSG = 22, 74
TR_VALID = 0x80000000
UNIT = 64                                    # records per wave unit
SHAS = (1, 256, 384, 512)
HASH_ESN = [(sha, esn) for sha in SHAS for esn in (False, True)]
HASH_ESN_IDS = ["sha%d%s" % (sha, "-esn" if esn else "") for sha, esn in HASH_ESN]
MLEN = {1: 12, 256: 16, 384: 24, 512: 32}    # xform_ah_authsize
HASHSIZE = {1: 20, 256: 32, 384: 48, 512: 64}
MIXED_UNITS = 32

LONG_LENS = list(range(1480, 1521)) + list(range(8990, 9011)) + list(range(65400, 65536))


def dense_lens(sha, mlen=None):
    """Every byte length from the record that is its ICV field alone up to
    four hash blocks and 8 bytes."""
    return list(range(MLEN[sha] if mlen is None else mlen, 4 * BLOCK[sha] + 9))


def total_blocks(sha, esn, L):
    """Hash blocks of the inner message rec[0, L) || be32(esn_hi)? after the
    SHA padding (0x80, zeros, a 64- or 128-bit length), the key block not
    counted."""
    blk = BLOCK[sha]
    return (L + (4 if esn else 0) + 1 + blk // 8 + blk - 1) // blk


def key_lens(sha):
    """HMAC key lengths around the block: a key longer than the block is
    hashed first."""
    blk = BLOCK[sha]
    return [1, HASHSIZE[sha], blk - 1, blk, blk + 1, 2 * blk + 7]


FIELD_CLASSES = ("whole", "two-whole", "whole-tail", "tail")


def field_class(sha, L, salt, mlen):
    """Where the field [salt, salt + mlen) lies against the record's whole
    hash blocks (those that end inside the L record bytes) and its tail (the
    rest, hashed together with the ESN word and the padding): in one whole
    block, across two whole blocks, across the last whole block and the tail,
    or in the tail.  -> (the class, whether the field ends exactly at L)."""
    blk = BLOCK[sha]
    whole = L // blk
    first, last = salt // blk, (salt + mlen - 1) // blk
    if first >= whole:
        c = "tail"
    elif last >= whole:
        c = "whole-tail"
    else:
        c = "whole" if first == last else "two-whole"
    return c, salt + mlen == L


def make_sa(rng, sha, esn=False, mlen=None, aklen=None):
    """An AhSA; mlen 0 is csp_auth_mlen = 0, the whole hash."""
    sa = AhSA(rng, sha, esn=esn, mlen=mlen or None, aklen=aklen)
    if mlen == 0:
        sa.sa.mlen, sa.mlen = 0, HASHSIZE[sha]
    return sa


# ---------------------------------------------------------------------------
# a layout and its reference

BAD_KINDS = ("len0", "short", "salt-odd", "salt-past", "salt-big", "orphan", "freed")


class Layout:
    """Records of random bytes (the ICV field too) at 4-aligned offsets with
    random guard bytes between them, built once, shared by the cases and never
    written to.
      sas:       the AhSAs; descs["sa"] indexes them; freed_sas: the indexes
                 of sessions that are opened and freed again before a run
      L, salt:   what the descriptors say (malformed values in place)
      arena:     before signing
      tampered:  well-formed records with one flipped bit in `bad`
      malformed: kind per record ("" = well formed), every one EINVAL:
                 len 0, len < mlen, salt & 3 != 0, salt + mlen > len,
                 salt > 0xffff, session id 0xFFFF, a freed session"""

    def __init__(self, rng, sas, sa_idx, lens, salts, tamper=(), bad=None, freed_sas=()):
        n = len(lens)
        self.n, self.sas, self.freed_sas = n, sas, tuple(freed_sas)
        self.descs = np.zeros(n, dtype=DESC)
        self.kind = np.array([""] * n, dtype=object)
        pos = 16
        for i in range(n):
            self.descs[i] = (pos // 4, lens[i], sa_idx[i], 0, salts[i])
            pos += ((int(lens[i]) + 3) & ~3) + 4 * int(rng.integers(1, 5))
        self.descs["esn_hi"] = rng.integers(0, 2**32, n, dtype=np.uint32)
        self.arena = rng.integers(0, 256, pos + 64, dtype=np.uint8)
        for i, kind in (bad or {}).items():
            sa = sas[sa_idx[i]]
            L = int(lens[i])
            d = self.descs
            if kind == "len0":
                d["len"][i] = 0
            elif kind == "short":
                d["len"][i], d["salt"][i] = int(rng.integers(1, sa.mlen)), 0
            elif kind == "salt-odd":
                d["salt"][i] = int(salts[i]) + int(rng.integers(1, 4))
            elif kind == "salt-past":
                d["salt"][i] = ((L - sa.mlen) & ~3) + 4 * int(rng.integers(1, 3))
            elif kind == "salt-big":
                d["salt"][i] = 0x10000 + 4 * int(rng.integers(0, 8))
            elif kind == "freed":
                d["sa"][i] = self.freed_sas[int(rng.integers(0, len(self.freed_sas)))]
            else:
                assert kind == "orphan"
            self.kind[i] = kind
        self.malformed = self.kind != ""
        self.orphan = self.kind == "orphan"
        self.L = self.descs["len"].astype(np.int64)
        self.salt = self.descs["salt"].astype(np.int64)
        self.off = self.descs["off4"].astype(np.int64) * 4
        self.mlen = np.array([sas[s].mlen for s in self.descs["sa"]], dtype=np.int64)
        # (record, byte of the record, bit) of every flipped bit
        self.tamper = []
        for k, (i, w) in enumerate(tamper):
            if self.malformed[i]:
                continue
            L, s, m = int(self.L[i]), int(self.salt[i]), int(self.mlen[i])
            at = {"first": 0, "last": L - 1, "field": s + (i + k) % m}.get(w)
            self.tamper.append((int(i), int(rng.integers(0, L)) if at is None else at, k % 8))
        self.tampered = np.zeros(n, dtype=bool)
        self.tampered[[i for i, _, _ in self.tamper]] = True
        self._ref = None
        for a in (self.descs, self.arena, self.malformed, self.orphan, self.tampered):
            a.setflags(write=False)

    def sa_of(self, i):
        return self.sas[self.descs["sa"][i]]

    def where(self, i):
        i = int(i)
        sa = self.sa_of(i)
        return "record %d (64-unit %d lane %d): L %d, salt %d, HMAC-SHA%s with %d ICV bytes, ESN %s%s" % (
            i, i // UNIT, i % UNIT, self.L[i], self.salt[i], {1: "1"}.get(sa.sha, "2-%d" % sa.sha), sa.mlen,
            "on" if sa.esn else "off", ", malformed: " + self.kind[i] if self.malformed[i] else "")

    def where_byte(self, pos):
        i = max(int(np.searchsorted(self.off, pos, side="right")) - 1, 0)
        return "byte %d, %d bytes into %s" % (pos, pos - self.off[i], self.where(i))


def reference(lay):
    """-> (signed, bad, status of a verify over bad), once per layout, by
    AhSA.icv_hole alone.
      signed: the arena after signing: every well-formed record's field holds
              the ICV of the record with the field read as zeros, every other
              byte as it was
      bad:    signed, with the tampered records' flipped bits
    Asserts first that the reference alone tells the record classes apart: a
    tampered record's stored ICV differs from icv_hole of its tampered bytes
    (an intact one's is icv_hole of its bytes by construction)."""
    if lay._ref is None:
        signed = lay.arena.copy()
        eh = lay.descs["esn_hi"]
        for i in np.nonzero(~lay.malformed)[0]:
            o, L, s, m = lay.off[i], lay.L[i], lay.salt[i], lay.mlen[i]
            icv = lay.sa_of(i).icv_hole(lay.arena[o:o + L].tobytes(), s, int(eh[i]))
            assert len(icv) == m
            signed[o + s:o + s + m] = np.frombuffer(icv, dtype=np.uint8)
        bad = signed.copy()
        for i, at, bit in lay.tamper:
            bad[lay.off[i] + at] ^= 1 << bit
        for i in np.nonzero(lay.tampered)[0]:
            o, L, s, m = lay.off[i], lay.L[i], lay.salt[i], lay.mlen[i]
            again = lay.sa_of(i).icv_hole(bad[o:o + L].tobytes(), s, int(eh[i]))
            assert again != bad[o + s:o + s + m].tobytes(), "the reference accepts a tampered " + lay.where(i)
        st = np.where(lay.malformed, EINVAL, np.where(lay.tampered, EBADMSG, 0)).astype(np.uint8)
        for a in (signed, bad, st):
            a.setflags(write=False)
        lay._ref = (signed, bad, st)
    return lay._ref


OUT_FILL = 0xA5
TRL_FILL = 0x5A5A5A5A
MODES = ["sign", "inplace", "outofplace"]


def check(drv, lay, sids, mode, grouped=True, place=None):
    """Run lay on the GPU and compare with the reference; nothing is left out:
      * sign (encrypt_batch): 0 for every well-formed record, EINVAL for the
        others; the whole arena equals `signed`, byte for byte;
      * inplace (decrypt_batch with trailer words): the statuses are 0,
        EBADMSG or EINVAL as the layout prescribes; the arena is unchanged;
      * outofplace: as inplace, and the prefilled `out` is unchanged;
      * both verifies: the prefilled trailer words are ESPGPU_TR_VALID for the
        accepted records and 0 for every other.  (Every record of these
        layouts names a DIGEST session or none at all; a record without a
        session is answered EINVAL with the trailer word 0, as for every
        other kind of session.)
    sids: the device's session id per entry of lay.sas.
    place (high_offset_helpers.Placed): the layout lies at place.base of a
    large arena, every off4 relocated; the same comparisons run on that window
    of the arena and of `out`, and place.finish() then requires every byte
    outside the window untouched."""
    if place is None:
        return _check(drv, lay, sids, mode, grouped, None)
    try:
        return _check(drv, lay, sids, mode, grouped, place)
    finally:
        place.finish()


def _check(drv, lay, sids, mode, grouped, place):
    import torch
    from espgpu.batch import decrypt_batch, encrypt_batch
    signed, bad, vst = reference(lay)
    sign = mode == "sign"
    src = lay.arena if sign else bad
    want_st = np.where(lay.malformed, EINVAL, 0).astype(np.uint8) if sign else vst
    want_arena = signed if sign else bad
    d = lay.descs.copy()
    d["sa"] = [sids[s] for s in lay.descs["sa"]]
    d["sa"][lay.orphan] = 0xFFFF
    n = lay.n
    if place is None:
        arena = win = torch.from_numpy(np.array(src)).cuda()
    else:
        d = place.relocate(d)
        arena, win = place.load(src)               # win: the layout's bytes inside arena
    descs = torch.from_numpy(np.ascontiguousarray(d).view(np.uint8).copy()).cuda()
    st = torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda")
    trl = torch.from_numpy(np.full(n, TRL_FILL, dtype=np.uint32).view(np.int32)).cuda()
    out = None
    if sign:
        encrypt_batch(drv, arena, descs, n, st, grouped=grouped)
    elif mode == "inplace":
        decrypt_batch(drv, arena, descs, n, st, out=None, grouped=grouped, trailer=trl)
    else:
        out, owin = (torch.full_like(arena, OUT_FILL),) * 2 if place is None else place.out(OUT_FILL)
        decrypt_batch(drv, arena, descs, n, st, out=out, grouped=grouped, trailer=trl)
    torch.cuda.synchronize()
    got = st.cpu().numpy()
    wrong = np.nonzero(got != want_st)[0]
    assert not len(wrong), "%s: %d statuses differ (lengths %s), first: got %d, expected %d at %s" % (
        mode, len(wrong), sorted({int(lay.L[i]) for i in wrong})[:24], got[wrong[0]], want_st[wrong[0]],
        lay.where(wrong[0]))
    diff = win.cpu().numpy() != want_arena
    assert not diff.any(), "%s: %d bytes of the arena differ, first at %s" % (
        mode, int(diff.sum()), lay.where_byte(int(np.argmax(diff))))
    if out is not None:
        diff = owin.cpu().numpy() != OUT_FILL
        assert not diff.any(), "out was written at " + lay.where_byte(int(np.argmax(diff)))
    if not sign:
        gt = trl.cpu().numpy().view(np.uint32)
        want_trl = np.where(want_st == 0, TR_VALID, 0).astype(np.uint32)
        wrong = np.nonzero(gt != want_trl)[0]
        assert not len(wrong), "%s: %d trailer words differ, first: got %#x, expected %#x at %s" % (
            mode, len(wrong), gt[wrong[0]], want_trl[wrong[0]], lay.where(wrong[0]))
    return want_st


# ---------------------------------------------------------------------------
# uniform units: 64 records of one length

def _salt_walk(u, L, mlen):
    """The 64 salts of unit u: the multiples of 4 in [0, (L - mlen) & ~3],
    from a start and with a stride that rotate with u (1 where the stride
    would not reach every salt)."""
    ns = ((L - mlen) & ~3) // 4 + 1
    start, stride = (29 * u) % ns, (1, 3, 2, 5)[u % 4]
    if math.gcd(stride, ns) != 1:
        stride = 1
    return [4 * ((start + stride * k) % ns) for k in range(UNIT)]


def unit_lens(sha):
    """dense_lens(sha) in the order of the uniform units: ascending, but in
    every eight the 5th and 6th and the 7th and 8th change places, so that
    the odd units (and the even ones) hold every L & 3."""
    lens = dense_lens(sha)
    for g in range(0, len(lens) - 7, 8):
        lens[g + 4], lens[g + 5], lens[g + 6], lens[g + 7] = lens[g + 5], lens[g + 4], lens[g + 7], lens[g + 6]
    return lens


@functools.lru_cache(maxsize=2)
def uniform(sha, esn):
    """unit_lens(sha), 64 consecutive records each, the salts by _salt_walk.
    Even units are intact; in odd units three records at rotating lanes are
    tampered (byte 0, byte L - 1: the partial dword when L & 3 != 0, and one
    byte of the field), so the accepted lanes are no prefix of the unit."""
    rng = np.random.default_rng(9100 + 2 * SHAS.index(sha) + esn)
    sa = make_sa(rng, sha, esn)
    lens = unit_lens(sha)
    Ls = np.repeat(lens, UNIT)
    salts = [s for u, L in enumerate(lens) for s in _salt_walk(u, L, sa.mlen)]
    tamper = []
    for u in range(1, len(lens), 2):
        a = (u // 2) % UNIT
        tamper += [(u * UNIT + (a + 21 * k) % UNIT, w) for k, w in enumerate(("first", "last", "field"))]
    return Layout(rng, [sa], np.zeros(len(Ls), dtype=np.int64), Ls, salts, tamper)


# ---------------------------------------------------------------------------
# mixed units: the composition of each unit prescribed, seeded

def _any_salt(rng, L, mlen):
    return 4 * int(rng.integers(0, ((L - mlen) & ~3) // 4 + 1))


def _len_of(rng, sha, esn, mlen, t, r):
    """A length of t total blocks with L & 3 == r, at least the field."""
    blk = BLOCK[sha]
    c = (4 if esn else 0) + 1 + blk // 8
    cand = [L for L in range(max(mlen, (t - 1) * blk - c + 1), t * blk - c + 1) if L & 3 == r]
    return int(rng.choice(cand))


@functools.lru_cache(maxsize=None)
def quads(sha, esn):
    """j-quads: the four records of every quad have four different total
    block counts (of 1..8) and four different L & 3; which position holds
    which rotates from quad to quad.  One record tampered in every third
    unit."""
    rng = np.random.default_rng(9200 + 2 * SHAS.index(sha) + esn)
    sa = make_sa(rng, sha, esn)
    Ls = []
    for q in range(MIXED_UNITS * UNIT // 4):
        ts = sorted(rng.choice(np.arange(1, 9), 4, replace=False))
        Ls += [_len_of(rng, sha, esn, sa.mlen, int(ts[(k + q // 4) % 4]), (k + q) % 4) for k in range(4)]
    salts = [_any_salt(rng, L, sa.mlen) for L in Ls]
    tamper = [(u * UNIT + (5 * u) % UNIT, ("last", "field", "first")[u % 3]) for u in range(0, MIXED_UNITS, 3)]
    return Layout(rng, [sa], np.zeros(len(Ls), dtype=np.int64), Ls, salts, tamper)


@functools.lru_cache(maxsize=None)
def one_long(sha, esn):
    """k-one-long: one record of LONG_LENS (65535 among them) at lane u mod
    64 of unit u, so at each of the four quad positions in turn; the other 63
    records are one block or shorter.  The wave's block loop runs far past
    the end of most lanes.  The long record is tampered in every fifth unit,
    a short one in every seventh."""
    rng = np.random.default_rng(9300 + 2 * SHAS.index(sha) + esn)
    sa = make_sa(rng, sha, esn)
    short = [L for L in dense_lens(sha) if total_blocks(sha, esn, L) == 1]
    Ls = rng.choice(short, MIXED_UNITS * UNIT)
    long = rng.choice([L for L in LONG_LENS if L != 65535], MIXED_UNITS, replace=False)
    long[5] = 65535
    Ls[[u * UNIT + u for u in range(MIXED_UNITS)]] = long
    salts = [_any_salt(rng, int(L), sa.mlen) for L in Ls]
    tamper = [(u * UNIT + u, ("last", "any", "first")[u % 3]) for u in range(0, MIXED_UNITS, 5)]
    tamper += [(u * UNIT + (u + 9) % UNIT, "any") for u in range(0, MIXED_UNITS, 7)]
    return Layout(rng, [sa], np.zeros(len(Ls), dtype=np.int64), Ls, salts, tamper)


# wide and narrow in turn, so every four neighbours of the cyclic order hold
# both: (sha, esn, mlen); mlen 0 is csp_auth_mlen = 0
L_SESSIONS = [(384, False, None), (1, False, None), (512, False, None), (256, False, None), (384, True, None),
              (1, True, None), (512, True, None), (256, True, None), (512, False, 64), (1, True, 20),
              (384, True, 0)]


@functools.lru_cache(maxsize=None)
def hashes():
    """l-hashes: SHA-1, SHA2-256, SHA2-384 and SHA2-512 sessions, ESN and
    not, and three with another ICV size (SHA-1 with 20 bytes, SHA2-512 with
    64, SHA2-384 with csp_auth_mlen = 0), interleaved lane by lane, the order
    rotating from unit to unit: both launches see lanes that are not theirs
    inside every quad, the narrow launch runs both of its passes over every
    wave, the wide one mixes SHA2-384 and SHA2-512 lane by lane.  Random
    lengths of each hash's dense set, 5 % tampered anywhere."""
    rng = np.random.default_rng(9400)
    sas = [make_sa(rng, sha, esn, mlen) for sha, esn, mlen in L_SESSIONS]
    n = MIXED_UNITS * UNIT
    sa_idx = np.array([(i % UNIT + i // UNIT) % len(sas) for i in range(n)])
    Ls = [int(rng.choice(dense_lens(sas[s].sha, sas[s].mlen))) for s in sa_idx]
    salts = [_any_salt(rng, L, sas[s].mlen) for L, s in zip(Ls, sa_idx)]
    tamper = [(int(i), "any") for i in np.nonzero(rng.random(n) < 0.05)[0]]
    return Layout(rng, sas, sa_idx, Ls, salts, tamper)


@functools.lru_cache(maxsize=None)
def random_mix():
    """m-random: random draws from the dense sets of all four hashes (ESN and
    not), 20 malformed records of each of BAD_KINDS, about 5 % of the records
    tampered anywhere, and a partial last unit."""
    rng = np.random.default_rng(9500)
    sas = [make_sa(rng, sha, esn) for sha, esn in HASH_ESN] + [make_sa(rng, 256), make_sa(rng, 512, True)]
    freed = (len(sas) - 2, len(sas) - 1)
    n = MIXED_UNITS * UNIT - 27
    sa_idx = rng.integers(0, len(HASH_ESN), n)
    Ls = [int(rng.choice(dense_lens(sas[s].sha))) for s in sa_idx]
    salts = [_any_salt(rng, L, sas[s].mlen) for L, s in zip(Ls, sa_idx)]
    picks = rng.choice(n - 1, 20 * len(BAD_KINDS), replace=False)
    bad = {int(i): BAD_KINDS[k // 20] for k, i in enumerate(picks)}
    bad[n - 1] = "salt-past"                               # in the last, partial unit
    tamper = [(int(i), "any") for i in np.nonzero(rng.random(n) < 0.05)[0]]
    return Layout(rng, sas, sa_idx, Ls, salts, tamper, bad=bad, freed_sas=freed)


# ---------------------------------------------------------------------------
# HMAC key lengths

def key_rec_lens(sha, mlen):
    return [mlen, BLOCK[sha] - 9, BLOCK[sha], 2 * BLOCK[sha] + 3]


@functools.lru_cache(maxsize=None)
def key_lengths():
    """One session per hash and key length of key_lens (24 sessions, fresh
    random keys, ESN on every second), each with four records of mlen,
    blk - 9, blk and 2 * blk + 3 bytes; the last two tampered in every third
    session."""
    rng = np.random.default_rng(9600)
    sas, sa_idx, Ls = [], [], []
    for sha in SHAS:
        for kl in key_lens(sha):
            sas.append(make_sa(rng, sha, esn=len(sas) % 2 == 1, aklen=kl))
            assert len(sas[-1].key) == kl
            Ls += key_rec_lens(sha, sas[-1].mlen)
            sa_idx += [len(sas) - 1] * 4
    salts = [_any_salt(rng, L, sas[s].mlen) for L, s in zip(Ls, sa_idx)]
    tamper = [(4 * s + k, "any") for s in range(0, len(sas), 3) for k in (2, 3)]
    return Layout(rng, sas, np.array(sa_idx), Ls, salts, tamper)
