"""Shared by the staging sweeps (test_staging_sweep.py on the CPU,
test_staging_sweep_gpu.py on the GPU): the layouts of requests that go through
the driver path (espgpu_process / flush / poll), what the oracle expects of
them, and the comparison.

The driver path puts xfer_copy (csrc/xfer_copy.h) in front of and behind the
crypto kernels: in the xfer kernel (256 threads per piece of at most 4096
bytes), in the self-staging prologue of the small-batch GCM kernels (64 down
to 2 threads per record, falling as the chunk's record count rises) and in
their epilogues (64 threads).  The copy picks its code from the source and
destination address mod 16 and mod 4, the length mod 16 and mod 4 and the
number of threads.  A record in registered memory is read in place (its start
residue is the source's on the way in and the destination's on the way out);
every other record is gathered to a 16-aligned place of the pinned staging
buffer first.  The layouts here say where each record lies and how long it is;
the rules of the engine they rest on (the small-batch bound, the chunk size
and the threads per record) are restated below and asserted of the layouts by
the CPU module, so a change of a rule shows up as lost coverage.

Every expectation is the oracle's: ciphertext and ICV for esp_output,
plaintext with the header and ICV left as given for esp_input, EBADMSG and an
untouched buffer for a record that fails its ICV, oracle.hmac for the AH
digests."""
import functools

import numpy as np

import oracle as O
from ah_helpers import BLOCK, AhSA
from helpers import EtaSA, GcmSA, build_records, oracle_decrypt

SKIP = 20                                    # outer IPv4 header in front of every ESP record
GUARD = 16                                   # zero bytes kept before the outer header and after the record
SMALL_BATCH = 128 << 10                      # espgpu.cpp kSmallBatchBytes: up to here a slot is a small batch
PIECE = 4096                                 # espgpu_internal.h kXferPiece

# ---------------------------------------------------------------------------
# the engine's rules, restated


def slot_stat_off(lens):
    """launch_slot's stat_off of a slot that holds records of these lengths
    (each at the next multiple of 16, 16 bytes of slack, the descriptors):
    the slot is a small batch while this is <= SMALL_BATCH."""
    return sum((int(L) + 15) & ~15 for L in lens) + 16 + 16 * len(lens)


def gcm_chunk(n, grid, burst):
    """launch_gcm's chunk size of an n-record small GCM batch on `grid`
    workgroups: from 4 (burst kernel) or 8 (fused small-batch kernel), doubled
    while below ceil(n / grid), at most 256."""
    chunk, per = (4 if burst else 8), (n + grid - 1) // grid
    while chunk < per and chunk < 256:
        chunk <<= 1
    return chunk


def stage_tpr(count, wg):
    """stage_in's threads per record for a chunk of `count` records in a
    workgroup of wg threads: the largest power of two <= 64 with
    tpr * count <= wg."""
    tpr = 64
    while tpr > 1 and tpr * count > wg:
        tpr >>= 1
    return tpr


WG = {"fused": 1024, "burst": 512}           # gcm_kernel<.., 1024, 8, true> / gcm_burst_kernel<.., 512, true>


def record_tpr(n, grid, kernel):
    """-> the threads per record that stage_in gives each of the n records."""
    chunk = gcm_chunk(n, grid, kernel == "burst")
    return [stage_tpr(min(chunk, n - (i // chunk) * chunk), WG[kernel]) for i in range(n)]


# ---------------------------------------------------------------------------
# ESP layouts

ESP_KINDS = {
    "gcm128-icv16": lambda rng: GcmSA(rng, 16),
    "gcm256-esn-icv12": lambda rng: GcmSA(rng, 32, esn=True, mlen=12),
    "cbc256-sha1": lambda rng: EtaSA(rng, 32),
    "ctr128-sha256-esn": lambda rng: EtaSA(rng, 16, ctr=True, sha=256, esn=True),
    "null-sha1": lambda rng: EtaSA(rng, null=True, sha=1),
    "cbc128-noauth": lambda rng: EtaSA(rng, 16, noauth=True),
    "cbc192-sha512": lambda rng: EtaSA(rng, 24, sha=512),
}


def is_cbc(kind):
    return kind.startswith("cbc")


def group_small(lens):
    """Consecutive records in groups that each stay a small batch."""
    groups, cur = [], []
    for i, L in enumerate(lens):
        if cur and slot_stat_off([lens[j] for j in cur] + [L]) > SMALL_BATCH:
            groups.append(cur)
            cur = []
        cur.append(i)
    if cur:
        groups.append(cur)
    return groups


class EspLayout:
    """ESP requests, built and encrypted by the oracle once, shared by the
    cases and never written to.
      kinds / sas:  the session kinds (names of ESP_KINDS) and their SAs
      sa / L:       per request: index into sas, record length
      registered:   the record lies in registered memory, its start at
                    reg_off (res = reg_off mod 16; the buffer is 16-aligned),
                    its outer header in the SKIP bytes before; else the packet
                    is a buffer of its own
      tampered:     one bit flipped in `bad`, the arena esp_input reads
      groups:       the requests of each slot (flushed and drained in turn)"""

    def __init__(self, name, rng, kinds, sa_idx, cts, registered, res, tamper, large=False):
        n = len(sa_idx)
        self.name, self.n, self.kinds, self.large = name, n, list(kinds), large
        self.sas = [ESP_KINDS[k](rng) for k in kinds]
        self.sa = np.asarray(sa_idx, dtype=np.int64)
        eh = rng.integers(0, 2**32, n, dtype=np.uint32)
        self.plain, self.ct, self.descs, self.eh = build_records(rng, self.sas, self.sa, np.asarray(cts), esn_hi=eh)
        self.L = self.descs["len"].astype(np.int64)
        self.off = self.descs["off4"].astype(np.int64) * 4
        self.registered = np.asarray(registered, dtype=bool)
        self.res = np.where(self.registered, np.asarray(res, dtype=np.int64), -1)
        self.hdr = rng.integers(1, 256, (n, SKIP), dtype=np.uint8)
        self.reg_off = np.full(n, -1, dtype=np.int64)
        pos = 64
        for i in np.nonzero(self.registered)[0]:
            s = pos + GUARD + SKIP
            s += (int(self.res[i]) - s) % 16
            self.reg_off[i] = s
            pos = s + int(self.L[i])
        self.reg_size = pos + 64
        self.bad = self.ct.copy()
        self.tampered = np.zeros(n, dtype=bool)
        for k, i in enumerate(tamper):
            sa = self.sas[self.sa[i]]
            o, L = int(self.off[i]), int(self.L[i])
            # the ICV's last bytes, or for every third (and a session without ICV) the payload's first byte
            at = o + sa.hlen if (k % 3 == 2 or not sa.mlen) else o + L - 1 - k % 4
            self.bad[at] ^= 1 << (k % 8)
            self.tampered[i] = True
        self.groups = [list(range(n))] if large else group_small(self.L)
        self._exp = {}
        for a in (self.plain, self.ct, self.bad, self.descs, self.L, self.off, self.registered, self.res, self.hdr,
                  self.reg_off, self.tampered):
            a.setflags(write=False)

    def sa_of(self, i):
        return self.sas[self.sa[i]]

    def where(self, i, path):
        i = int(i)
        return "request %d of %s: session %s, record of %d bytes (%d mod 16), %s, path %s" % (
            i, self.name, self.kinds[self.sa[i]], self.L[i], self.L[i] % 16,
            "registered, start residue %d" % self.res[i] if self.registered[i] else "staged", path)

    def source(self, encrypt):
        return self.plain if encrypt else self.bad

    def image(self, recs):
        """The registered buffer with every registered record's outer header
        and its bytes from `recs` (a list of bytes per request); zeros
        elsewhere."""
        img = np.zeros(self.reg_size, dtype=np.uint8)
        for i in np.nonzero(self.registered)[0]:
            s, L = int(self.reg_off[i]), int(self.L[i])
            img[s - SKIP:s] = self.hdr[i]
            img[s:s + L] = np.frombuffer(recs[i], dtype=np.uint8)
        return img

    def records(self, arena):
        return [arena[o:o + L].tobytes() for o, L in zip(self.off, self.L)]


def expect(lay, encrypt):
    """-> (crp_etype per request, the record's bytes afterwards per request),
    the oracle's, once per direction.  esp_output: the oracle's ciphertext and
    ICV.  esp_input over `bad`: where the oracle accepts, its plaintext
    between the header and the ICV as they were given; where it answers
    EBADMSG, the record as it was given."""
    if encrypt not in lay._exp:
        if encrypt:
            lay._exp[True] = (np.zeros(lay.n, dtype=np.int64), lay.records(lay.ct))
        else:
            dec, st = oracle_decrypt(lay.sas, lay.bad, lay.descs, lay.eh)
            recs = []
            for i in range(lay.n):
                sa, o, L = lay.sa_of(i), int(lay.off[i]), int(lay.L[i])
                if st[i] == 0:
                    recs.append(lay.bad[o:o + sa.hlen].tobytes() + dec[o + sa.hlen:o + L - sa.mlen].tobytes() +
                                lay.bad[o + L - sa.mlen:o + L].tobytes())
                else:
                    recs.append(lay.bad[o:o + L].tobytes())
            lay._exp[False] = (st.astype(np.int64), recs)
    return lay._exp[encrypt]


def _first_diff(a, b):
    return next((k for k, (x, y) in enumerate(zip(a, b)) if x != y), min(len(a), len(b)))


def run_esp(fw, drv, reg, ses, lay, path, encrypt):
    """One direction of lay through the driver (ses: a crypto_session per
    entry of lay.sas; reg: the registered buffer) and the comparison:
      * every crp_etype;
      * every byte of every packet buffer (outer header, header, payload, ICV);
      * the whole image of the registered buffer, so every byte between the
        packets -- at least GUARD zero bytes before each outer header and
        after each record -- is as it was;
      * stats()["zerocopy"] rose by the number of registered records.
    The first difference is named by lay.where."""
    from espgpu.esp import esp_input_crp, esp_output_crp
    assert reg.ctypes.data % 16 == 0 and lay.reg_size <= len(reg)
    src = lay.records(lay.source(encrypt))
    reg[:lay.reg_size] = lay.image(src)
    bufs = []
    for i in range(lay.n):
        if lay.registered[i]:
            s = int(lay.reg_off[i])
            bufs.append(reg[s - SKIP:s + int(lay.L[i])])
        else:
            bufs.append(bytearray(lay.hdr[i].tobytes() + src[i]))
    build = esp_output_crp if encrypt else esp_input_crp
    crps = [build(fw, ses[lay.sa[i]], lay.sa_of(i).esp_sa(), bufs[i], SKIP, esn_hi=int(lay.eh[i]))
            for i in range(lay.n)]
    z0 = drv.stats()["zerocopy"]
    for g in lay.groups:
        for i in g:
            assert fw.crypto_dispatch(crps[i]) == 0
        fw.crypto_drain()
    zc = drv.stats()["zerocopy"] - z0
    et, want = expect(lay, encrypt)
    what = "esp_output" if encrypt else "esp_input"
    for i in range(lay.n):
        assert crps[i].crp_etype == et[i], "%s: crp_etype %d, the oracle %d at %s" % (
            what, crps[i].crp_etype, et[i], lay.where(i, path))
        got, exp = bytes(bufs[i]), lay.hdr[i].tobytes() + want[i]
        assert got == exp, "%s: byte %d of the record differs (%d bytes differ) at %s" % (
            what, _first_diff(got, exp) - SKIP, sum(x != y for x, y in zip(got, exp)), lay.where(i, path))
    diff = np.nonzero(reg[:lay.reg_size] != lay.image(want))[0]
    if len(diff):
        regd = np.nonzero(lay.registered)[0]
        k = regd[max(int(np.searchsorted(lay.reg_off[regd], diff[0], side="right")) - 1, 0)]
        raise AssertionError("%s: registered memory written outside the packets, first %d bytes past the start of %s" % (
            what, diff[0] - lay.reg_off[k], lay.where(k, path)))
    assert zc == lay.registered.sum(), "%s: %d zero-copy records, %d registered (%s, path %s)" % (
        what, zc, lay.registered.sum(), lay.name, path)


# a. the xfer kernel: length mod 16 x start residue, every session kind

_LEN_STEPS = (0, 1, 5, 90)                   # 16-byte blocks added to the base payload, by residue


@functools.lru_cache(maxsize=None)
def esp_residues():
    """For every session kind, every record length mod 16 it can have (all of
    0, 4, 8, 12 for GCM, AES-CTR and ESP-NULL; one for AES-CBC, whose payload
    is whole blocks) and every start residue 0..15: one registered record;
    behind every fourth, a staged record of the same length.  A tenth of the
    decrypts are tampered."""
    rng = np.random.default_rng(9700)
    kinds = list(ESP_KINDS)
    sa_idx, cts, registered, res = [], [], [], []
    for k, kind in enumerate(kinds):
        sa = ESP_KINDS[kind](np.random.default_rng(0))
        for m in (0, 4, 8, 12):
            base = (m - sa.hlen - sa.mlen) % 16
            base = base if base else 16
            if is_cbc(kind) and base != 16:
                continue
            for r in range(16):
                ct = base + 16 * _LEN_STEPS[(r + m // 4 + k) % 4]
                sa_idx.append(k), cts.append(ct), registered.append(True), res.append(r)
                if r % 4 == (m // 4 + k) % 4:
                    sa_idx.append(k), cts.append(ct), registered.append(False), res.append(-1)
    n = len(sa_idx)
    tamper = [int(i) for i in rng.choice(n, n // 10, replace=False)]
    return EspLayout("a-residues", rng, kinds, sa_idx, cts, registered, res, tamper)


# b. records that span several pieces

PIECE_LENS = (4092, 4096, 4100, 8188, 8192, 8196, 65532)
PIECE_RES = (0, 1, 2, 3, 5, 15)
PIECE_KINDS = ("gcm128-icv16", "cbc256-sha1")


def piece_ct(kind, L):
    """The payload of a record of L bytes, or for AES-CBC (whole blocks) of
    the nearest length there is, the lower of two."""
    sa = ESP_KINDS[kind](np.random.default_rng(0))
    ct = L - sa.hlen - sa.mlen
    if is_cbc(kind):
        lo = ct // 16 * 16
        ct = lo if ct - lo <= lo + 16 - ct else lo + 16
    return ct


@functools.lru_cache(maxsize=None)
def esp_pieces(large):
    """PIECE_LENS for GCM and the nearest valid lengths for AES-CBC + HMAC,
    each registered at every residue of PIECE_RES.  large: the whole layout is
    one slot (a large batch); else slots that each stay a small batch."""
    rng = np.random.default_rng(9710)
    sa_idx, cts, res = [], [], []
    for r in PIECE_RES:
        for L in PIECE_LENS:
            for k, kind in enumerate(PIECE_KINDS):
                sa_idx.append(k), cts.append(piece_ct(kind, L)), res.append(r)
    n = len(sa_idx)
    tamper = [int(i) for i in rng.choice(n, n // 10, replace=False)]
    return EspLayout("b-pieces-large" if large else "b-pieces", rng, PIECE_KINDS, sa_idx, cts, [True] * n, res, tamper,
                     large=large)


# d. self-staging: threads per record

STAGE_SESSIONS = ("gcm128-icv16", "gcm256-esn-icv12")
STAGE_N = {"fused": (8, 16, 24, 40, 100, 200, 256, 300), "burst": (4, 8, 12, 24, 40, 100, 200, 256, 300)}
STAGE_SMALL_CT = (16, 4, 8, 12)
STAGE_LARGE_CT = (1456, 1444, 1448, 1452)           # the same record length mod 16 as STAGE_SMALL_CT, entry by entry
STAGE_MAX_LARGE = 60                         # long records per batch: the slot stays a small batch


@functools.lru_cache(maxsize=None)
def esp_stage(kind, n):
    """n records of one GCM session, one slot.  Payloads of STAGE_SMALL_CT
    and, for half the records drawn at random and at most STAGE_MAX_LARGE, of
    STAGE_LARGE_CT, so that the record length mod 16 takes 0, 4, 8 and 12.
    Every second record is registered, at residues 0..15 in turn (residue 0:
    both sides 16-aligned, as for the staged ones).  An eighth of the decrypts
    are tampered."""
    rng = np.random.default_rng(9720 + 1000 * STAGE_SESSIONS.index(kind) + n)
    nl = min(n // 2, STAGE_MAX_LARGE) if n >= 8 else 0
    big = np.zeros(n, dtype=bool)
    big[rng.choice(n, nl, replace=False)] = True
    # every eight consecutive records: each payload of its set once staged and once registered
    cts = [(STAGE_LARGE_CT if big[i] else STAGE_SMALL_CT)[(i // 2 if n >= 8 else i) % 4] for i in range(n)]
    registered = [i % 2 == 1 for i in range(n)]
    res = [(i // 2) % 16 for i in range(n)]
    tamper = [int(i) for i in rng.choice(n, max(1, n // 8), replace=False)]
    # (large=True: one slot; the CPU module asserts that it is a small batch)
    return EspLayout("d-stage-%s-n%d" % (kind, n), rng, [kind], [0] * n, [int(c) for c in cts], registered, res,
                     tamper, large=True)


# ---------------------------------------------------------------------------
# c. AH (DIGEST sessions) through the xfer kernel

AH_SESSIONS = [(1, False), (1, True), (512, False), (512, True)]
AH_IDS = ["sha1", "sha1-esn", "sha512", "sha512-esn"]
AH_LEAD = 16                                 # bytes of the request buffer before and after the hashed range
COMPUTE, VERIFY = 0x0, 0x2                   # CRYPTO_OP_COMPUTE_DIGEST, CRYPTO_OP_VERIFY_DIGEST (cryptodev.h)


class AhLayout:
    """Digest requests over byte ranges in registered memory: range i is L
    bytes at reg_off (res = reg_off mod 16), its digest field mlen bytes at
    doff (a multiple of 4) into it.  arena: the registered buffer before
    COMPUTE, random bytes in the ranges (the field too) and zeros between."""

    def __init__(self, rng, sha, esn):
        self.sha, self.esn = sha, esn
        self.sa = AhSA(rng, sha, esn=esn)
        m = self.sa.mlen
        lens = list(range(m, 2 * BLOCK[sha] + 9))
        L, res = [], []
        seen = {}
        for n_ in lens:
            j = seen.get(n_ % 16, 0)
            seen[n_ % 16] = j + 1
            for q in range(3):                # the j-th length of its class mod 16: residues 3j, 3j+1, 3j+2
                L.append(n_), res.append((3 * j + q) % 16)
        order = rng.permutation(len(L))
        self.L, self.res = np.array(L)[order], np.array(res)[order]
        self.n = len(L)
        self.doff = np.array([4 * int(rng.integers(0, (int(n_) - m) // 4 + 1)) for n_ in self.L])
        self.eh = rng.integers(0, 2**32, self.n, dtype=np.uint32)
        self.reg_off = np.zeros(self.n, dtype=np.int64)
        pos = 64
        for i in range(self.n):
            s = pos + AH_LEAD
            s += (int(self.res[i]) - s) % 16
            self.reg_off[i] = s
            pos = s + int(self.L[i])
        self.reg_size = pos + 64
        self.arena = np.zeros(self.reg_size, dtype=np.uint8)
        for i in range(self.n):
            s = int(self.reg_off[i])
            self.arena[s:s + int(self.L[i])] = rng.integers(0, 256, int(self.L[i]), dtype=np.uint8)
        self.tampered = np.zeros(self.n, dtype=bool)
        self.tampered[rng.choice(self.n, self.n // 10, replace=False)] = True
        self.groups = group_small(self.L + 2 * AH_LEAD)
        self._exp = None
        for a in (self.L, self.res, self.doff, self.eh, self.reg_off, self.arena, self.tampered):
            a.setflags(write=False)

    def where(self, i, path):
        i = int(i)
        return "request %d: AH HMAC-SHA%s%s, range of %d bytes (%d mod 16), registered, start residue %d, " \
               "digest at %d, path %s" % (i, {1: "1"}.get(self.sha, "2-%d" % self.sha), " ESN" if self.esn else "",
                                          self.L[i], self.L[i] % 16, self.res[i], self.doff[i], path)


@functools.lru_cache(maxsize=None)
def ah_layout(sha, esn):
    """Every byte length from mlen to two hash blocks + 8, each at three
    start residues chosen so that every pair (length mod 16, residue) occurs;
    shuffled."""
    return AhLayout(np.random.default_rng(9730 + sha + esn), sha, esn)


def ah_expect(lay):
    """-> (signed, bad, VERIFY's crp_etype over bad).  signed: arena after
    COMPUTE, each digest field holding the first mlen bytes of the HMAC of
    its range as it stood (swcr_authcompute hashes the field's bytes as they
    are), every other byte as it was.  bad: signed with one bit flipped in
    the tampered ranges.  VERIFY hashes the range as it stands, the field
    included, and compares with the field."""
    if lay._exp is None:
        signed = lay.arena.copy()
        for i in range(lay.n):
            s, L, d = int(lay.reg_off[i]), int(lay.L[i]), int(lay.doff[i])
            signed[s + d:s + d + lay.sa.mlen] = np.frombuffer(
                lay.sa.icv(lay.arena[s:s + L].tobytes(), int(lay.eh[i])), dtype=np.uint8)
        bad = signed.copy()
        for k, i in enumerate(np.nonzero(lay.tampered)[0]):
            bad[int(lay.reg_off[i]) + (k * 7) % int(lay.L[i])] ^= 1 << (k % 8)
        et = np.zeros(lay.n, dtype=np.int64)
        for i in range(lay.n):
            s, L, d = int(lay.reg_off[i]), int(lay.L[i]), int(lay.doff[i])
            if lay.sa.icv(bad[s:s + L].tobytes(), int(lay.eh[i])) != bad[s + d:s + d + lay.sa.mlen].tobytes():
                et[i] = O.EBADMSG
        for a in (signed, bad, et):
            a.setflags(write=False)
        lay._exp = (signed, bad, et)
    return lay._exp


def run_ah(fw, drv, reg, ses, lay, path, op):
    """COMPUTE over lay.arena or VERIFY over the signed, tampered buffer:
    every crp_etype, the whole registered buffer (COMPUTE writes the mlen
    digest bytes and nothing else, VERIFY nothing), the zero-copy count."""
    from espgpu import _lib as L
    signed, bad, vet = ah_expect(lay)
    src, want, et = (lay.arena, signed, np.zeros(lay.n, dtype=np.int64)) if op == COMPUTE else (bad, bad, vet)
    assert op == (L.CRYPTO_OP_COMPUTE_DIGEST if op == COMPUTE else L.CRYPTO_OP_VERIFY_DIGEST)
    assert reg.ctypes.data % 16 == 0 and lay.reg_size <= len(reg)
    reg[:lay.reg_size] = src
    crps = []
    for i in range(lay.n):
        s, n_ = int(lay.reg_off[i]), int(lay.L[i])
        crp = fw.crypto_getreq(ses)
        crp.crp_op, crp.crp_flags = op, L.CRYPTO_F_CBIFSYNC
        crp.crp_buf = reg[s - AH_LEAD:s + n_ + AH_LEAD]
        crp.crp_payload_start, crp.crp_payload_length = AH_LEAD, n_
        crp.crp_digest_start = AH_LEAD + int(lay.doff[i])
        crp.crp_esn = int(lay.eh[i]).to_bytes(4, "big")
        crps.append(crp)
    z0 = drv.stats()["zerocopy"]
    for g in lay.groups:
        for i in g:
            assert fw.crypto_dispatch(crps[i]) == 0
        fw.crypto_drain()
    zc = drv.stats()["zerocopy"] - z0
    what = "COMPUTE" if op == COMPUTE else "VERIFY"
    for i in range(lay.n):
        assert crps[i].crp_etype == et[i], "%s: crp_etype %d, expected %d at %s" % (
            what, crps[i].crp_etype, et[i], lay.where(i, path))
    diff = np.nonzero(reg[:lay.reg_size] != want)[0]
    if len(diff):
        k = max(int(np.searchsorted(lay.reg_off, diff[0], side="right")) - 1, 0)
        raise AssertionError("%s: %d bytes of registered memory differ, first %d bytes past the start of %s" % (
            what, len(diff), diff[0] - lay.reg_off[k], lay.where(k, path)))
    assert zc == lay.n, "%s: %d zero-copy records of %d (path %s)" % (what, zc, lay.n, path)


def aligned_zeros(nbytes):
    """A zeroed uint8 buffer whose address is a multiple of 64."""
    raw = np.zeros(nbytes + 64, dtype=np.uint8)
    o = (-raw.ctypes.data) % 64
    return raw[o:o + nbytes]
