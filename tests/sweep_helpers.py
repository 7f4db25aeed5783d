"""Shared by the payload-length sweeps (test_length_sweep.py on the CPU,
test_length_sweep_gpu.py and test_long_records_gpu.py on the GPU): the length
sets, the session kinds, the batch layouts and the comparison with the oracle.

The kernels choose their code path from a record's length and from the
lengths of the other records of its wave: the GCM kernels through the wave
maxima of their step counts and the 4-lane kernel's aligned schedule (every
record of the wave with nct + 1 a multiple of 4, nct = its ciphertext
blocks), the ETA kernels through wave-uniform trip counts, the quad
transposes (four records per load) and the equal-length fast path of the
verified decrypt.  The layouts here rest on how a caller-grouped batch
(implicit chunks) maps records to waves: 16 consecutive descriptors are one
wave of the 4-lane GCM kernel (8 of the 8-lane one), 64 consecutive
descriptors one ETA wave unit.  They arrange by that and do not assert it.

The comparison is the byte-for-byte rule of test_gcm_waits_gpu.py (_oracle
and _payload_mask live here and are imported there), extended by the trailer
words and a prefilled `out`."""
import functools

import numpy as np

import oracle as O
from helpers import EtaSA, GcmSA, build_records

# ---------------------------------------------------------------------------
# length sets

GCM_LENS = [L for L in range(0, 8225, 4) if L <= 2112 or 4032 <= L <= 4128 or 8128 <= L <= 8224]
CBC_LENS = [16 * nb for nb in range(69)]
CTR_LENS = list(range(0, 1089, 4))           # AES-CTR and ESP-NULL

GCM_RUN = 16                                 # records of one length (one wave of the 4-lane kernel)
ETA_UNIT = 64                                # records per ETA wave unit

# (key bytes, ESN, ICV bytes)
GCM_SESSIONS = [(16, False, 16), (32, True, 12), (24, False, 8)]
GCM_SESSION_IDS = ["aes128-icv16", "aes256-esn-icv12", "aes192-icv8"]

ETA_KINDS = {
    "cbc128-sha1": dict(klen=16, sha=1),
    "cbc256-sha1-esn": dict(klen=32, sha=1, esn=True),
    "cbc192-sha256-esn": dict(klen=24, sha=256, esn=True),
    "cbc128-sha384": dict(klen=16, sha=384),
    "cbc256-sha512-esn": dict(klen=32, sha=512, esn=True),
    "cbc128-noauth": dict(klen=16, noauth=True),
    "ctr128-sha1-esn": dict(klen=16, ctr=True, sha=1, esn=True),
    "ctr256-sha256": dict(klen=32, ctr=True, sha=256),
    "ctr192-sha384-esn": dict(klen=24, ctr=True, sha=384, esn=True),
    "ctr128-sha512": dict(klen=16, ctr=True, sha=512),
    "null-sha1": dict(null=True, sha=1),
    "null-sha256-esn": dict(null=True, sha=256, esn=True),
    "null-sha512-esn": dict(null=True, sha=512, esn=True),
}
# the mixed-wave families run one kind per code path: the quad HMAC at both
# narrow hashes, the wide hash, the CBC chain alone, AES-CTR and ESP-NULL
MIXED_KINDS = ["cbc128-sha1", "cbc192-sha256-esn", "cbc256-sha512-esn", "cbc128-noauth", "ctr256-sha256",
               "null-sha1"]
HASH_BLOCK = {1: 64, 256: 64, 384: 128, 512: 128}


def eta_sa(rng, kind):
    return EtaSA(rng, **ETA_KINDS[kind])


def eta_lens(kind):
    return CBC_LENS if kind.startswith("cbc") else CTR_LENS


# --- long records: from jumbo size to the largest a descriptor carries -------

MAX_RECORD = 65532                           # len is 16 bits and a multiple of 4
LONG_ARENA_CAP = 48 << 20                    # every long layout's arena stays below this


def gcm_ctr_edge(k):
    """The GCM counter cache (esp_gcm.hip ctr_cache_build) is keyed on
    ctr >> 8 and CT block i uses counter i + 2: block 256 k - 2 is the first
    of key k, and it starts at this payload byte."""
    return 4096 * k - 32


GCM_LONG_KEYS = [3, 4, 7, 8, 15]             # each of the key's four bits on and off
GCM_JUMBO = list(range(8936, 8961, 4))


def gcm_top(mlen):
    """The largest GCM payload of a session with mlen ICV bytes."""
    return MAX_RECORD - 16 - mlen


def GCM_LONG_LENS(mlen):
    """Around the key changes of GCM_LONG_KEYS every multiple of 4 in
    [c_k - 16, c_k + 32] (the last block on either side of the change, at
    every last-block size), the jumbo window, and the 13 largest payloads."""
    lens = [L for k in GCM_LONG_KEYS for L in range(gcm_ctr_edge(k) - 16, gcm_ctr_edge(k) + 33, 4)]
    top = gcm_top(mlen)
    return sorted(lens + GCM_JUMBO + list(range(top - 48, top + 1, 4)))


def gcm_j0_back_key(L):
    """The 4-lane kernel's aligned schedule (a wave whose records all have
    nct + 1 a multiple of 4) deals the counter blocks out densely and gives
    E_K(J0), counter 1, the LAST slot: slot nct, in lane 3 after that lane's CT
    block nct - 4.  It is the one place where a lane's counter goes back, from
    this key to key 0 (every other schedule and kernel starts with J0 and
    counts up).  None for a length the schedule does not take."""
    nct = gcm_nct(L)
    return (nct - 2) >> 8 if gcm_aligned(L) and nct >= 4 else None


def GCM_LONG_ALIGNED():
    """nct = 256 k + 3 for the k of GCM_LONG_KEYS, the last block of 4 and of
    16 bytes: aligned records whose J0 lane steps back from key k.  In
    GCM_LONG_LENS the aligned lengths just past c_k have nct = 256 k - 1, and
    that lane is still under key k - 1."""
    return [16 * (256 * k + 3) - cut for k in GCM_LONG_KEYS for cut in (12, 0)]


def gcm_ctr_keys(L):
    """(the ctr >> 8 values a payload of L bytes runs through, the last CT
    block's)."""
    last = (gcm_nct(L) + 1) >> 8
    return list(range(last + 1)), last


def eta_hlen_mlen(kind):
    """(header bytes in front of the payload, ICV bytes) of a kind, as EtaSA
    has them."""
    k = ETA_KINDS[kind]
    hlen = 16 if k.get("ctr") else 8 if k.get("null") else 24
    return hlen, 0 if k.get("noauth") else {1: 12, 256: 16, 384: 24, 512: 32}[k["sha"]]


def eta_top(kind):
    """The kind's largest payload: whole blocks for CBC."""
    hlen, mlen = eta_hlen_mlen(kind)
    room = MAX_RECORD - hlen - mlen
    return room // 16 * 16 if kind.startswith("cbc") else room


CBC_LONG_NB = list(range(556, 564)) + [1024, 2048]


def CBC_LONG_LENS(kind):
    """Eight consecutive block counts at jumbo size (every residue mod 128 of
    the hashed length), 1024 and 2048 blocks, and the eight largest."""
    nbmax = eta_top(kind) // 16
    return [16 * nb for nb in CBC_LONG_NB + list(range(nbmax - 7, nbmax + 1))]


def CTR_LONG_LENS(kind):
    """AES-CTR and ESP-NULL: every multiple of 4 in the jumbo window, one
    past 16 KiB and one short of 32 KiB, and the eight largest."""
    top = eta_top(kind)
    return list(range(8936, 8965, 4)) + [16388, 32764] + list(range(top - 28, top + 1, 4))


def eta_long_lens(kind):
    return CBC_LONG_LENS(kind) if kind.startswith("cbc") else CTR_LONG_LENS(kind)


def arena_bytes(rec_lens, stride_pad=0):
    """The arena helpers.build_records lays out for records of these lengths
    (header and ICV included)."""
    return sum(((int(L) + 3) & ~3) + stride_pad for L in rec_lens) + 64


# what the GCM kernels derive from a payload length (esp_gcm.hip do_group)
def gcm_nct(L):
    return (L + 15) // 16


def gcm_shape(L, S):
    """(M, pad, last-block bytes) of a payload of L > 0 bytes at S lanes per
    record: N = nct + 2 GHASH blocks, M steps per lane, pad zero blocks in
    front."""
    nct = gcm_nct(L)
    N = nct + 2
    M = (N + S - 1) // S
    return M, S * M - N, L - 16 * (nct - 1)


def gcm_aligned(L):
    """The 4-lane kernel's aligned schedule takes a wave whose records all
    have this."""
    return L > 0 and (gcm_nct(L) + 1) % 4 == 0


# ---------------------------------------------------------------------------
# the oracle's side of the comparison

def _oracle(sas, arena, descs, eh, keep, encrypt=False):
    """The oracle over the records in `keep` (a bool per record), in a copy of
    arena.  -> (arena after, one status per record; EINVAL where not kept)."""
    out = arena.copy()
    idx = np.nonzero(keep)[0]
    st = np.full(len(descs), O.EINVAL, dtype=np.uint8)
    _, s = O.batch([x.oracle for x in sas], out, descs["off4"][idx], descs["len"][idx], descs["sa"][idx],
                   esn_hi=eh[idx], nthreads=8, encrypt=encrypt)
    if encrypt:
        # the oracle's encrypt reports no status: the records it refused are
        # those it left untouched (an encrypted record gains at least its ICV)
        for i in idx:
            o, L = int(descs["off4"][i]) * 4, max(int(descs["len"][i]), 32)
            st[i] = O.EINVAL if (out[o:o + L] == arena[o:o + L]).all() else 0
    else:
        st[idx] = s
    return out, st


def _payload_mask(descs, which, size, sas):
    m = np.zeros(size, dtype=bool)
    for i in np.nonzero(which)[0]:
        o, L = int(descs["off4"][i]) * 4, int(descs["len"][i])
        m[o + sas[descs["sa"][i]].hlen:o + L - sas[descs["sa"][i]].mlen] = True
    return m


class Batch:
    """One layout: records built and encrypted by the oracle once, shared by
    the cases and never written to.
      plain / bad: the arena before encryption / after it, with the tampered
                   records' flipped bits
      descs:       sa indexes sas; malformed lengths already in place
      tampered:    records with a flipped bit (all well formed)
      malformed:   records every side must refuse (EINVAL): bad lengths,
                   `foreign` (another session's id inside a caller-grouped
                   GCM chunk: the engine's own rule, so the oracle is run
                   without them) and `orphan` (session id 0xFFFF on the
                   device, no such session)"""

    def __init__(self, sas, plain, bad, descs, eh, tampered, malformed, foreign, orphan):
        self.sas, self.plain, self.bad, self.descs, self.eh = sas, plain, bad, descs, eh
        self.tampered, self.malformed, self.foreign, self.orphan = tampered, malformed, foreign, orphan
        self.n = len(descs)
        for a in (plain, bad, descs, eh, tampered, malformed, foreign, orphan):
            a.setflags(write=False)
        self._exp = {}

    def payload(self, i):
        sa = self.sas[self.descs["sa"][i]]
        return int(self.descs["len"][i]) - sa.hlen - sa.mlen

    def where(self, i):
        i = int(i)
        return "record %d (16-run %d lane %d, 64-unit %d lane %d): payload %d bytes, session %d" % (
            i, i // GCM_RUN, i % GCM_RUN, i // ETA_UNIT, i % ETA_UNIT, self.payload(i), self.descs["sa"][i])

    def where_byte(self, pos):
        i = int(np.searchsorted(self.descs["off4"].astype(np.int64) * 4, pos, side="right")) - 1
        return "byte %d, %d bytes into %s" % (pos, pos - int(self.descs["off4"][i]) * 4, self.where(i))


def make_batch(rng, sas, sa_idx, cts, tamper=(), stride_pad=0, len_delta=None, foreign=None, orphan=None):
    """tamper: (record, where) pairs, where = "first" / "last" payload byte,
    "icv" (the last ICV byte the session keeps; without auth the last payload
    byte) or "any" (a random byte of the record).  len_delta: {record: bytes
    added to the descriptor's len after the build} (a malformed length).
    foreign: {record: index in sas of the session whose id it carries}."""
    n = len(sa_idx)
    sa_idx = np.asarray(sa_idx, dtype=np.int64)
    cts = np.asarray(cts, dtype=np.int64)
    eh = rng.integers(0, 2**32, n, dtype=np.uint32)
    plain, ct, descs, eh = build_records(rng, sas, sa_idx, cts, esn_hi=eh, stride_pad=stride_pad)
    malformed = cts <= 0
    for i, dl in (len_delta or {}).items():
        descs["len"][i] = int(descs["len"][i]) + dl
        malformed[i] = True
    fmask, omask = np.zeros(n, dtype=bool), np.zeros(n, dtype=bool)
    for i, s in (foreign or {}).items():
        descs["sa"][i] = s
        fmask[i] = True
    for i in (orphan or ()):
        omask[i] = True
    malformed |= fmask | omask
    bad = ct.copy()
    tampered = np.zeros(n, dtype=bool)
    for k, (i, where) in enumerate(tamper):
        if malformed[i]:
            continue
        sa = sas[sa_idx[i]]
        o, L = int(descs["off4"][i]) * 4, int(descs["len"][i])
        pos = {"first": o + sa.hlen, "last": o + L - sa.mlen - 1, "icv": o + L - 1}.get(where)
        if pos is None:
            pos = o + int(rng.integers(0, L))
        bad[pos] ^= 1 << (k % 8)
        tampered[i] = True
    return Batch(sas, plain, bad, descs, np.asarray(eh), tampered, malformed, fmask, omask)


def expected(b, encrypt):
    """-> (the oracle's arena, statuses, trailer words) for b, once per
    direction.  Asserts first that the oracle alone tells the layout's record
    classes apart: EINVAL for every malformed record, EBADMSG for every
    tampered one (0 for a session without auth, which decrypts whatever it
    gets), 0 for every other."""
    from espgpu.esp import trailer_word
    if encrypt not in b._exp:
        ref, st = _oracle(b.sas, b.plain if encrypt else b.bad, b.descs, b.eh, ~(b.foreign | b.orphan),
                          encrypt=encrypt)
        auth = np.array([s.mlen > 0 for s in b.sas])[b.descs["sa"]]
        want = np.where(b.malformed, O.EINVAL, np.where(b.tampered & auth & (not encrypt), O.EBADMSG, 0))
        wrong = np.nonzero(st != want)[0]
        assert not len(wrong), "the oracle answers %d, the layout expects %d: %s" % (
            st[wrong[0]], want[wrong[0]], b.where(wrong[0]))
        trl = np.zeros(b.n, dtype=np.uint32)
        if not encrypt:
            for i in np.nonzero(st == 0)[0]:
                sa = b.sas[b.descs["sa"][i]]
                o, L = int(b.descs["off4"][i]) * 4, int(b.descs["len"][i])
                trl[i] = trailer_word(ref[o + sa.hlen:o + L - sa.mlen])
        for a in (ref, st, trl):
            a.setflags(write=False)
        b._exp[encrypt] = (ref, st, trl)
    return b._exp[encrypt]


OUT_FILL = 0xA5
TRL_FILL = 0xEEEEEEEE


def check(drv, b, sids, mode, grouped=True, place=None):
    """Run b on the GPU (mode: "outofplace", "inplace" or "encrypt") and
    compare with the oracle:
      * statuses equal for every record;
      * in place and encrypt: the whole arena equals the oracle's, byte for
        byte (guard bytes, rejected records);
      * out of place: the arena unchanged; `out`, prefilled, holds the
        oracle's plaintext on every verified record's payload span and its
        prefill everywhere else.  The payload span of a record that failed
        its ICV is left out: unspecified for GCM (the single pass has written
        unverified plaintext there), and for the ETA kernels include/espgpu.h
        promises an untouched failed record only in place, not that an
        out-of-place verify-first decrypt writes nothing;
      * decrypt: trailer words (prefilled) equal esp.trailer_word of the
        oracle's plaintext for verified records, 0 for every other.
    place (high_offset_helpers.Placed): the layout lies at place.base of a
    large arena, every off4 relocated; the same comparisons run on that window
    of the arena and of `out`, and place.finish() then requires every byte
    outside the window untouched."""
    if place is None:
        return _check(drv, b, sids, mode, grouped, None)
    try:
        return _check(drv, b, sids, mode, grouped, place)
    finally:
        place.finish()


def _check(drv, b, sids, mode, grouped, place):
    import torch
    from espgpu.batch import decrypt_batch, encrypt_batch
    enc = mode == "encrypt"
    ref, ref_st, ref_trl = expected(b, enc)
    src = b.plain if enc else b.bad
    d = b.descs.copy()
    d["sa"] = [sids[s] for s in b.descs["sa"]]
    d["sa"][b.orphan] = 0xFFFF
    n = b.n
    if place is None:
        arena = win = torch.from_numpy(np.array(src)).cuda()
    else:
        d = place.relocate(d)
        arena, win = place.load(src)               # win: the layout's bytes inside arena
    descs = torch.from_numpy(np.ascontiguousarray(d).view(np.uint8).copy()).cuda()
    st = torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda")
    trl = torch.from_numpy(np.full(n, TRL_FILL, dtype=np.uint32).view(np.int32)).cuda()
    out = None
    if enc:
        encrypt_batch(drv, arena, descs, n, st, grouped=grouped)
    elif mode == "inplace":
        decrypt_batch(drv, arena, descs, n, st, out=None, grouped=grouped, trailer=trl)
    else:
        out, owin = (torch.full_like(arena, OUT_FILL),) * 2 if place is None else place.out(OUT_FILL)
        decrypt_batch(drv, arena, descs, n, st, out=out, grouped=grouped, trailer=trl)
    torch.cuda.synchronize()
    got = st.cpu().numpy()
    wrong = np.nonzero(got != ref_st)[0]
    assert not len(wrong), "%d statuses differ (payload lengths %s), first: got %d, the oracle %d at %s" % (
        len(wrong), sorted({b.payload(i) for i in wrong})[:24], got[wrong[0]], ref_st[wrong[0]], b.where(wrong[0]))
    res = win.cpu().numpy()
    if mode == "outofplace":
        assert (res == src).all(), "out of place: the arena changed at " + b.where_byte(int(np.argmax(res != src)))
        want = np.full_like(src, OUT_FILL)
        okm = _payload_mask(b.descs, ref_st == 0, len(src), b.sas)
        want[okm] = ref[okm]
        care = ~_payload_mask(b.descs, ref_st == O.EBADMSG, len(src), b.sas)
        diff = (owin.cpu().numpy() != want) & care
        assert not diff.any(), "out differs at " + b.where_byte(int(np.argmax(diff)))
    else:
        diff = res != ref
        assert not diff.any(), "the arena differs at " + b.where_byte(int(np.argmax(diff)))
    if not enc:
        gt = trl.cpu().numpy().view(np.uint32)
        wrong = np.nonzero(gt != ref_trl)[0]
        assert not len(wrong), "%d trailer words differ, first: got %#x, expected %#x at %s" % (
            len(wrong), gt[wrong[0]], ref_trl[wrong[0]], b.where(wrong[0]))
    return ref_st


# ---------------------------------------------------------------------------
# uniform layouts: one length per wave

def _gcm_sa(rng, si):
    klen, esn, mlen = GCM_SESSIONS[si]
    return GcmSA(rng, klen, esn=esn, mlen=mlen)


@functools.lru_cache(maxsize=None)
def gcm_uniform(si):
    """GCM_LENS, 16 consecutive records each.  In every second 16-run two
    records are tampered, at lanes that rotate with the run: one in its last
    payload byte, one in the last ICV byte its session keeps."""
    rng = np.random.default_rng(8100 + si)
    cts = np.repeat(GCM_LENS, GCM_RUN)
    tamper = []
    for r in range(1, len(GCM_LENS), 2):
        a = (r // 2) % GCM_RUN
        b = (a + 1 + (r // 32) % (GCM_RUN - 1)) % GCM_RUN
        tamper += [(r * GCM_RUN + a, "last"), (r * GCM_RUN + b, "icv")]
    return make_batch(rng, [_gcm_sa(rng, si)], np.zeros(len(cts), dtype=np.int64), cts, tamper)


@functools.lru_cache(maxsize=2)
def eta_uniform(kind):
    """The kind's length set, 64 consecutive records each.  Even units are
    intact (the equal-length path of the verified decrypt); in odd units three
    records at rotating lanes are tampered (first payload byte, last payload
    byte, last ICV byte), so the verified lanes are no prefix of the unit."""
    rng = np.random.default_rng(8200 + list(ETA_KINDS).index(kind))
    lens = eta_lens(kind)
    cts = np.repeat(lens, ETA_UNIT)
    tamper = []
    for u in range(1, len(lens), 2):
        a = (u // 2) % ETA_UNIT
        tamper += [(u * ETA_UNIT + (a + 21 * k) % ETA_UNIT, w) for k, w in enumerate(("first", "last", "icv"))]
    return make_batch(rng, [eta_sa(rng, kind)], np.zeros(len(cts), dtype=np.int64), cts, tamper)


# ---------------------------------------------------------------------------
# mixed layouts: the composition of each wave prescribed, seeded

GCM_FAMILIES = ["a-aligned", "b-one-unaligned", "c-one-long", "d-ascending", "e-random"]
GCM_WAVES = 64
_ALIGNED_NCT = list(range(3, 132, 4))                     # 3, 7, ..., 131
_LONG_LENS = [L for L in GCM_LENS if L >= 4032] + [2112]


def _len_of(rng, nct):
    """A payload of nct blocks whose last block has 4, 8, 12 or 16 bytes."""
    return 16 * (nct - 1) + 4 * int(rng.integers(1, 5))


def gcm_family_lens(family, rng):
    """-> the payload lengths, one row of 16 per wave.
    a: every record aligned for the 4-lane kernel, block counts differing.
       Runs in turn: at least 4 distinct counts drawn at random; exactly one
       record at the maximum (its lane rotating); all but one at the maximum.
    b: as a, with one record (its lane rotating) of a block count that is
       not aligned: the whole wave takes the position schedule.
    c: one record from the counter windows or of 2112 bytes at a rotating
       lane, the others at most 64 bytes.
    d: block counts ascending by one across the run, the start swept."""
    rows = []
    for r in range(GCM_WAVES):
        if family in ("a-aligned", "b-one-unaligned"):
            if r % 3 == 0:
                ncts = list(rng.choice(_ALIGNED_NCT, 4 + r % 5, replace=False))
                ncts += list(rng.choice(ncts, GCM_RUN - len(ncts)))
                rng.shuffle(ncts)
            else:
                top = int(rng.choice(_ALIGNED_NCT[4:]))
                low = [x for x in _ALIGNED_NCT if x < top]
                if r % 3 == 1:
                    ncts = list(rng.choice(low, 3, replace=False)) + list(rng.choice(low, GCM_RUN - 4))
                    rng.shuffle(ncts)
                    ncts.insert(r % GCM_RUN, top)
                else:
                    ncts = [top] * (GCM_RUN - 1)
                    ncts.insert(r % GCM_RUN, int(rng.choice(low)))
            if family == "b-one-unaligned":
                ncts[(5 * r + 2) % GCM_RUN] += 1 + r % 3
            rows.append([_len_of(rng, int(x)) for x in ncts])
        elif family == "c-one-long":
            row = [4 * int(rng.integers(1, 17)) for _ in range(GCM_RUN)]
            row[(7 * r) % GCM_RUN] = _LONG_LENS[r % len(_LONG_LENS)]
            rows.append(row)
        else:
            rows.append([_len_of(rng, 1 + r + k) for k in range(GCM_RUN)])
    return np.array(rows)


@functools.lru_cache(maxsize=None)
def gcm_mixed(family):
    """One session per family (the three of GCM_SESSIONS in turn), guard bytes
    between the records.  a-d: 64 waves, one record tampered in every fourth.
    e: random draws from GCM_LENS (length 0 among them), some descriptors with
    len % 4 == 2 or another session's id, 5 % tampered, and 16 k + 5 records,
    so the last wave and chunk are partial."""
    f = GCM_FAMILIES.index(family)
    rng = np.random.default_rng(8300 + f)
    sas = [_gcm_sa(rng, f % 3), _gcm_sa(rng, (f + 1) % 3)]
    if family != "e-random":
        cts = gcm_family_lens(family, rng).reshape(-1)
        tamper = [(r * GCM_RUN + (3 * r) % GCM_RUN, ("last", "icv", "first")[r % 3])
                  for r in range(0, GCM_WAVES, 4)]
        return make_batch(rng, sas, np.zeros(len(cts), dtype=np.int64), cts, tamper, stride_pad=8)
    n = GCM_WAVES * GCM_RUN + 5
    cts = rng.choice(GCM_LENS, n)
    cts[rng.choice(n, 24, replace=False)] = 0
    # a chunk's first record names its session, and chunks are as few as four
    # records (launch_gcm): no foreign id at a multiple of four
    odd = np.array([i for i in range(n) if i % 4])
    picks = rng.choice(odd, 40, replace=False)
    foreign = {int(i): 1 for i in picks[:20]}
    len_delta = {int(i): 2 for i in picks[20:]}
    len_delta[n - 2] = 2                                  # in the last, partial wave
    tamper = [(int(i), "any") for i in np.nonzero(rng.random(n) < 0.05)[0]]
    return make_batch(rng, sas, np.zeros(n, dtype=np.int64), cts, tamper, stride_pad=8, len_delta=len_delta,
                      foreign=foreign)


ETA_FAMILIES = ["f-quads", "g-one-long", "h-random"]
ETA_UNITS = 32


def _eta_len(rng, kind, nb):
    """A payload of nb blocks: whole for CBC, the last block of 4, 8, 12 or
    16 bytes for AES-CTR and ESP-NULL."""
    return 16 * nb if kind.startswith("cbc") else 16 * (nb - 1) + 4 * int(rng.integers(1, 5))


@functools.lru_cache(maxsize=None)
def eta_mixed(family, kind):
    """f: every quad of four consecutive records holds four block counts with
       four different nb mod 4, the residues rotating from quad to quad.
    g: one record of 68 blocks (CTR / NULL: 1088 bytes) at lane u mod 64 of
       unit u, so at each of the four quad positions in turn, among 63 of one
       block (CTR / NULL: 4 bytes).
    h: random draws from the kind's set with malformed records (a CBC payload
       shortened by 4, an empty payload, session id 0xFFFF), about 5 % of the
       records tampered anywhere, and a partial last unit."""
    rng = np.random.default_rng(8400 + 16 * ETA_FAMILIES.index(family) + list(ETA_KINDS).index(kind))
    sas = [eta_sa(rng, kind)]
    cbc = kind.startswith("cbc")
    if family == "f-quads":
        cts = []
        for q in range(ETA_UNITS * ETA_UNIT // 4):
            for k in range(4):
                nb = 4 * int(rng.integers(0, 17)) + (k + q) % 4
                cts.append(_eta_len(rng, kind, nb if nb else 4))
        tamper = [(u * ETA_UNIT + (5 * u) % ETA_UNIT, "icv") for u in range(0, ETA_UNITS, 3)]
        return make_batch(rng, sas, np.zeros(len(cts), dtype=np.int64), cts, tamper, stride_pad=4)
    if family == "g-one-long":
        cts = np.full(ETA_UNITS * ETA_UNIT, 16 if cbc else 4)
        cts[[u * ETA_UNIT + u for u in range(ETA_UNITS)]] = 1088
        tamper = [(u * ETA_UNIT + u, "last") for u in range(0, ETA_UNITS, 5)]
        return make_batch(rng, sas, np.zeros(len(cts), dtype=np.int64), cts, tamper, stride_pad=4)
    n = ETA_UNITS * ETA_UNIT - 27
    cts = rng.choice(eta_lens(kind), n)
    picks = rng.choice(n, 90, replace=False)
    cts[picks[:30]] = 0
    orphan = [int(i) for i in picks[30:60]]
    len_delta = {int(i): -4 for i in picks[60:]} if cbc else {}
    tamper = [(int(i), "any") for i in np.nonzero(rng.random(n) < 0.05)[0]]
    return make_batch(rng, sas, np.zeros(n, dtype=np.int64), cts, tamper, stride_pad=4, len_delta=len_delta,
                      orphan=orphan)


@functools.lru_cache(maxsize=None)
def eta_interleaved():
    """i: four sessions of different cipher and hash interleaved lane by lane
    in every unit (CBC-SHA1, CTR-SHA2-256-ESN, NULL-SHA2-512, CBC-SHA2-384),
    the order rotating from unit to unit: the cipher passes walk the sessions
    one at a time and both quad HMAC passes run with lanes off inside every
    quad.  Random lengths of each kind's set, 5 % tampered."""
    rng = np.random.default_rng(8500)
    sas = [EtaSA(rng, 16, sha=1), EtaSA(rng, 16, ctr=True, sha=256, esn=True), EtaSA(rng, null=True, sha=512),
           EtaSA(rng, 16, sha=384)]
    n = ETA_UNITS * ETA_UNIT
    sa_idx = np.array([(i % ETA_UNIT + i // ETA_UNIT) % 4 for i in range(n)])
    cts = np.where((sa_idx == 0) | (sa_idx == 3), rng.choice(CBC_LENS[1:], n), rng.choice(CTR_LENS[1:], n))
    tamper = [(int(i), "any") for i in np.nonzero(rng.random(n) < 0.05)[0]]
    return make_batch(rng, sas, sa_idx, cts, tamper, stride_pad=4)


# ---------------------------------------------------------------------------
# long layouts (test_long_records_gpu.py): the length sets above.  A uniform
# one is about 40 MiB and drags its two oracle arenas along, so ONE long
# layout is kept at a time, whichever function made it.

_long_slot = {}


def _one_long(key, make):
    if key not in _long_slot:
        _long_slot.clear()
        _long_slot[key] = make()
    return _long_slot[key]


def gcm_long_uniform(si):
    """GCM_LONG_LENS of the session's ICV length, 16 consecutive records each;
    tampered as gcm_uniform."""
    def make():
        rng = np.random.default_rng(8700 + si)
        lens = GCM_LONG_LENS(GCM_SESSIONS[si][2])
        cts = np.repeat(lens, GCM_RUN)
        tamper = []
        for r in range(1, len(lens), 2):
            a = (r // 2) % GCM_RUN
            b = (a + 1 + (r // 32) % (GCM_RUN - 1)) % GCM_RUN
            tamper += [(r * GCM_RUN + a, "last"), (r * GCM_RUN + b, "icv")]
        return make_batch(rng, [_gcm_sa(rng, si)], np.zeros(len(cts), dtype=np.int64), cts, tamper)
    return _one_long(("gcm_long_uniform", si), make)


def gcm_long_aligned(si):
    """GCM_LONG_ALIGNED, 16 consecutive records each (every wave takes the
    aligned schedule at 4 lanes); one ICV tampered in every second run."""
    def make():
        rng = np.random.default_rng(8750 + si)
        cts = np.repeat(GCM_LONG_ALIGNED(), GCM_RUN)
        tamper = [(r * GCM_RUN + (5 * r) % GCM_RUN, "icv") for r in range(1, len(cts) // GCM_RUN, 2)]
        return make_batch(rng, [_gcm_sa(rng, si)], np.zeros(len(cts), dtype=np.int64), cts, tamper)
    return _one_long(("gcm_long_aligned", si), make)


def eta_long_uniform(kind):
    """The kind's long set, 64 consecutive records each; even units intact
    (the equal-length path of the verified decrypt at nbu up to 4093), three
    records tampered in every odd one, as eta_uniform."""
    def make():
        rng = np.random.default_rng(8800 + list(ETA_KINDS).index(kind))
        lens = eta_long_lens(kind)
        cts = np.repeat(lens, ETA_UNIT)
        tamper = []
        for u in range(1, len(lens), 2):
            a = (5 * u) % ETA_UNIT
            tamper += [(u * ETA_UNIT + (a + 21 * k) % ETA_UNIT, w) for k, w in enumerate(("first", "last", "icv"))]
        return make_batch(rng, [eta_sa(rng, kind)], np.zeros(len(cts), dtype=np.int64), cts, tamper)
    return _one_long(("eta_long_uniform", kind), make)


def _log_uniform(rng, lo, hi, step, size):
    """Multiples of step in [lo, hi], their logarithm uniform."""
    x = np.exp(rng.uniform(np.log(lo), np.log(hi + step), size))
    return np.clip(x.astype(np.int64) // step * step, lo, hi)


GCM_LONG_WAVES = 32
ETA_LONG_UNITS = 8


def gcm_long_mixed(foreign=True):
    """32 waves of 16 records and 5 more, lengths log-uniform over 4..top, so
    every lane of a wave rebuilds its counter cache at steps of its own.  In
    every whole wave one record (its lane rotating) lies above 32 KiB and
    another below 64 bytes.  Two sessions, one per aligned run of 256 records
    (include/espgpu.h), guard bytes between the records, 5 % tampered anywhere,
    some descriptors with len % 4 == 2 and (foreign=True: the grouped form)
    some with the other session's id, neither at a multiple of four
    (gcm_mixed) nor on a wave's two prescribed records."""
    def make():
        rng = np.random.default_rng(8900)
        sas = [_gcm_sa(rng, 0), _gcm_sa(rng, 1)]
        n = GCM_LONG_WAVES * GCM_RUN + 5
        sa_idx = np.arange(n) // 256 % 2
        tops = np.array([gcm_top(sas[s].mlen) for s in sa_idx])
        cts = np.minimum(_log_uniform(rng, 4, tops.max(), 4, n), tops)
        fixed = set()
        for w in range(GCM_LONG_WAVES):
            a, b = w * GCM_RUN + (7 * w) % GCM_RUN, w * GCM_RUN + (7 * w + 5) % GCM_RUN
            cts[a] = _log_uniform(rng, 32772, tops[a], 4, 1)[0]
            cts[b] = 4 * int(rng.integers(1, 16))
            fixed |= {a, b}
        free = np.array([i for i in range(n) if i % 4 and i not in fixed and i != n - 2])
        picks = rng.choice(free, 24, replace=False)
        other = {int(i): 1 - int(sa_idx[i]) for i in picks[:12]}
        len_delta = {int(i): 2 for i in picks[12:]}
        len_delta[n - 2] = 2                              # in the last, partial wave
        tamper = [(int(i), "any") for i in np.nonzero(rng.random(n) < 0.05)[0]]
        return make_batch(rng, sas, sa_idx, cts, tamper, stride_pad=8, len_delta=len_delta,
                          foreign=other if foreign else None)
    return _one_long(("gcm_long_mixed", foreign), make)


def eta_long_mixed(kind):
    """8 units of 64 records less 27, lengths log-uniform up to the kind's
    largest (CBC: whole blocks), one record at the largest in every unit at a
    rotating lane; 5 % tampered anywhere, and a few empty payloads, orphans and
    CBC payloads shortened by 4 as eta_mixed("h-random")."""
    def make():
        rng = np.random.default_rng(9000 + list(ETA_KINDS).index(kind))
        sas = [eta_sa(rng, kind)]
        cbc = kind.startswith("cbc")
        step, top = (16, eta_top(kind)) if cbc else (4, eta_top(kind))
        n = ETA_LONG_UNITS * ETA_UNIT - 27
        cts = _log_uniform(rng, step, top, step, n)
        fixed = [u * ETA_UNIT + (9 * u + 3) % (ETA_UNIT - 27) for u in range(ETA_LONG_UNITS)]
        cts[fixed] = top
        free = np.array([i for i in range(n) if i not in fixed])
        picks = rng.choice(free, 24, replace=False)
        cts[picks[:8]] = 0
        orphan = [int(i) for i in picks[8:16]]
        len_delta = {int(i): -4 for i in picks[16:]} if cbc else {}
        tamper = [(int(i), "any") for i in np.nonzero(rng.random(n) < 0.05)[0]]
        return make_batch(rng, sas, np.zeros(n, dtype=np.int64), cts, tamper, stride_pad=4, len_delta=len_delta,
                          orphan=orphan)
    return _one_long(("eta_long_mixed", kind), make)
