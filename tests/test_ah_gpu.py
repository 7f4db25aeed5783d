"""GPU tests of AH digest sessions (CSP_MODE_DIGEST, esp_ah.hip digest_kernel)
against oracle.hmac: the device-resident batch path (one record = one
packet, desc.salt = the ICV field's offset, the field read as zeros) and the
opencrypto driver path (swcr_authcompute to the letter)."""
import numpy as np
import pytest

import oracle as O
from ah_helpers import BLOCK, DESC, SKIP, AhSA, golden_ah, golden_sa
from helpers import EtaSA, GcmSA, build_records, oracle_decrypt

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

EINVAL, EBADMSG, ENOTSUP = 22, 74, 95
TR_VALID = 0x80000000
SHAS = (1, 256, 384, 512)


def _driver(**kw):
    from espgpu.opencrypto import GpuCryptoDriver
    if not torch.cuda.is_available():
        pytest.fail("GPU test run without a visible HIP device")
    return GpuCryptoDriver(**kw)


@pytest.fixture(scope="module", autouse=True)
def ah_offered():
    """The driver path's sessions go through the probe: the bid for AH sessions on
    (set_tuning "ah_offer", process-wide), and back to the default afterwards.  The
    batch tests open their SAs with espgpu_newsession, which serves them either way."""
    from espgpu import _lib as L
    assert L.lib().espgpu_set_tuning(None, b"ah_offer", 1) == 0
    yield
    L.lib().espgpu_set_tuning(None, b"ah_offer", -1)


@pytest.fixture(scope="module")
def drv():
    d = _driver(max_sessions=64)
    yield d
    d.close()


@pytest.fixture(scope="module")
def ahsas(drv):
    """One SA per hash and ESN setting, shared by the batch tests: {(sha, esn): AhSA with .sid}"""
    rng = np.random.default_rng(7000)
    out = {}
    for sha in SHAS:
        for esn in (False, True):
            s = AhSA(rng, sha, esn=esn, aklen=150 if (sha == 256 and esn) else None)   # one key past the block
            rc, s.sid = drv.newsession(s.csp())
            assert rc == 0, drv.last_error()
            out[(sha, esn)] = s
    return out


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _descs_dev(d):
    return torch.from_numpy(np.ascontiguousarray(d).view(np.uint8).copy()).cuda()


class Batch:
    """Records of random bytes (the ICV field too: garbage) at 4-byte aligned
    offsets with random guard bytes between them.  recs: (AhSA, len, salt)."""

    def __init__(self, rng, recs, esn_hi=None):
        self.recs = recs
        n = len(recs)
        self.n = n
        self.descs = np.zeros(n, dtype=DESC)
        pos = 16
        for i, (sa, L, salt) in enumerate(recs):
            self.descs[i] = (pos // 4, L, sa.sid, 0, salt)
            pos += ((L + 3) & ~3) + 4 * int(rng.integers(1, 5))
        self.descs["esn_hi"] = rng.integers(0, 2**32, n, dtype=np.uint32) if esn_hi is None else esn_hi
        self.arena = rng.integers(0, 256, pos + 64, dtype=np.uint8)

    def span(self, i):
        return int(self.descs["off4"][i]) * 4, int(self.descs["len"][i])

    def signed(self):
        """The arena after encrypt_batch, by oracle.hmac: every record's ICV
        field holds its ICV (hashed with the field as zeros), nothing else moved."""
        a = self.arena.copy()
        for i, (sa, L, salt) in enumerate(self.recs):
            o, _ = self.span(i)
            icv = sa.icv_hole(a[o:o + L].tobytes(), salt, int(self.descs["esn_hi"][i]))
            a[o + salt:o + salt + sa.mlen] = np.frombuffer(icv, dtype=np.uint8)
        return a


def _encrypt(drv, arena, descs, grouped=True):
    from espgpu.batch import encrypt_batch
    n = len(descs)
    a = _dev(arena)
    st = torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda")
    encrypt_batch(drv, a, _descs_dev(descs), n, st, grouped=grouped)
    torch.cuda.synchronize()
    return a.cpu().numpy(), st.cpu().numpy()


def _decrypt(drv, arena, descs, grouped=True, inplace=True, trailer=False):
    """-> status, arena after, d_out after (prefilled 0xCC; None in place), trailer words"""
    from espgpu.batch import decrypt_batch
    n = len(descs)
    a = _dev(arena)
    out = None if inplace else torch.full_like(a, 0xCC)
    st = torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda")
    tr = torch.full((n,), 0x5a5a5a5a, dtype=torch.int32, device="cuda") if trailer else None
    decrypt_batch(drv, a, _descs_dev(descs), n, st, out=out, grouped=grouped, trailer=tr)
    torch.cuda.synchronize()
    return (st.cpu().numpy(), a.cpu().numpy(), None if inplace else out.cpu().numpy(),
            tr.cpu().numpy().view(np.uint32) if trailer else None)


def _check_both_ways(drv, b, grouped=True):
    """encrypt_batch writes exactly the ICVs; decrypt_batch accepts them in
    place, out of place and with trailer words, writing nothing."""
    want = b.signed()
    got, st = _encrypt(drv, b.arena, b.descs, grouped)
    assert (st == 0).all(), np.nonzero(st)[0][:10]
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, bad[:10]
    for inplace, trailer in ((True, False), (False, True)):
        st, a, out, tr = _decrypt(drv, want, b.descs, grouped, inplace, trailer)
        assert (st == 0).all(), (inplace, np.nonzero(st)[0][:10])
        assert (a == want).all()
        assert out is None or (out == 0xCC).all()
        assert tr is None or (tr == TR_VALID).all()
    return want


def _tail_lengths(sha, esn):
    """L0 over one to three hash blocks at every residue where the padding
    changes shape: the ESN word moves the boundary down by 4."""
    blk = BLOCK[sha]
    res = [0, 1, 2, 3, 51, 52, 54, 55, 56, 57, 63] if blk == 64 else [0, 1, 107, 108, 110, 111, 112, 113, 127]
    return sorted(set(blk * k + r for r in res for k in range(4) if 48 <= blk * k + r <= 3 * blk + 3))


@pytest.mark.parametrize("sha", SHAS)
@pytest.mark.parametrize("esn", [False, True])
def test_lengths(drv, ahsas, sha, esn):
    sa = ahsas[(sha, esn)]
    rng = np.random.default_rng(7100 + sha + esn)
    at = SKIP + 12
    lens = _tail_lengths(sha, esn) + [44, 1500, 9000, 65535]    # 44: the smallest AH packet (IPv4, HMAC-SHA1-96)
    recs = [(sa, L, min(at, (L - sa.mlen) & ~3)) for L in lens]
    _check_both_ways(drv, Batch(rng, recs))


@pytest.mark.parametrize("sha", SHAS)
def test_icv_field_positions(drv, ahsas, sha):
    rng = np.random.default_rng(7200 + sha)
    blk = BLOCK[sha]
    recs = []
    for esn in (False, True):
        sa = ahsas[(sha, esn)]
        m = sa.mlen
        for L in (200, 3 * blk + 29, 1500):
            # IPv4, IPv6, IPv4 with 40 B of options; straddling a block boundary; in the last
            # block beside the padding; ending exactly at len (L a multiple of 4 or not)
            for salt in (32, 52, 72, blk - 8, 2 * blk - 4, (L - m - 8) & ~3, (L - m) & ~3):
                if salt + m <= L:                           # (a field past the record is EINVAL: see below)
                    recs.append((sa, L, salt))
        recs.append((sa, 64 + m, 64))                       # the field is the record's last dwords exactly
        recs.append((sa, m, 0))                             # the record is the field
    _check_both_ways(drv, Batch(rng, recs))


def test_straddle_mlen_12_and_32(drv):
    """salt = 56 with a 12-byte and a 32-byte field (64-byte blocks), 120 for the wide hashes."""
    rng = np.random.default_rng(7250)
    d = _driver(max_sessions=8)
    try:
        recs = []
        for sha, mlen, salt in ((1, 12, 56), (256, 32, 56), (256, 12, 56), (384, 12, 120), (512, 32, 120),
                                (512, 64, 120), (1, 20, 56), (384, 0, 120)):
            sa = AhSA(rng, sha, esn=bool(mlen & 4), mlen=mlen or None)
            if mlen == 0:                                    # csp_auth_mlen 0: the whole hash
                sa.sa.mlen, sa.mlen = 0, 48
            rc, sa.sid = d.newsession(sa.csp())
            assert rc == 0, d.last_error()
            recs += [(sa, L, salt) for L in (salt + sa.mlen, 191, 300)]
        _check_both_ways(d, Batch(rng, recs))
    finally:
        d.close()


@pytest.mark.parametrize("n", [1, 3, 63, 64, 65, 130])
def test_batch_sizes(drv, ahsas, n):
    rng = np.random.default_rng(7300 + n)
    sas = list(ahsas.values())
    blocks = (1, 2, 5, 24)                                  # a quad's four records differ in length
    recs = []
    for i in range(n):
        sa = sas[(i // 4) % len(sas)] if n > 3 else sas[i]
        L = BLOCK[sa.sha] * blocks[i % 4] - 9 - int(rng.integers(0, 40))
        recs.append((sa, max(L, 32 + sa.mlen), 32))
    for grouped in (True, False):
        _check_both_ways(drv, Batch(rng, recs), grouped)


def test_quads_with_dead_records(drv, ahsas):
    """A freed session's record, a len 0 record and bad salts between live ones: EINVAL for
    those, and the live neighbours in their quads are unaffected."""
    rng = np.random.default_rng(7400)
    dead = AhSA(rng, 256)
    rc, dead.sid = drv.newsession(dead.csp())
    assert rc == 0
    drv.freesession(dead.sid)
    recs, kind = [], []
    for sha in SHAS:
        sa = ahsas[(sha, False)]
        for L, salt, k in ((300, 32, "ok"), (0, 0, "inv"), (555, 32, "ok"), (300, 32, "dead"), (200, 34, "inv"),
                           (129, 32, "ok"), (100, 100 - sa.mlen + 4, "inv"), (100, 0x10020, "inv"), (77, 32, "ok")):
            recs.append((dead if k == "dead" else sa, L, salt))
            kind.append(k)
    b = Batch(rng, recs)
    ok = np.array([k == "ok" for k in kind])
    want = b.arena.copy()
    for i in np.nonzero(ok)[0]:
        sa, L, salt = recs[i]
        o, _ = b.span(i)
        want[o + salt:o + salt + sa.mlen] = np.frombuffer(
            sa.icv_hole(b.arena[o:o + L].tobytes(), salt, int(b.descs["esn_hi"][i])), dtype=np.uint8)
    for grouped in (True, False):
        got, st = _encrypt(drv, b.arena, b.descs, grouped)
        assert (st[ok] == 0).all() and (st[~ok] == EINVAL).all(), (grouped, st)
        assert (got == want).all()
        st, a, out, tr = _decrypt(drv, want, b.descs, grouped, inplace=False, trailer=True)
        assert (st[ok] == 0).all() and (st[~ok] == EINVAL).all(), (grouped, st)
        assert (a == want).all() and (out == 0xCC).all()
        assert (tr[ok] == TR_VALID).all() and (tr[~ok] == 0).all()


@pytest.mark.parametrize("sha", SHAS)
def test_verify_rejects_any_flipped_bit(drv, ahsas, sha):
    rng = np.random.default_rng(7500 + sha)
    sa = ahsas[(sha, True)]
    m, blk = sa.mlen, BLOCK[sha]
    L, salt = 2 * blk + 35, 32
    flips = [None, 0, L - 1, blk - 1, blk, 2 * blk, salt - 1, salt + m] + list(range(salt, salt + m))
    b = Batch(rng, [(sa, L, salt)] * len(flips))
    good = b.signed()
    bad = good.copy()
    for i, f in enumerate(flips):
        if f is not None:
            bad[b.span(i)[0] + f] ^= 1 << int(rng.integers(0, 8))
    want_st = np.array([0 if f is None else EBADMSG for f in flips])
    for inplace in (True, False):
        st, a, out, tr = _decrypt(drv, bad, b.descs, True, inplace, trailer=True)
        assert (st == want_st).all(), (inplace, st)
        assert (a == bad).all() and (out is None or (out == 0xCC).all())
        assert (tr == np.where(want_st == 0, TR_VALID, 0)).all()
    # the ESN high word is part of the message
    d = b.descs.copy()
    d["esn_hi"] ^= 1
    st, _, _, _ = _decrypt(drv, good, d)
    assert (st == EBADMSG).all()


def test_hole_ignores_what_the_field_held(drv, ahsas):
    rng = np.random.default_rng(7600)
    recs = [(ahsas[(sha, False)], L, 32) for sha in SHAS for L in (100, 64 * 3, 777)]
    b = Batch(rng, recs)
    zeroed = b.arena.copy()
    for i, (sa, L, salt) in enumerate(recs):
        o, _ = b.span(i)
        zeroed[o + salt:o + salt + sa.mlen] = 0
    g1, st1 = _encrypt(drv, b.arena, b.descs)
    g2, st2 = _encrypt(drv, zeroed, b.descs)
    assert (st1 == 0).all() and (st2 == 0).all()
    assert (g1 == g2).all() and (g1 == b.signed()).all()


def _mixed(drv, rng, grouped):
    """GCM, CBC+SHA1, CTR+SHA-512, ESP-NULL records (helpers.build_records, the
    oracle's ESP) and AH records of all four hashes in one batch."""
    esas = [GcmSA(rng, 16), EtaSA(rng, 32), EtaSA(rng, 16, ctr=True, sha=512), EtaSA(rng, null=True, sha=256)]
    asas = [AhSA(rng, sha, esn=(sha in (1, 512))) for sha in SHAS]
    esid = []
    for s in esas:
        rc, sid = drv.newsession(s.esp_sa().csp())
        assert rc == 0, drv.last_error()
        esid.append(sid)
    for s in asas:
        rc, s.sid = drv.newsession(s.csp())
        assert rc == 0, drv.last_error()
    run = 256 if grouped else 75
    ne = run * len(esas)
    eidx = np.repeat(np.arange(len(esas)), run)
    cts = np.where(eidx == 1, rng.choice([16, 48, 208], ne), rng.choice([4, 12, 100, 260], ne))
    plain, ct, edescs, eh = build_records(rng, esas, eidx, cts, esn_hi=np.zeros(ne, dtype=np.uint32))
    ab = Batch(rng, [(asas[i // run], int(rng.choice([64, 67, 77, 120, 129, 300])), 32)   # (>= 32 + the longest ICV)
                     for i in range(run * len(asas))])
    # one arena: the ESP records, then the AH records
    base = (len(ct) + 15) & ~15
    ad = ab.descs.copy()
    ad["off4"] += base // 4
    ed = edescs.copy()
    ed["sa"] = [esid[s] for s in eidx]
    descs = np.concatenate([ed, ad])
    kind = np.concatenate([np.zeros(ne, dtype=bool), np.ones(ab.n, dtype=bool)])      # True: AH
    if not grouped:
        perm = rng.permutation(len(descs))
        descs, kind = descs[perm], kind[perm]

    def arena(esp_part, ah_part):
        a = np.zeros(base + len(ah_part), dtype=np.uint8)
        a[:len(esp_part)] = esp_part
        a[base:] = ah_part
        return a

    signed = ab.signed()
    # encrypt: the oracle's ciphertext and ICVs, the AH ICVs, nothing else
    got, st = _encrypt(drv, arena(plain, ab.arena), descs, grouped)
    assert (st == 0).all(), np.nonzero(st)[0][:10]
    assert (got == arena(ct, signed)).all()
    # decrypt out of place, some ESP and AH records tampered
    bad_e, bad_a = ct.copy(), signed.copy()
    te = rng.random(ne) < 0.1
    for i in np.nonzero(te)[0]:
        bad_e[int(edescs["off4"][i]) * 4 + int(edescs["len"][i]) - 2] ^= 4
    ta = rng.random(ab.n) < 0.1
    for i in np.nonzero(ta)[0]:
        o, L = ab.span(i)
        bad_a[o + int(rng.integers(0, L))] ^= 0x20
    ref_out, ref_st = oracle_decrypt(esas, bad_e, edescs, eh)
    want_st = np.concatenate([ref_st, np.where(ta, EBADMSG, 0)])
    if not grouped:
        want_st = want_st[perm]
    src = arena(bad_e, bad_a)
    st, a, out, _ = _decrypt(drv, src, descs, grouped, inplace=False)
    assert (st == want_st).all(), np.nonzero(st != want_st)[0][:10]
    assert (a == src).all()
    assert (out[base:] == 0xCC).all()                       # AH: nothing written to d_out
    for i in np.nonzero(ref_st == 0)[0]:
        s = esas[eidx[i]]
        o, L = int(edescs["off4"][i]) * 4, int(edescs["len"][i])
        assert (out[o + s.hlen:o + L - s.mlen] == ref_out[o + s.hlen:o + L - s.mlen]).all(), i
    for sid in esid + [s.sid for s in asas]:
        drv.freesession(sid)


@pytest.mark.parametrize("grouped", [False, True])
def test_mixed_esp_and_ah_batch(grouped):
    d = _driver(max_sessions=16)
    try:
        _mixed(d, np.random.default_rng(7700 + grouped), grouped)
    finally:
        d.close()


def test_packed_and_host_paths_answer_enotsup(drv, ahsas):
    a = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    dd = np.zeros(1, dtype=DESC)
    dd[0] = (0, 128, ahsas[(1, False)].sid, 0, 32)
    st = torch.zeros(1, dtype=torch.uint8, device="cuda")
    out = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    rc = drv.lib.espgpu_decrypt_batch_packed(drv.ctx, a.data_ptr(), _descs_dev(dd).data_ptr(), 1, st.data_ptr(),
                                             out.data_ptr(), 128, 0, None)
    assert rc == ENOTSUP
    ha, ho = torch.zeros(4096, dtype=torch.uint8).pin_memory(), torch.zeros(4096, dtype=torch.uint8).pin_memory()
    hd = torch.from_numpy(dd.view(np.uint8).copy()).pin_memory()
    hs = torch.zeros(1, dtype=torch.uint8).pin_memory()
    rc = drv.lib.espgpu_decrypt_host(drv.ctx, ha.data_ptr(), 4096, hd.data_ptr(), 1, hs.data_ptr(), ho.data_ptr(),
                                     0, 0)
    assert rc == ENOTSUP


def test_context_without_digest_sessions_is_unchanged():
    """n_dig follows new and freed sessions: packed output works again once the last is freed."""
    d = _driver(max_sessions=8)
    try:
        rng = np.random.default_rng(7800)
        g = GcmSA(rng, 16)
        rc, gs = d.newsession(g.esp_sa().csp())
        assert rc == 0
        plain, ct, descs, eh = build_records(rng, [g], np.zeros(4, dtype=np.int64), np.full(4, 100))
        descs["sa"] = gs
        a = _dev(ct)
        out = torch.zeros(4 * 256, dtype=torch.uint8, device="cuda")
        st = torch.full((4,), 0xEE, dtype=torch.uint8, device="cuda")

        def packed():
            return d.lib.espgpu_decrypt_batch_packed(d.ctx, a.data_ptr(), _descs_dev(descs).data_ptr(), 4,
                                                     st.data_ptr(), out.data_ptr(), 256, 0, None)
        assert packed() == 0
        s1, s2 = AhSA(rng, 1), AhSA(rng, 512)
        for s in (s1, s2):
            rc, s.sid = d.newsession(s.csp())
            assert rc == 0
        assert packed() == ENOTSUP
        d.freesession(s1.sid)
        assert packed() == ENOTSUP
        d.freesession(s2.sid)
        assert packed() == 0
        torch.cuda.synchronize()
        assert (st.cpu().numpy() == 0).all()
    finally:
        d.close()


# ---- the opencrypto driver path ------------------------------------------------

def _cut(pkt, cuts):
    c = [0] + sorted(cuts) + [len(pkt)]
    return [bytearray(pkt[a:b]) for a, b in zip(c, c[1:])]


def _flat(p):
    return bytes(p) if not isinstance(p, list) else b"".join(bytes(b) for b in p)


def _digest_req(fw, ses, sa, buf, start, length, doff, op, esn_hi=0):
    from espgpu import _lib as L
    crp = fw.crypto_getreq(ses)
    crp.crp_op = op
    crp.crp_flags = L.CRYPTO_F_CBIFSYNC
    crp.crp_buf = buf
    crp.crp_payload_start, crp.crp_payload_length, crp.crp_digest_start = start, length, start + doff
    crp.crp_esn = int(esn_hi).to_bytes(4, "big")
    return crp


def test_driver_compute_and_verify():
    """COMPUTE writes the mlen digest bytes of the range as it stands (swcr_authcompute) and
    nothing else, contiguous and as chains cut anywhere; VERIFY writes nothing; malformed
    requests complete with EINVAL."""
    from espgpu import _lib as L
    from espgpu.opencrypto import CryptoFramework
    d = _driver(max_sessions=16)
    try:
        fw = CryptoFramework(d)
        rng = np.random.default_rng(7900)
        crps, checks = [], []
        for sha in SHAS:
            for esn in (False, True):
                sa = AhSA(rng, sha, esn=esn)
                err, ses = fw.crypto_newsession(sa.csp())
                assert err == 0
                for k, n in enumerate((sa.mlen, 44, 63, 64, 65, 121, 128, 1499, 9001, 65535)):
                    lead = (0, 3, 14)[k % 3]                   # bytes before the range: any alignment
                    pkt = rng.integers(0, 256, lead + n + 5, dtype=np.uint8).tobytes()
                    doff = min(32, (n - sa.mlen) & ~3)
                    eh = int(rng.integers(0, 2**32))
                    want = bytearray(pkt)
                    want[lead + doff:lead + doff + sa.mlen] = sa.icv(pkt[lead:lead + n], eh)
                    cuts = None if k % 2 == 0 else sorted(set(
                        [1, lead + doff + 2, lead + n - 2] + list(range(3000, len(pkt), 3000))))
                    cuts = cuts and [c for c in cuts if 0 < c < len(pkt)]
                    buf = bytearray(pkt) if not cuts else _cut(pkt, cuts)
                    crps.append(_digest_req(fw, ses, sa, buf, lead, n, doff, L.CRYPTO_OP_COMPUTE_DIGEST, eh))
                    checks.append((0, bytes(want)))
                    # VERIFY over the signed range: the digest field is itself hashed, so it cannot match
                    vbuf = bytearray(want) if not cuts else _cut(bytes(want), cuts)
                    crps.append(_digest_req(fw, ses, sa, vbuf, lead, n, doff, L.CRYPTO_OP_VERIFY_DIGEST, eh))
                    checks.append((EBADMSG, bytes(want)))
                # malformed: digest field not at a multiple of 4, outside the range, AAD, ENCRYPT bit, empty
                pkt = bytes(200)
                for kw in (dict(doff=30), dict(doff=200 - sa.mlen + 4), dict(doff=-4), dict(aad=1), dict(op=1),
                           dict(length=0)):
                    c = _digest_req(fw, ses, sa, bytearray(pkt), 0, kw.get("length", 200), kw.get("doff", 32),
                                    kw.get("op", 0))
                    c.crp_aad_length = 8 if kw.get("aad") else 0
                    crps.append(c)
                    checks.append((EINVAL, pkt))
        for c in crps:
            assert fw.crypto_dispatch(c) == 0
        fw.crypto_drain()
        for i, (c, (etype, want)) in enumerate(zip(crps, checks)):
            assert c.crp_etype == etype, (i, c.crp_etype, etype)
            assert _flat(c.crp_buf) == want, i
    finally:
        d.close()


@pytest.mark.parametrize("xfer", [1, 0])
def test_driver_registered_memory_any_alignment(xfer):
    """Ranges in registered memory at byte alignments 0..3 (zero-copy: the GPU reads them in
    place and writes the digest bytes back), with guard bytes around each one."""
    from espgpu import _lib as L
    from espgpu.opencrypto import CryptoFramework
    d = _driver(max_sessions=8)
    try:
        assert d.set_tuning("xfer", xfer) == 0
        fw = CryptoFramework(d)
        rng = np.random.default_rng(8000 + xfer)
        reg = rng.integers(0, 256, 1 << 18, dtype=np.uint8)
        d.register_host(reg)
        before = reg.copy()
        want = reg.copy()
        crps, pos, nrec = [], 64, 0
        for sha in SHAS:
            sa = AhSA(rng, sha, esn=(sha == 256))
            err, ses = fw.crypto_newsession(sa.csp())
            assert err == 0
            for k, n in enumerate((44 if sha < 384 else 64, 61, 130, 255, 1500, 1501, 1502, 1503)):
                n = max(n, 32 + sa.mlen)
                start = ((pos + 3) & ~3) + (k % 4)             # every byte alignment
                eh = int(rng.integers(0, 2**32))
                want[start + 32:start + 32 + sa.mlen] = np.frombuffer(
                    sa.icv(before[start:start + n].tobytes(), eh), dtype=np.uint8)
                # the buffer is the packet's whole mbuf: guard bytes on both sides belong to it
                crps.append(_digest_req(fw, ses, sa, reg[start - 16:start + n + 16], 16, n, 32,
                                        L.CRYPTO_OP_COMPUTE_DIGEST, eh))
                pos = start + n + 48
                nrec += 1
        z0 = d.stats()["zerocopy"]
        for c in crps:
            assert fw.crypto_dispatch(c) == 0
        fw.crypto_drain()
        assert d.stats()["zerocopy"] - z0 == nrec
        assert all(c.crp_etype == 0 for c in crps)
        diff = np.nonzero(reg != want)[0]
        assert diff.size == 0, diff[:10]                     # the digests, and not one byte more
        d.unregister_host(reg)
    finally:
        d.close()


def test_driver_burst_mixing_ah_and_esp_with_overflow():
    """AH and ESP requests interleaved through 8 small staging slots with the host overflow on."""
    from espgpu import _lib as L
    from espgpu.esp import esp_input_crp, esp_output_crp
    from espgpu.opencrypto import CryptoFramework
    d = _driver(max_sessions=16, batch_records=16, batch_bytes=1 << 18, nbatches=8)
    try:
        assert d.set_tuning("overflow_mb", 16) == 0
        fw = CryptoFramework(d)
        rng = np.random.default_rng(8100)
        esas = [GcmSA(rng, 16), EtaSA(rng, 32, sha=256), EtaSA(rng, null=True, sha=1, esn=True)]
        eses = []
        for s in esas:
            err, cs = fw.crypto_newsession(s.esp_sa().csp())
            assert err == 0
            eses.append(cs)
        asas = [AhSA(rng, sha, esn=(sha == 384)) for sha in SHAS]
        ases = []
        for s in asas:
            err, cs = fw.crypto_newsession(s.csp())
            assert err == 0
            ases.append(cs)
        n = 400
        eidx = rng.integers(0, len(esas), n)
        eh = rng.integers(0, 2**32, n, dtype=np.uint32)
        cts = np.where(eidx == 1, rng.choice([16, 48, 208], n), rng.choice([4, 100, 260], n))
        plain, ct, descs, eh = build_records(rng, esas, eidx, cts, esn_hi=eh)
        crps, checks = [], []
        for i in range(n):
            o, Ln = int(descs["off4"][i]) * 4, int(descs["len"][i])
            s = esas[eidx[i]]
            if i % 2:
                pkt = bytearray(bytes(20) + ct[o:o + Ln].tobytes())
                crps.append(esp_input_crp(fw, eses[eidx[i]], s.esp_sa(), pkt, 20, esn_hi=int(eh[i])))
                checks.append((0, 20 + s.hlen, plain[o + s.hlen:o + Ln - s.mlen].tobytes()))
            else:
                pkt = bytearray(bytes(20) + plain[o:o + Ln].tobytes())
                crps.append(esp_output_crp(fw, eses[eidx[i]], s.esp_sa(), pkt, 20, esn_hi=int(eh[i])))
                checks.append((0, 20, ct[o:o + Ln].tobytes()))
            a = asas[i % len(asas)]
            m = int(rng.choice([64, 67, 99, 1500]))                # (>= 32 + the longest ICV)
            pkt = rng.integers(0, 256, m, dtype=np.uint8).tobytes()
            ah = int(rng.integers(0, 2**32))
            crps.append(_digest_req(fw, ases[i % len(asas)], a, bytearray(pkt) if i % 3 else _cut(pkt, [9, 33, m - 1]),
                                    0, m, 32, L.CRYPTO_OP_COMPUTE_DIGEST, ah))
            checks.append((0, 32, a.icv(pkt, ah)))
        e0 = d.stats()
        for c in crps:
            assert fw.crypto_dispatch(c) == 0
        fw.crypto_drain()
        assert d.stats()["overflow"] > e0["overflow"] and d.stats()["erestart"] == e0["erestart"]
        for i, (c, (etype, off, exp)) in enumerate(zip(crps, checks)):
            assert c.crp_etype == etype, (i, c.crp_etype)
            assert _flat(c.crp_buf)[off:off + len(exp)] == exp, i
    finally:
        d.close()


@pytest.mark.parametrize("v", golden_ah(), ids=lambda v: v["name"])
def test_driver_golden_packets(v):
    """DPDK's AH packets through ah_input_crp / ah_input_cb and ah_output_crp on the GPU."""
    from espgpu import ah as A
    from espgpu.opencrypto import CryptoFramework
    d = _driver(max_sessions=4)
    try:
        fw = CryptoFramework(d)
        sa = golden_sa(v)
        err, ses = fw.crypto_newsession(sa.csp())
        assert err == 0
        good = bytes.fromhex(v["output"])
        at = SKIP + 12
        cases = [good]
        for pos in (len(good) - 1, at, at + 15, 12, SKIP + 4):
            b = bytearray(good)
            b[pos] ^= 0x40
            cases.append(bytes(b))
        pkts = [bytearray(c) if i % 2 == 0 else _cut(c, [6, at + 7, len(c) - 1]) for i, c in enumerate(cases)]
        crps = [A.ah_input_crp(fw, ses, sa.sa, p, SKIP) for p in pkts]
        out = bytearray(good)
        out[at:at + 16] = b"\xee" * 16
        ocrp = A.ah_output_crp(fw, ses, sa.sa, out, SKIP)
        for c in crps + [ocrp]:
            assert fw.crypto_dispatch(c) == 0
        fw.crypto_drain()
        assert all(c.crp_etype == 0 for c in crps + [ocrp])
        verdicts = [A.ah_input_cb(c.crp_opaque, p) for c, p in zip(crps, pkts)]
        assert verdicts == [True] + [False] * (len(cases) - 1)
        out[:SKIP] = ocrp.crp_opaque
        assert bytes(out) == good
        assert O.hmac(O.CRYPTO_SHA2_256_HMAC, sa.key, b"x") != b""
    finally:
        d.close()
