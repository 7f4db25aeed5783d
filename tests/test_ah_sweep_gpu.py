"""GPU parity of the AH digest kernels (esp_ah.hip digest_kernel<false> and
<true>) over dense byte-length, ICV-field and key-length sweeps and
prescribed wave compositions (ah_sweep_helpers.py), on the device-resident
batch path (signing, verifying in place and out of place with trailer words)
and the opencrypto driver path (DigestParams::op 2).

Uniform: every byte length from the ICV field alone to four hash blocks and
8 bytes fills a unit of 64 records of its own, the field walking the record.
Mixed: the records of a unit differ as each family prescribes (see the layout
functions).  Every case is decided by oracle.hmac (AhSA.icv_hole / AhSA.icv,
pinned to hashlib in test_ah_sweep.py), over every status, every byte of the
arena and of the prefilled `out`, and every trailer word
(ah_sweep_helpers.check); a failure names the first differing record, its
unit and lane, its length, salt, hash and ESN setting."""
import numpy as np
import pytest

import ah_sweep_helpers as H
import sweep_helpers as S
from ah_helpers import BLOCK
from helpers import EtaSA

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

HASH_ESN = pytest.mark.parametrize("sha,esn", H.HASH_ESN, ids=H.HASH_ESN_IDS)
MODE = pytest.mark.parametrize("mode", H.MODES)


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


def _run(drv, lay, mode, grouped=True):
    """The layout's sessions opened, those of freed_sas freed again (their
    records keep the stale id), the comparison, every session freed."""
    sids = []
    try:
        for s in lay.sas:
            rc, sid = drv.newsession(s.csp())
            assert rc == 0, drv.last_error()
            sids.append(sid)
        for k in lay.freed_sas:
            drv.freesession(sids[k])
        return H.check(drv, lay, sids, mode, grouped=grouped)
    finally:
        for k, s in enumerate(sids):
            if k not in lay.freed_sas:
                drv.freesession(s)


@MODE
@HASH_ESN
def test_uniform_units(drv, sha, esn, mode):
    """Every byte length in [mlen, 4 * blk + 8], 64 consecutive records each
    (a wave of equal lengths), the ICV field at every multiple of 4 the record
    admits (at 64 of them, rotating, where it admits more); even units
    intact, three records tampered in every odd one."""
    _run(drv, H.uniform(sha, esn), mode)


@MODE
@HASH_ESN
def test_quads_of_four_block_counts(drv, sha, esn, mode):
    _run(drv, H.quads(sha, esn), mode)


@MODE
@HASH_ESN
def test_one_long_record_in_a_unit(drv, sha, esn, mode):
    _run(drv, H.one_long(sha, esn), mode)


@MODE
def test_hashes_interleaved_in_a_unit(drv, mode):
    _run(drv, H.hashes(), mode)


@MODE
@pytest.mark.parametrize("grouped", [True, False], ids=["grouped", "planner"])
def test_random_with_malformed_records(drv, grouped, mode):
    _run(drv, H.random_mix(), mode, grouped=grouped)


def test_hashes_interleaved_through_the_planner(drv):
    _run(drv, H.hashes(), "outofplace", grouped=False)


# ---- HMAC key lengths ------------------------------------------------------------

def test_hmac_key_lengths():
    """Keys of 1, hash size, blk - 1, blk, blk + 1 and 2 * blk + 7 bytes for
    every hash (host_crypto.cpp's pad states hash a key longer than the block
    first): 24 AH sessions, and one ESP-NULL + HMAC session per hash with a
    key of blk + 1 bytes.  Each signs and verifies four records."""
    d = _driver(max_sessions=40)
    try:
        lay = H.key_lengths()
        for mode in H.MODES:
            _run(d, lay, mode)
        rng = np.random.default_rng(9700)
        sas = [EtaSA(rng, null=True, sha=sha, esn=(sha in (1, 384)), aklen=BLOCK[sha] + 1) for sha in H.SHAS]
        cts = [4, 60, 128, 1088]
        assert set(cts) <= set(S.CTR_LENS) and all(len(s.akey) == BLOCK[s.sha] + 1 for s in sas)
        b = S.make_batch(rng, sas, np.repeat(np.arange(4), 4), np.tile(cts, 4), tamper=[(2, "icv"), (13, "first")])
        sids = []
        for s in sas:
            rc, sid = d.newsession(s.esp_sa().csp())
            assert rc == 0, d.last_error()
            sids.append(sid)
        for mode in ("encrypt", "inplace", "outofplace"):
            st = S.check(d, b, sids, mode)
            assert (st != 0).sum() == (0 if mode == "encrypt" else 2)
    finally:
        d.close()


# ---- the opencrypto driver path --------------------------------------------------

def _cut(pkt, cuts):
    c = [0] + sorted(cuts) + [len(pkt)]
    return [bytearray(pkt[a:b]) for a, b in zip(c, c[1:])]


def _flat(p):
    return bytes(p) if not isinstance(p, list) else b"".join(bytes(b) for b in p)


def _digest_req(fw, ses, buf, start, length, doff, op, esn_hi):
    from espgpu import _lib as L
    crp = fw.crypto_getreq(ses)
    crp.crp_op = op
    crp.crp_flags = L.CRYPTO_F_CBIFSYNC
    crp.crp_buf = buf
    crp.crp_payload_start, crp.crp_payload_length, crp.crp_digest_start = start, length, start + doff
    crp.crp_esn = int(esn_hi).to_bytes(4, "big")
    return crp


def test_driver_every_length():
    """COMPUTE_DIGEST over every byte length in [mlen, 2 * blk + 8] for
    SHA-1 with ESN, SHA2-256, SHA2-384 with ESN and SHA2-512 (720 requests):
    the range at byte alignments 0..3 of its buffer, the digest offset
    rotating over the multiples of 4, every third request a chain cut at
    three points.  The digest of the range as it stands (no hole) is written
    into the field and not one other byte of the buffer changes.  One
    VERIFY_DIGEST per length over the signed buffer: the field is itself
    hashed, so it cannot match (EBADMSG), and nothing is written.  (No
    length is thinned out: the 1440 requests take well under a second.)"""
    from espgpu import _lib as L
    from espgpu.opencrypto import CryptoFramework
    d = _driver(max_sessions=8)
    try:
        fw = CryptoFramework(d)
        rng = np.random.default_rng(9800)
        crps, checks, aligns = [], [], set()
        for sha, esn in ((1, True), (256, False), (384, True), (512, False)):
            sa = H.make_sa(rng, sha, esn)
            err, ses = fw.crypto_newsession(sa.csp())
            assert err == 0
            for k, n in enumerate(range(sa.mlen, 2 * BLOCK[sha] + 9)):
                lead = 4 * (k % 3) + (k // 4) % 4             # bytes before the range: every alignment
                pkt = rng.integers(0, 256, lead + n + 5, dtype=np.uint8).tobytes()
                doff = 4 * ((7 * k) % (((n - sa.mlen) & ~3) // 4 + 1))
                eh = int(rng.integers(0, 2**32))
                want = bytearray(pkt)
                want[lead + doff:lead + doff + sa.mlen] = sa.icv(pkt[lead:lead + n], eh)
                cuts = None
                if k % 3 == 2:
                    cuts = sorted({c for c in (1, lead + doff + 2, lead + n - 2) if 0 < c < len(pkt)})
                    aligns.add(lead % 4)
                what = "HMAC-SHA%d, ESN %s: %d bytes at %d, digest at %d%s" % (
                    sha, esn, n, lead, doff, ", chain cut at %s" % cuts if cuts else "")
                buf = _cut(pkt, cuts) if cuts else bytearray(pkt)
                crps.append(_digest_req(fw, ses, buf, lead, n, doff, L.CRYPTO_OP_COMPUTE_DIGEST, eh))
                checks.append((0, bytes(want), "compute, " + what))
                vbuf = _cut(bytes(want), cuts) if cuts else bytearray(want)
                crps.append(_digest_req(fw, ses, vbuf, lead, n, doff, L.CRYPTO_OP_VERIFY_DIGEST, eh))
                checks.append((H.EBADMSG, bytes(want), "verify, " + what))
        assert len(crps) == 2 * 720 and aligns == {0, 1, 2, 3}       # (the chains too at every alignment)
        # in a seeded random order: hashes and lengths mix in the waves, and in the staging a short
        # range follows a longer one
        for i in rng.permutation(len(crps)):
            assert fw.crypto_dispatch(crps[i]) == 0
        fw.crypto_drain()
        for c, (etype, want, what) in zip(crps, checks):
            assert c.crp_etype == etype, (what, c.crp_etype, etype)
            got = _flat(c.crp_buf)
            assert got == want, "%s: byte %d differs" % (what, next(i for i in range(len(want)) if got[i] != want[i]))
    finally:
        d.close()
