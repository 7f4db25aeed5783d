"""CPU tests of the AH (CSP_MODE_DIGEST) boundary: what espgpu_probesession
answers for the sessions ah_init builds (check_csp, crypto.c:792-821, and
swcr_auth_supported), and the caller side in espgpu.ah (ah_init,
ah_massage_headers, ah_input / ah_input_cb, ah_output) against DPDK's AH
known-answer packets.  No compute calls: no GPU here."""
import numpy as np
import pytest

import oracle as O
from ah_helpers import SKIP, AhSA, golden_ah, golden_sa
from espgpu import _lib as L
from espgpu import ah as A
from espgpu.opencrypto import GpuCryptoDriver, crypto_session_params, cryptop

HASHLEN = {L.CRYPTO_SHA1_HMAC: 20, L.CRYPTO_SHA2_256_HMAC: 32, L.CRYPTO_SHA2_384_HMAC: 48,
           L.CRYPTO_SHA2_512_HMAC: 64}
CRYPTO_NULL_HMAC, CRYPTO_RIPEMD160_HMAC, CRYPTO_SHA2_256, CRYPTO_AES_NIST_GMAC = 9, 8, 35, 26   # cryptodev.h
CSP_F_SEPARATE_OUTPUT = 0x1


def _probe(**kw):
    return GpuCryptoDriver.probesession(crypto_session_params(**kw))


def _offer(v):
    assert L.lib().espgpu_set_tuning(None, b"ah_offer", v) == 0


@pytest.fixture(autouse=True)
def ah_offered():
    """The driver's bid for AH sessions switched on (set_tuning "ah_offer",
    process-wide, no context needed), and back to the default afterwards."""
    _offer(1)
    yield
    _offer(-1)


def test_probe_bids_for_ah_only_when_offered(monkeypatch):
    """Off by default, so that a deployment that sets nothing keeps AH on
    cryptosoft whatever binding it was linked with; FF_GPUCRYPTO_AH=1 or
    set_tuning "ah_offer" 1 switches the bid on."""
    sha256 = L.CRYPTO_SHA2_256_HMAC
    monkeypatch.delenv("FF_GPUCRYPTO_AH", raising=False)
    _offer(-1)
    assert _ah(sha256, 16) == L.EINVAL
    monkeypatch.setenv("FF_GPUCRYPTO_AH", "0")
    assert _ah(sha256, 16) == L.EINVAL
    monkeypatch.setenv("FF_GPUCRYPTO_AH", "1")
    assert _ah(sha256, 16) == L.CRYPTODEV_PROBE_HARDWARE
    assert _ah(sha256, 10) == L.EINVAL
    _offer(0)                                                  # the switch beats the environment
    assert _ah(sha256, 16) == L.EINVAL
    _offer(1)
    monkeypatch.delenv("FF_GPUCRYPTO_AH")
    assert _ah(sha256, 16) == L.CRYPTODEV_PROBE_HARDWARE
    assert L.lib().espgpu_set_tuning(None, b"ah_offer", 2) == L.EINVAL
    # the ESP modes do not depend on it
    _offer(0)
    assert _probe(csp_mode=L.CSP_MODE_AEAD, csp_ivlen=12, csp_cipher_alg=L.CRYPTO_AES_NIST_GCM_16,
                  csp_cipher_klen=16, csp_cipher_key=b"k" * 16) == L.CRYPTODEV_PROBE_HARDWARE


def _ah(aalg, mlen, flags=0, klen=None, **kw):
    klen = HASHLEN[aalg] if klen is None else klen
    args = dict(csp_mode=L.CSP_MODE_DIGEST, csp_flags=flags, csp_auth_alg=aalg, csp_auth_klen=klen,
                csp_auth_key=b"k" * klen if klen else None, csp_auth_mlen=mlen)
    args.update(kw)
    return _probe(**args)


def test_constants():
    assert L.CSP_MODE_DIGEST == 3 and L.CRYPTO_OP_COMPUTE_DIGEST == 0
    src = open(L.HEADER).read()
    assert "#define ESPGPU_CSP_MODE_DIGEST      3" in src
    assert "#define ESPGPU_CRYPTO_OP_COMPUTE_DIGEST 0x0" in src
    assert L.lib().espgpu_abi_version() == 6


@pytest.mark.parametrize("aalg", sorted(HASHLEN))
@pytest.mark.parametrize("esn", [False, True])
def test_probe_accepts_ah_hmacs(aalg, esn):
    flags = L.CSP_F_ESN if esn else 0
    for mlen in (0, 12, 16, 24, 32, HASHLEN[aalg]):
        if mlen <= HASHLEN[aalg]:
            assert _ah(aalg, mlen, flags) == L.CRYPTODEV_PROBE_HARDWARE, (aalg, mlen)
    # keys longer than the hash block (hashed down by hmac_init_pad)
    assert _ah(aalg, 12, flags, klen=200) == L.CRYPTODEV_PROBE_HARDWARE


def test_probe_accepts_what_ah_init_builds():
    rng = np.random.default_rng(3)
    for sha in (1, 256, 384, 512):
        for esn in (False, True):
            assert GpuCryptoDriver.probesession(AhSA(rng, sha, esn=esn).csp()) == L.CRYPTODEV_PROBE_HARDWARE


def test_probe_rejects():
    sha256 = L.CRYPTO_SHA2_256_HMAC
    assert _ah(sha256, 16) == L.CRYPTODEV_PROBE_HARDWARE            # (the accepted shape, for contrast)
    for alg in (CRYPTO_NULL_HMAC, CRYPTO_RIPEMD160_HMAC, CRYPTO_SHA2_256):
        assert _probe(csp_mode=L.CSP_MODE_DIGEST, csp_auth_alg=alg, csp_auth_klen=20, csp_auth_key=b"k" * 20,
                      csp_auth_mlen=12) == L.EINVAL
    for ivlen in (0, 12):                                              # AH-GMAC: left to cryptosoft
        assert _probe(csp_mode=L.CSP_MODE_DIGEST, csp_auth_alg=CRYPTO_AES_NIST_GMAC, csp_auth_klen=16,
                      csp_auth_key=b"k" * 16, csp_auth_mlen=16, csp_ivlen=ivlen) == L.EINVAL
    assert _ah(sha256, 16, csp_cipher_alg=L.CRYPTO_AES_CBC, csp_cipher_klen=16, csp_cipher_key=b"k" * 16) == L.EINVAL
    assert _ah(sha256, 16, csp_cipher_alg=L.CRYPTO_NULL_CBC) == L.EINVAL
    assert _ah(sha256, 16, csp_cipher_klen=16, csp_cipher_key=b"k" * 16) == L.EINVAL
    assert _ah(sha256, 16, csp_ivlen=16) == L.EINVAL
    assert _ah(sha256, 10) == L.EINVAL                                # not a multiple of 4
    assert _ah(sha256, 36) == L.EINVAL                                # above the hash size
    assert _ah(L.CRYPTO_SHA1_HMAC, 24) == L.EINVAL
    assert _ah(L.CRYPTO_SHA2_384_HMAC, 52) == L.EINVAL
    assert _ah(L.CRYPTO_SHA2_512_HMAC, 68) == L.EINVAL
    assert _ah(sha256, 16, flags=L.CSP_F_SEPARATE_AAD) == L.EINVAL
    assert _ah(sha256, 16, flags=CSP_F_SEPARATE_OUTPUT) == L.EINVAL
    assert _ah(sha256, 16, klen=0) == L.EINVAL
    assert _probe(csp_mode=L.CSP_MODE_DIGEST, csp_auth_alg=sha256, csp_auth_klen=32, csp_auth_key=None,
                  csp_auth_mlen=16) == L.EINVAL                        # no session key


def test_csp_follows_ah_init():
    rng = np.random.default_rng(4)
    want = {1: (L.CRYPTO_SHA1_HMAC, 12), 256: (L.CRYPTO_SHA2_256_HMAC, 16), 384: (L.CRYPTO_SHA2_384_HMAC, 24),
            512: (L.CRYPTO_SHA2_512_HMAC, 32)}
    for sha, (aalg, authsize) in want.items():
        for esn in (False, True):
            s = AhSA(rng, sha, esn=esn)
            c = s.csp()
            assert s.sa.authsize == authsize and s.sa.rplen == 12
            assert c.csp_mode == L.CSP_MODE_DIGEST and c.csp_flags == (L.CSP_F_ESN if esn else 0)
            assert (c.csp_auth_alg, c.csp_auth_klen, c.csp_auth_key, c.csp_auth_mlen) == (aalg, len(s.key), s.key,
                                                                                          authsize)
            assert (c.csp_cipher_alg, c.csp_cipher_klen, c.csp_cipher_key, c.csp_ivlen) == (0, 0, None, 0)


@pytest.mark.parametrize("v", golden_ah(), ids=lambda v: v["name"])
def test_massage_and_hmac_reproduce_golden_icv(v):
    sa = golden_sa(v)
    out = bytearray.fromhex(v["output"])
    at = SKIP + sa.sa.rplen
    icv = bytes(out[at:at + 16])
    out[:SKIP] = A.ah_massage_ipv4(out, SKIP, 1)
    assert out[1] == 0 and out[6:8] == b"\0\0" and out[8] == 0 and out[10:12] == b"\0\0"
    assert sa.icv_hole(out, at) == icv
    assert icv.hex().startswith({"pkt_ah_tunnel_sha256": "59fdb4db", "pkt_ah_transport_sha256": "6c2ef71f"}[v["name"]])


def test_massage_ipv4_options():
    hdr = bytearray(bytes([0x4f, 0x55, 0, 100, 1, 2, 0x40, 0, 64, 51, 0xab, 0xcd]) + bytes(range(8)))
    # NOP, router alert (kept), LSRR with one address (zeroed; its last address = the destination on
    # output), a timestamp option (zeroed), EOL and what follows it (left alone)
    opts = bytes([1, 0x94, 4, 0, 0, 0x83, 7, 4, 9, 9, 9, 9, 0x44, 4, 5, 0, 0, 0xff, 0xee]) + bytes(21)
    pkt = hdr + opts + b"payload!"
    skip = 20 + len(opts)
    for out in (0, 1):
        m = A.ah_massage_ipv4(pkt, skip, out)
        assert len(m) == skip and m[1] == 0 and m[6:8] == b"\0\0" and m[8] == 0 and m[10:12] == b"\0\0"
        assert m[0] == 0x4f and m[2:6] == bytes(hdr[2:6]) and m[9] == 51 and m[12:16] == bytes(hdr[12:16])
        assert m[16:20] == (bytes([9, 9, 9, 9]) if out else bytes(hdr[16:20]))
        assert m[20:25] == opts[0:5] and m[25:32] == bytes(7) and m[32:36] == bytes(4)
        assert m[36:] == opts[16:]
    with pytest.raises(ValueError):
        A.ah_massage_ipv4(hdr + bytes([0x44, 1, 0, 0]), 24, 0)        # option length < 2
    with pytest.raises(ValueError):
        A.ah_massage_ipv4(hdr + bytes([0x44, 8, 0, 0]), 24, 0)        # option runs past the header


def test_massage_ipv6_basic_header():
    h = bytes([0x6a, 0xbc, 0xde, 0xf0, 0, 64, 51, 63]) + bytes([0xfe, 0x80, 0x12, 0x34]) + bytes(range(12)) + \
        bytes([0x20, 0x01, 0x0d, 0xb8]) + bytes(range(12))
    m = A.ah_massage_ipv6(h + b"rest")
    assert m[0:4] == b"\x60\0\0\0" and m[4:7] == h[4:7] and m[7] == 0
    assert m[8:12] == bytes([0xfe, 0x80, 0, 0]) and m[12:24] == h[12:24] and m[24:40] == h[24:40]
    with pytest.raises(ValueError):
        A.ah_massage_ipv6(bytes([0x60, 0, 0, 0, 0, 0]) + bytes(34))   # jumbogram


class _SoftFramework:
    """crypto_getreq / crypto_dispatch with swcr_authcompute played by oracle.hmac."""

    def __init__(self, sa):
        self.sa = sa

    def crypto_getreq(self, ses):
        return cryptop(ses)

    def crypto_dispatch(self, crp):
        assert crp.crp_op == L.CRYPTO_OP_COMPUTE_DIGEST and crp.crp_aad is None and crp.crp_aad_length == 0
        buf = crp.crp_buf
        msg = bytes(buf[crp.crp_payload_start:crp.crp_payload_start + crp.crp_payload_length])
        buf[crp.crp_digest_start:crp.crp_digest_start + self.sa.mlen] = self.sa.icv(msg)
        return 0


@pytest.mark.parametrize("v", golden_ah(), ids=lambda v: v["name"])
def test_input_crp_and_cb_on_golden_packets(v):
    sa = golden_sa(v)
    fw = _SoftFramework(sa)
    good = bytes.fromhex(v["output"])
    at = SKIP + sa.sa.rplen

    def run(pkt):
        pkt = bytearray(pkt)
        crp = A.ah_input_crp(fw, None, sa.sa, pkt, SKIP)
        assert (crp.crp_payload_start, crp.crp_payload_length, crp.crp_digest_start) == (0, len(pkt), at)
        assert pkt[at:at + 16] == bytes(16)                            # zeroed before the digest
        assert fw.crypto_dispatch(crp) == 0
        return A.ah_input_cb(crp.crp_opaque, pkt)

    assert run(good)
    # mutable fields may change in flight: TOS, flags / offset, TTL, checksum
    mut = bytearray(good)
    mut[1], mut[8] = 0x2e, 7
    mut[6:8], mut[10:12] = b"\x40\x00", b"\x12\x34"
    assert run(mut)
    for pos in (len(good) - 1, SKIP + 30, at, at + 15, 12, 16, 9, 3, SKIP + 5):   # payload, ICV, immutable header, AH header
        bad = bytearray(good)
        bad[pos] ^= 0x10
        assert not run(bad), pos


@pytest.mark.parametrize("v", golden_ah(), ids=lambda v: v["name"])
def test_output_crp_reproduces_golden_packet(v):
    sa = golden_sa(v)
    fw = _SoftFramework(sa)
    good = bytes.fromhex(v["output"])
    at = SKIP + sa.sa.rplen
    pkt = bytearray(good)
    pkt[at:at + 16] = b"\xa5" * 16                                     # whatever was there
    crp = A.ah_output_crp(fw, None, sa.sa, pkt, SKIP)
    assert fw.crypto_dispatch(crp) == 0
    pkt[:SKIP] = crp.crp_opaque                                        # ah_output_cb restores the header
    assert bytes(pkt) == good
    assert O.hmac(O.CRYPTO_SHA2_256_HMAC, sa.key, b"") != b""          # (the checker is loaded)
