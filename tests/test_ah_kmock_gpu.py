"""AH sessions through the kernel-domain driver F-Stack links
(integration/ff_gpucrypto.c over integration/kmock, the host shim and
libespgpu.so; see tests/test_kmock_driver_gpu.py for the chain).

The binding offers CSP_MODE_DIGEST sessions only when asked: with AH offload
off (the default) crypto_newsession lands on the software driver; after
ff_gpucrypto_host_tune("ah", 1) it lands on gpucrypto, and the requests
ah_output / ah_input build complete with cryptosoft's results and errno
mapping (FreeBSD EBADMSG 89, EINVAL 22)."""
import ctypes as C
import os
import time

import numpy as np
import pytest

from ah_helpers import SKIP, AhSA, golden_ah, golden_sa

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KD_LIB = os.path.join(ROOT, "integration", "libkmockdrv.so")
BSD_EBADMSG, BSD_EINVAL = 89, 22
CRYPTO_OP_COMPUTE_DIGEST, CRYPTO_OP_VERIFY_DIGEST, CRYPTO_OP_ENCRYPT = 0, 2, 1


class _Fw:
    def crypto_getreq(self, ses):
        from espgpu.opencrypto import cryptop
        return cryptop(ses)


@pytest.fixture
def kd():
    if not torch.cuda.is_available():
        pytest.fail("GPU test run without a visible HIP device")
    L = C.CDLL(KD_LIB)
    vp, i = C.c_void_p, C.c_int
    L.kd_open.argtypes = [i, i, i, i]
    L.kd_newsession.argtypes = [i, i, i, i, i, vp, i, i, vp, i, C.POINTER(vp)]
    L.kd_freesession.argtypes = [vp]
    L.kd_request.restype = vp
    L.kd_request.argtypes = [vp, i, i, i, C.POINTER(vp), C.POINTER(i), i, vp, i, i, vp, vp, i, i, i, i]
    L.kd_dispatch.argtypes = [vp]
    L.kd_result.argtypes = [vp]
    L.kd_free.argtypes = [vp]
    L.kd_tune.argtypes = [C.c_char_p, i]
    L.kd_soft.argtypes = [vp]
    assert L.kd_open(64, 2, 4 << 20, 1) == 0
    L.kd_soft_enable(1)
    try:
        yield L
    finally:
        L.kd_tune(b"ah", 0)
        L.kd_soft_enable(0)
        L.kd_close()
        from espgpu import _lib
        _lib.lib().espgpu_set_tuning(None, b"ah_offer", -1)   # the engine's bid back to its default


def _newsession(L, csp):
    ak = C.create_string_buffer(bytes(csp.csp_auth_key), csp.csp_auth_klen)
    h = C.c_void_p()
    e = L.kd_newsession(csp.csp_mode, csp.csp_flags, csp.csp_ivlen, csp.csp_cipher_alg, csp.csp_cipher_klen, None,
                        csp.csp_auth_alg, csp.csp_auth_klen, C.cast(ak, C.c_void_p), csp.csp_auth_mlen, C.byref(h))
    return e, h.value


def _soft_sessions(L):
    a = (C.c_int * 4)()
    L.kd_soft(a)
    return a[0]


def _request(L, keep, ses, crp, bufs):
    chain = isinstance(bufs, list)
    segs = bufs if chain else [bufs]
    arrs = [(C.c_char * len(b)).from_buffer(b) for b in segs]
    bases = (C.c_void_p * len(segs))(*[C.addressof(a) for a in arrs])
    lens = (C.c_int * len(segs))(*[len(b) for b in segs])
    esn = C.create_string_buffer(bytes(crp.crp_esn)[:4], 4)
    iv = C.create_string_buffer(bytes(16), 16)
    r = L.kd_request(ses, crp.crp_op, crp.crp_flags, int(chain), bases, lens, len(segs), None, crp.crp_aad_start,
                     crp.crp_aad_length, esn, iv, crp.crp_iv_start, crp.crp_payload_start, crp.crp_payload_length,
                     crp.crp_digest_start)
    assert r
    keep.append((arrs, bases, lens))
    return r


def _wait(L, reqs, timeout_s=60.0):
    t_end = time.monotonic() + timeout_s
    while time.monotonic() < t_end:
        res = [L.kd_result(r) for r in reqs]
        if min(res) >= 0:
            return res
        for _ in range(64):
            L.kd_poll()
    raise AssertionError("requests did not complete")


def test_ah_session_lands_on_software_unless_switched_on(kd):
    L = kd
    rng = np.random.default_rng(8200)
    sa = AhSA(rng, 256)
    e, s0 = _newsession(L, sa.csp())
    assert e == 0 and _soft_sessions(L) == 1                 # AH off: the software driver keeps it
    assert L.kd_tune(b"ah", 2) != 0                          # 0 or 1
    assert L.kd_tune(b"ah", 1) == 0
    e, s1 = _newsession(L, sa.csp())
    assert e == 0 and _soft_sessions(L) == 1                 # on gpucrypto
    assert L.kd_tune(b"ah", 0) == 0
    e, s2 = _newsession(L, sa.csp())
    assert e == 0 and _soft_sessions(L) == 2
    for s in (s0, s1, s2):
        L.kd_freesession(s)


def test_ah_requests_through_the_kernel_driver(kd):
    from espgpu import ah as A
    L = kd
    assert L.kd_tune(b"ah", 1) == 0
    rng = np.random.default_rng(8300)
    keep, reqs, checks = [], [], []
    at = SKIP + 12
    sessions = []
    # DPDK's AH packets, ah_input's and ah_output's request
    for v in golden_ah():
        sa = golden_sa(v)
        e, ses = _newsession(L, sa.csp())
        assert e == 0
        sessions.append(ses)
        good = bytes.fromhex(v["output"])
        for chain in (False, True):
            pkt = bytearray(good)
            pkt[at:at + 16] = b"\x33" * 16
            crp = A.ah_output_crp(_Fw(), None, sa.sa, pkt, SKIP)
            want = bytearray(pkt)
            want[at:at + 16] = good[at:at + 16]
            bufs = pkt if not chain else [bytearray(pkt[a:b]) for a, b in ((0, 9), (9, at + 6), (at + 6, len(pkt)))]
            reqs.append(_request(L, keep, ses, crp, bufs))
            checks.append((0, bufs, bytes(want)))
    for sha in (1, 256, 384, 512):
        for esn in (False, True):
            sa = AhSA(rng, sha, esn=esn)
            e, ses = _newsession(L, sa.csp())
            assert e == 0
            sessions.append(ses)
            for k, n in enumerate((at + sa.mlen, 127, 128, 129, 1500)):
                n = max(n, at + sa.mlen)
                pkt = bytearray(rng.integers(0, 256, n, dtype=np.uint8).tobytes())
                pkt[0] = 0x45
                eh = int(rng.integers(0, 2**32))
                crp = (A.ah_input_crp if k % 2 else A.ah_output_crp)(_Fw(), None, sa.sa, pkt, SKIP, esn_hi=eh)
                want = bytearray(pkt)
                want[at:at + sa.mlen] = sa.icv(bytes(pkt), eh)
                bufs = pkt if k % 2 == 0 else [bytearray(pkt[a:b]) for a, b in ((0, 3), (3, at + 1), (at + 1, n - 1),
                                                                                    (n - 1, n))]
                reqs.append(_request(L, keep, ses, crp, bufs))
                checks.append((0, bufs, bytes(want)))
                # VERIFY over the signed packet hashes the digest field too: EBADMSG, as cryptosoft
                vb = bytearray(want)
                crp.crp_op = CRYPTO_OP_VERIFY_DIGEST
                reqs.append(_request(L, keep, ses, crp, vb))
                checks.append((BSD_EBADMSG, vb, bytes(want)))
            # malformed: the ENCRYPT bit, a digest field outside the range
            bad = bytearray(200)
            crp = A.ah_output_crp(_Fw(), None, sa.sa, bytearray(bad), SKIP)
            crp.crp_op = CRYPTO_OP_ENCRYPT
            reqs.append(_request(L, keep, ses, crp, bad))
            checks.append((BSD_EINVAL, bad, bytes(200)))
            bad2 = bytearray(200)
            crp = A.ah_output_crp(_Fw(), None, sa.sa, bytearray(bad2), SKIP)
            crp.crp_digest_start = 200 - sa.mlen + 4
            reqs.append(_request(L, keep, ses, crp, bad2))
            checks.append((BSD_EINVAL, bad2, bytes(200)))
    assert _soft_sessions(L) == 0
    for r in reqs:
        assert L.kd_dispatch(r) == 0
    res = _wait(L, reqs)
    for i, (et, (want_et, bufs, want)) in enumerate(zip(res, checks)):
        assert et == want_et, (i, et, want_et)
        got = bytes(bufs) if not isinstance(bufs, list) else b"".join(bytes(b) for b in bufs)
        assert got == want, i
    for r in reqs:
        L.kd_free(r)
    for s in sessions:
        L.kd_freesession(s)
