"""AH sessions under F-Stack's own opencrypto framework with the MI355X driver.

The executables of integration/fstack_run.py (F-Stack's crypto.c, cryptosoft
and gpucrypto in one process; see tests/test_fstack_run.py) started with
FF_GPUCRYPTO_AH=1, the binding's switch for AH offload:
  * every CSP_MODE_DIGEST session ah_init builds (the four HMACs, with and
    without ESN) must select gpucrypto under esp_init's crid;
  * every request -- ah_output's and ah_input's over DPDK's AH known-answer
    packets, and random packets of every length class, contiguous and as
    mbuf chains cut inside the IP header, the ICV field and the last dword --
    must come back byte for byte as cryptosoft's own run of it, and carry the
    ICV oracle.hmac computes.
Without the switch AH stays on cryptosoft: tests/test_fstack_run.py.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

from ah_helpers import SKIP, AhSA, golden_ah, golden_sa
from espgpu import ah as A
from espgpu.opencrypto import cryptop

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "integration"))
import fstack_run as FR  # noqa: E402


class _Fw:
    def crypto_getreq(self, ses):
        return cryptop(ses)


def _sess(csp):
    return dict(mode=csp.csp_mode, flags=csp.csp_flags, ivlen=csp.csp_ivlen, calg=csp.csp_cipher_alg,
                cklen=csp.csp_cipher_klen, aalg=csp.csp_auth_alg, aklen=csp.csp_auth_klen,
                mlen=csp.csp_auth_mlen, ckey=csp.csp_cipher_key, akey=csp.csp_auth_key)


def _req(si, crp, cuts):
    """The request as dispatched: crp_buf is the packet after ah_input /
    ah_output zeroed the authenticator and massaged the headers."""
    return dict(ses=si, op=crp.crp_op, flags=crp.crp_flags, aad_start=crp.crp_aad_start,
                aad_len=crp.crp_aad_length, iv_start=crp.crp_iv_start, payload_start=crp.crp_payload_start,
                payload_len=crp.crp_payload_length, digest_start=crp.crp_digest_start, aad=None,
                esn=bytes(crp.crp_esn), iv=bytes(crp.crp_iv), mbuf=cuts is not None, cuts=cuts or [],
                buf=bytes(crp.crp_buf))


BSD_EBADMSG = 89
CRYPTO_OP_VERIFY_DIGEST = 0x2


def _expect(sa, crp, esn_hi=0):
    """COMPUTE_DIGEST: the dispatched buffer with the ICV at crp_digest_start, nothing else
    changed.  VERIFY_DIGEST hashes the digest field too (swcr_authcompute), so it cannot
    match: EBADMSG, the buffer untouched."""
    if crp.crp_op & CRYPTO_OP_VERIFY_DIGEST:
        return BSD_EBADMSG, bytes(crp.crp_buf)
    buf = bytearray(crp.crp_buf)
    at = crp.crp_digest_start
    buf[at:at + sa.mlen] = sa.icv(bytes(crp.crp_buf), esn_hi)
    return 0, bytes(buf)


def _workload():
    sessions, reqs, want = [], [], []
    rng = np.random.default_rng(5200)
    at = SKIP + A.AhSecAssoc.rplen

    def add(sa, crp, cuts, esn_hi=0):
        reqs.append(_req(sa.si, crp, cuts))
        want.append(_expect(sa, crp, esn_hi))

    # DPDK's AH packets: ah_input's request (the ICV recomputed over the zeroed,
    # massaged packet = the packet's own) and ah_output's
    for v in golden_ah():
        sa = golden_sa(v, rng)
        sessions.append(_sess(sa.csp()))
        sa.si = len(sessions) - 1
        good = bytes.fromhex(v["output"])
        for cuts in (None, [7, at + 5, len(good) - 2]):
            crp = A.ah_input_crp(_Fw(), sa.si, sa.sa, bytearray(good), SKIP)
            add(sa, crp, cuts)
            assert want[-1][1][at:at + 16] == good[at:at + 16]           # the known answer
            dirty = bytearray(good)
            dirty[at:at + 16] = b"\x5a" * 16
            add(sa, A.ah_output_crp(_Fw(), sa.si, sa.sa, dirty, SKIP), cuts)
            assert want[-1][1][at:at + 16] == good[at:at + 16]
    # every HMAC, with and without ESN: packets whose length covers the padding
    # boundaries of the hash block, the smallest AH packet, an MTU and a jumbo
    for sha in (1, 256, 384, 512):
        for esn in (False, True):
            sa = AhSA(rng, sha, esn=esn)
            sessions.append(_sess(sa.csp()))
            sa.si = len(sessions) - 1
            blk = 128 if sha >= 384 else 64
            lens = [at + sa.mlen, blk, blk + 1, 2 * blk - 9, 2 * blk - 8 - (4 if esn else 0), 2 * blk - 1, 3 * blk + 3,
                    1500, 9001]
            for k, n in enumerate(lens):
                n = max(n, at + sa.mlen)
                pkt = bytearray(rng.integers(0, 256, n, dtype=np.uint8).tobytes())
                pkt[0] = 0x45
                eh = int(rng.integers(0, 2**32)) if esn else 0
                build = A.ah_input_crp if k % 2 else A.ah_output_crp
                crp = build(_Fw(), sa.si, sa.sa, pkt, SKIP, esn_hi=eh)
                # chains cut inside the IP header, the ICV field and the last dword
                cuts = None if k % 3 == 0 else sorted(set([5, at + 3, n - 2] + list(range(2000, n, 2000))))
                add(sa, crp, cuts, eh)
            # a VERIFY_DIGEST request over a signed packet
            pkt = bytearray(want[-1][1])
            crp = A.ah_output_crp(_Fw(), sa.si, sa.sa, bytearray(pkt), SKIP, esn_hi=eh)
            crp.crp_buf = pkt
            crp.crp_op = CRYPTO_OP_VERIFY_DIGEST
            add(sa, crp, sorted(set([at + 1] + list(range(2000, len(pkt), 2000)))), eh)   # (mbufs <= MCLBYTES)
    return sessions, reqs, want


@pytest.fixture(scope="module")
def workload():
    return _workload()


def _run(exe, workload, tmp_path):
    sessions, reqs, want = workload
    rq, rs = str(tmp_path / "req.bin"), str(tmp_path / "res.bin")
    FR.pack_requests(rq, sessions, reqs)
    p = subprocess.run([exe, rq, rs], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, FF_GPUCRYPTO_AH="1"))
    assert p.returncode == 0, (p.returncode, p.stdout[-2000:], p.stderr[-4000:])
    assert "fstack_crypto_run OK" in p.stdout
    return FR.read_results(rs, [len(r["buf"]) for r in reqs])


def _check(res, workload):
    sessions, reqs, want = workload
    gpu_hid, sw_hid, ses, out = res
    assert gpu_hid >= 0 and sw_hid >= 0 and gpu_hid != sw_hid
    for i, (err_d, hid_d, err_s, hid_s) in enumerate(ses):
        assert err_d == 0 and hid_d == gpu_hid, (i, err_d, hid_d)        # AH offload on: gpucrypto
        assert err_s == 0 and hid_s == sw_hid, (i, err_s, hid_s)
    assert len(out) == len(want)
    for i, (r, (etype, exp)) in enumerate(zip(out, want)):
        assert r["dispatch"] == 0 and r["dispatch_sw"] == 0, i
        assert r["done_flag"] == 1 and r["done_flag_sw"] == 1, i
        assert r["etype"] == etype and r["etype_sw"] == etype, (i, r["etype"], r["etype_sw"])
        assert r["buf"] == r["buf_sw"], i                                # byte for byte as cryptosoft
        assert r["buf"] == exp, i                                        # and as oracle.hmac


HAVE_REF = os.path.isdir("/root/reference/lib")
MISSING_GPU_EXE = ("oracle/_ref/fstack_crypto_run_gpu missing: run __graft_entry__.build() where the F-Stack tree "
                   "exists and bring oracle/_ref/ along")


@pytest.fixture(scope="module")
def built(tmp_path_factory):
    if HAVE_REF:
        FR.build("/root/reference", str(tmp_path_factory.mktemp("fstack_run_build") / "w"))
    return FR.EXE_CPU, FR.EXE_GPU


def test_ah_under_fstack_opencrypto_cpu(built, workload, tmp_path):
    """The CPU executable (oracle stand-in behind the host shim interface)."""
    exe = built[0]
    if not os.path.exists(exe):
        pytest.skip("needs the F-Stack tree to build oracle/_ref/fstack_crypto_run_cpu")
    _check(_run(exe, workload, tmp_path), workload)


@pytest.mark.gpu
def test_ah_under_fstack_opencrypto_gpu(workload, tmp_path):
    """The GPU executable: F-Stack's crypto.c, the kernel-domain driver, the
    real host shim with AH offload on and libespgpu.so on the MI355X."""
    exe = FR.EXE_GPU
    assert os.path.exists(exe), MISSING_GPU_EXE                          # a failure, not a skip
    _check(_run(exe, workload, tmp_path), workload)
