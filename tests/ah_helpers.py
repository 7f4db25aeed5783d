"""Shared fixtures of the AH (CSP_MODE_DIGEST) tests: SAs, golden packets and
the checker, oracle.hmac (pinned to hashlib in test_oracle.py)."""
import json
import os

import numpy as np

import oracle as O
from espgpu import ah as A

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DESC = np.dtype([("off4", "<u4"), ("len", "<u2"), ("sa", "<u2"), ("esn_hi", "<u4"), ("salt", "<u4")])
AALG = {1: O.CRYPTO_SHA1_HMAC, 256: O.CRYPTO_SHA2_256_HMAC, 384: O.CRYPTO_SHA2_384_HMAC,
        512: O.CRYPTO_SHA2_512_HMAC}
ALG = {1: A.AH_SHA1, 256: A.AH_SHA256, 384: A.AH_SHA384, 512: A.AH_SHA512}
BLOCK = {1: 64, 256: 64, 384: 128, 512: 128}
SKIP = 20                                  # IPv4 header without options


def golden_ah():
    with open(os.path.join(GOLDEN, "ah_packets.json")) as f:
        return json.load(f)


class AhSA:
    """An AH SA: HMAC-SHA1-96 or HMAC-SHA2-256-128 / -384-192 / -512-256
    (sha: 1, 256, 384, 512), its key and the espgpu.ah view of it."""

    def __init__(self, rng, sha=256, esn=False, mlen=None, key=None, aklen=None):
        self.sha = sha
        if key is None:
            aklen = {1: 20, 256: 32, 384: 48, 512: 64}[sha] if aklen is None else aklen
            key = rng.integers(0, 256, aklen, dtype=np.uint8).tobytes()
        self.key = bytes(key)
        self.esn = esn
        self.sa = A.AhSecAssoc(int(rng.integers(256, 2**32 - 1)), ALG[sha], self.key, esn=esn, mlen=mlen)
        self.mlen = self.sa.mlen

    def csp(self):
        return self.sa.csp()

    def icv(self, msg, esn_hi=0):
        """The first mlen bytes of HMAC(key, msg || be32(esn_hi) for ESN SAs)."""
        m = bytes(msg) + (int(esn_hi).to_bytes(4, "big") if self.esn else b"")
        return O.hmac(AALG[self.sha], self.key, m)[:self.mlen]

    def icv_hole(self, rec, at, esn_hi=0):
        """The ICV of a record whose ICV field at `at` reads as zeros."""
        r = bytearray(rec)
        r[at:at + self.mlen] = bytes(self.mlen)
        return self.icv(r, esn_hi)


def golden_sa(v, rng=None):
    return AhSA(rng if rng is not None else np.random.default_rng(0), 256, key=bytes.fromhex(v["key"]))
