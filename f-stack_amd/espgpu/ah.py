"""AH request builders, the caller side of the digest path (unchanged semantics).

  AhSecAssoc.csp()    ah_init / ah_init0     freebsd/netipsec/xform_ah.c:150-246
  AhSecAssoc.authsize xform_ah_authsize      xform_ah.c:116-141
  ah_massage_ipv4()   ah_massage_headers     xform_ah.c:279-392 (AF_INET)
  ah_massage_ipv6()   ah_massage_headers     xform_ah.c:395-422 (the basic header;
                                             extension headers are out of scope)
  ah_input_crp()      ah_input               xform_ah.c:613-664
  ah_input_cb()       ah_input_cb's compare  xform_ah.c:735-749
  ah_output_crp()     ah_output              xform_ah.c:972-1047
Packets are IP packets with the AH header (struct newah: next header, length,
reserved, SPI, sequence number, then the ICV) at `skip`, in a bytearray or an
mbuf-like list of bytearrays.
"""
import struct

from . import _lib as L
from .opencrypto import crypto_session_params

AH_SHA1, AH_SHA256, AH_SHA384, AH_SHA512 = ("ah-hmac-sha1-96", "ah-hmac-sha2-256-128", "ah-hmac-sha2-384-192",
                                            "ah-hmac-sha2-512-256")
# auth algorithm, hash size
_ALG = {AH_SHA1: (L.CRYPTO_SHA1_HMAC, 20), AH_SHA256: (L.CRYPTO_SHA2_256_HMAC, 32),
        AH_SHA384: (L.CRYPTO_SHA2_384_HMAC, 48), AH_SHA512: (L.CRYPTO_SHA2_512_HMAC, 64)}
AH_ALGS = tuple(_ALG)
AH_HMAC_HASHLEN = 12                       # netipsec/ah.h
IPPROTO_AH = 51
IPOPT_EOL, IPOPT_NOP, IPOPT_LSRR, IPOPT_SSRR = 0, 1, 0x83, 0x89
_IPOPT_KEEP = (0x82, 0x85, 0x86, 0x94, 0x95)   # security, extended / commercial security, router alert, RFC 1770


class AhSecAssoc:
    """What key_setsaval leaves in struct secasvar for an AH SA."""

    rplen = 12                             # HDRSIZE: sizeof(struct newah), the header before the ICV

    def __init__(self, spi, alg, key, esn=False, mlen=None):
        self.spi = spi
        self.alg = alg
        self.key = bytes(key)
        self.esn = esn
        self.mlen = mlen if mlen is not None else self.authsize

    @property
    def auth_alg(self):
        return _ALG[self.alg][0]

    @property
    def hashsize(self):
        return _ALG[self.alg][1]

    @property
    def authsize(self):
        """xform_ah_authsize: hashsize / 2 for SHA2 (RFC 4868 2.3), else 12."""
        return AH_HMAC_HASHLEN if self.alg == AH_SHA1 else self.hashsize // 2

    def csp(self):
        """ah_init: CSP_MODE_DIGEST, CSP_F_ESN for ESN SAs; ah_init0: the
        auth algorithm, key and csp_auth_mlen = AUTHSIZE; no cipher, no IV."""
        return crypto_session_params(
            csp_mode=L.CSP_MODE_DIGEST, csp_flags=L.CSP_F_ESN if self.esn else 0,
            csp_auth_alg=self.auth_alg, csp_auth_klen=len(self.key), csp_auth_key=self.key,
            csp_auth_mlen=self.mlen)


def _flat(buf):
    return bytes(buf) if not isinstance(buf, list) else b"".join(bytes(b) for b in buf)


def _copyback(pkt, off, data):
    """m_copyback: data into the buffer (a bytearray or a chain) at off."""
    if not isinstance(pkt, list):
        pkt[off:off + len(data)] = data
        return
    for b in pkt:
        if off >= len(b):
            off -= len(b)
            continue
        k = min(len(data), len(b) - off)
        b[off:off + k] = data[:k]
        data = data[k:]
        off = 0
        if not data:
            return


def ah_massage_ipv4(pkt, skip, out):
    """ah_massage_headers for AF_INET, on the first `skip` bytes (the IP
    header with its options) of `pkt`: TOS (ah_cleartos), TTL, checksum and
    the fragment field zeroed; the option loop.  -> the massaged header
    (bytes); raises ValueError where the kernel answers EINVAL."""
    ptr = bytearray(_flat(pkt)[:skip])
    ptr[1] = 0                              # ip_tos (V_ah_cleartos = 1)
    ptr[8] = 0                              # ip_ttl
    ptr[10:12] = b"\0\0"                    # ip_sum
    ptr[6:8] = b"\0\0"                      # ip_off
    off = 20
    while off < skip:
        o = ptr[off]
        if not (o == IPOPT_EOL or o == IPOPT_NOP or off + 1 < skip):
            raise ValueError("illegal IPv4 option length for option %d" % o)
        if o == IPOPT_EOL:
            off = skip
        elif o == IPOPT_NOP:
            off += 1
        elif o in _IPOPT_KEEP:
            if ptr[off + 1] < 2:
                raise ValueError("illegal IPv4 option length for option %d" % o)
            off += ptr[off + 1]
        else:
            if ptr[off + 1] < 2:
                raise ValueError("illegal IPv4 option length for option %d" % o)
            if o in (IPOPT_LSRR, IPOPT_SSRR) and out:
                # the destination the receiver will see: the option's last address
                ptr[16:20] = ptr[off + ptr[off + 1] - 4:off + ptr[off + 1]]
            count = ptr[off + 1]
            ptr[off:off + count] = bytes(count)          # every other option zeroed
            off += count
        if off > skip:
            raise ValueError("malformed IPv4 options header")
    return bytes(ptr[:skip])


def ah_massage_ipv6(pkt):
    """ah_massage_headers for AF_INET6, the basic header only: flow label and
    traffic class, hop limit zeroed, version kept; link-local scope ids
    cleared.  -> the massaged 40-byte header."""
    h = bytearray(_flat(pkt)[:40])
    if h[4:6] == b"\0\0":
        raise ValueError("unsupported IPv6 jumbogram")
    h[0:4] = b"\x60\0\0\0"                  # ip6_flow = 0, ip6_vfc = IPV6_VERSION
    h[7] = 0                                # ip6_hlim
    for a in (8, 24):                       # IN6_IS_SCOPE_LINKLOCAL: fe80::/10
        if h[a] == 0xfe and (h[a + 1] & 0xc0) == 0x80:
            h[a + 2:a + 4] = b"\0\0"
    return bytes(h)


def _massage(pkt, skip, out):
    ver = _flat(pkt)[0] >> 4
    hdr = ah_massage_ipv6(pkt) if ver == 6 else ah_massage_ipv4(pkt, skip, out)
    _copyback(pkt, 0, hdr)


def _digest_crp(fw, ses, sa, pkt, skip, esn_hi):
    crp = fw.crypto_getreq(ses)
    crp.crp_payload_start = 0
    crp.crp_payload_length = len(_flat(pkt))
    crp.crp_digest_start = skip + sa.rplen
    crp.crp_op = L.CRYPTO_OP_COMPUTE_DIGEST
    crp.crp_flags = L.CRYPTO_F_CBIFSYNC
    crp.crp_buf = pkt
    if sa.esn:
        crp.crp_esn = struct.pack(">I", esn_hi)
    return crp


class AhXformData:
    """ah_input's xform_data: the skipped headers, the AH header and the
    authenticator as they arrived."""

    def __init__(self, saved, skip, mlen):
        self.saved = bytes(saved)
        self.skip = skip
        self.mlen = mlen


def ah_input_crp(fw, ses, sa, pkt, skip, esn_hi=0):
    """The cryptop ah_input builds: the authenticator and the headers saved
    (crp.crp_opaque, an AhXformData), the authenticator zeroed on the packet,
    the headers massaged, COMPUTE_DIGEST over the whole packet."""
    xd = AhXformData(_flat(pkt)[:skip + sa.rplen + sa.mlen], skip, sa.mlen)
    _copyback(pkt, skip + sa.rplen, bytes(sa.mlen))
    _massage(pkt, skip, 0)
    crp = _digest_crp(fw, ses, sa, pkt, skip, esn_hi)
    crp.crp_opaque = xd
    return crp


def ah_input_cb(saved, pkt):
    """ah_input_cb's verdict: the computed authenticator (on the packet at
    skip + rplen) against the one ah_input saved (`saved`: the request's
    crp_opaque).  True = authentic."""
    at = saved.skip + AhSecAssoc.rplen
    return saved.saved[at:at + saved.mlen] == _flat(pkt)[at:at + saved.mlen]


def ah_output_crp(fw, ses, sa, pkt, skip, esn_hi=0):
    """The cryptop ah_output builds over a packet that already holds the AH
    header at `skip` (next header, length, SPI, sequence number): the
    authenticator zeroed, the headers massaged (the caller restores the
    saved `skip` bytes afterwards, ah_output_cb), COMPUTE_DIGEST."""
    saved = _flat(pkt)[:skip]
    _copyback(pkt, skip + sa.rplen, bytes(sa.mlen))
    _massage(pkt, skip, 1)
    crp = _digest_crp(fw, ses, sa, pkt, skip, esn_hi)
    crp.crp_opaque = saved
    return crp
