"""AH request builders, the caller side of the digest path (unchanged semantics).

  AhSecAssoc.csp()    ah_init / ah_init0     freebsd/netipsec/xform_ah.c:150-246
  AhSecAssoc.authsize xform_ah_authsize      xform_ah.c:116-141
  ah_massage_ipv4()   ah_massage_headers     xform_ah.c:279-392 (AF_INET)
  ah_massage_ipv6()   ah_massage_headers     xform_ah.c:395-422 (the basic header;
                                             extension headers are out of scope)
  ah_input_crp()      ah_input               xform_ah.c:613-664
  ah_input_cb()       ah_input_cb's compare  xform_ah.c:735-749
  ah_output_crp()     ah_output              xform_ah.c:972-1047
The inbound AH stages of the device-resident batch path (include/espgpu.h, the
inbound AH block) are restated here on bytes:
  ipsec_input_classify_ah()  ip_input / ip6_input, ipsec_common_input for ip_p 51
                                             ipsec_input.c:141-208
  ah_hdrsiz()         ah_hdrsiz              xform_ah.c:144-169
  ah_input()          ah_input's length checks, save and massage
                                             xform_ah.c:576-600, :628-650
  ah_input_cb_decap() ah_input_cb after the compare, then
                      esp.ipsec_common_input_cb   xform_ah.c:758-814
The outbound AH stages (include/espgpu.h, the outbound AH block) likewise:
  ipsec_output_encap_ah()  ipsec4/6_perform_request, ipsec_encap, ah_output up
                      to the AH header   ipsec_output.c:221-242, :531-590,
                                             :882-992; xform_ah.c:855-935
  ah_output_seq()     ah_output's replay counter and SPI
                                             xform_ah.c:928, :937-958, :1045-1048
  ah_output()         the save and ah_massage_headers with out = 1
                                             xform_ah.c:988, :1027
  ah_output_cb()      ah_output_cb's m_copyback    xform_ah.c:1120
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


def ah_massage_ipv4(pkt, skip, out, cleartos=True):
    """ah_massage_headers for AF_INET, on the first `skip` bytes (the IP
    header with its options) of `pkt`: TOS (if cleartos: V_ah_cleartos, 1 by
    default), TTL, checksum and the fragment field zeroed; the option loop.
    -> the massaged header (bytes); raises ValueError where the kernel answers
    EINVAL."""
    ptr = bytearray(_flat(pkt)[:skip])
    if cleartos:
        ptr[1] = 0                          # ip_tos (V_ah_cleartos)
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
                if off + ptr[off + 1] > skip:           # (the reference swaps first and refuses at :386)
                    raise ValueError("malformed IPv4 options header")
                # the destination the receiver will see: the option's last address
                ptr[16:20] = ptr[off + ptr[off + 1] - 4:off + ptr[off + 1]]
            count = ptr[off + 1]
            ptr[off:off + count] = bytes(count)          # every other option zeroed
            off += count
        if off > skip:
            raise ValueError("malformed IPv4 options header")
    return bytes(ptr[:skip])


def ah_massage_ipv6(pkt, cleartos=True):
    """ah_massage_headers for AF_INET6, the basic header only: flow label and
    traffic class, hop limit zeroed, version kept; link-local scope ids
    cleared.  cleartos changes nothing here: ip6_flow is zeroed whatever
    V_ah_cleartos says (:410).  -> the massaged 40-byte header."""
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


# ---- the inbound AH stages of the device-resident batch path --------------------
IPPROTO_ESP = 50


def ipsec_input_classify_ah(sadb, pkt, off4=0, ipcsum=False, port=0):
    """esp.ipsec_input_classify_natt with the AH branch: what the stack does
    with a received ip_p / ip6_nxt 51 packet up to ah_input's first lines.
    ip_input's / ip6_input's checks as for ESP, then ipsec_common_input: the
    length check, here against struct newah up to the ICV (12 bytes; the
    reference answers EINVAL below 8, ipsec_input.c:141, and ENOBUFS from
    ah_input's pullup for 8..11: one code, EINVAL, is the engine's deliberate
    difference), the SPI at skip + 4 (:151-153) and key_allocsa with proto 51.
    No alignment check: that is esp_input's.  An IPv6 packet whose 40 + plen
    does not fit the descriptor's 16-bit length is the host stack's
    (ENOTSUP).  The descriptor of an accepted AH packet is the DIGEST record
    of the batch path: (off4, whole length, sa, 0, skip + 12).  Every other
    packet goes through esp.ipsec_input_classify_natt unchanged."""
    from . import esp as E
    raw = bytes(pkt)
    n = len(raw)
    v = raw[0] >> 4 if n >= 20 else 0
    isah = (v == 4 and raw[9] == IPPROTO_AH) or (v == 6 and n >= 40 and raw[6] == IPPROTO_AH)
    if not isah:
        return E.ipsec_input_classify_natt(sadb, raw, off4, ipcsum, port)
    def drop(status):
        return status, (off4, 0, 0xffff, 0, 0)

    if v == 4:
        hlen = (raw[0] & 0xf) << 2
        if hlen < 20 or hlen > n:
            return drop(L.EINVAL)
        if ipcsum and E.in_cksum(raw[:hlen]) != 0:
            return drop(L.EINVAL)
        ip_len, ip_off = struct.unpack(">H", raw[2:4])[0], struct.unpack(">H", raw[6:8])[0]
        if ip_len < hlen or n < ip_len:
            return drop(L.EINVAL)
        raw = raw[:ip_len]                                           # the trim, ip_input.c:555-561
        if ip_off & 0x3fff:                                          # IP_MF | IP_OFFMASK: ip_reass, the host's
            return drop(L.ENOTSUP)
        af, skip, dst = 4, hlen, raw[16:20]
    else:
        plen = struct.unpack(">H", raw[4:6])[0]
        if plen == 0:                                                # jumbo payload option
            return drop(L.ENOTSUP)
        if n - 40 < plen:                                            # ip6s_tooshort
            return drop(L.EINVAL)
        raw = raw[:40 + plen]
        af, skip, dst = 6, 40, raw[24:40]
        if dst[0] == 0xfe and dst[1] & 0xc0 == 0x80:                 # IN6_IS_SCOPE_LINKLOCAL
            return drop(L.ENOTSUP)
    if len(raw) - skip < AhSecAssoc.rplen:                           # ipsec_input.c:141 / ah_input's pullup
        return drop(L.EINVAL)
    if len(raw) > 65535:                                             # espgpu_desc.len
        return drop(L.ENOTSUP)
    spi = struct.unpack(">I", raw[skip + 4:skip + 8])[0]             # ipsec_input.c:151-153
    sav = sadb.get(spi) if spi else None
    if sav is None:
        return drop(L.ENOENT)
    sa, proto, saf, sdst = sav[:4]
    if proto != IPPROTO_AH or saf != af or bytes(sdst)[:len(dst)] != dst:    # key.c:1110-1118
        return drop(L.ENOENT)
    return 0, (off4, len(raw), sa, 0, skip + AhSecAssoc.rplen)


def ah_hdrsiz(mlen, af6):
    """ah_hdrsiz (xform_ah.c:144-169): roundup(HDRSIZE + AUTHSIZE, 4), or 8 for
    an AF_INET6 SA (RFC 4302)."""
    align = 8 if af6 else 4
    return (AhSecAssoc.rplen + mlen + align - 1) // align * align


def ah_input(af6, mlen, packet_bytes, skip, cleartos=True):
    """ah_input on bytes, without the replay check and the crypto request:
    the header-length checks (xform_ah.c:576-600), the save (:632) and
    ah_massage_headers with out = 0 (:641).  Returns (status, the packet with
    its first skip bytes massaged, the first skip bytes as they arrived), or
    (status, None, None) for a packet that is dropped.  What ah_input's
    callers guarantee is checked first, with EINVAL: skip as ip_input /
    ip6_input leave it, a header whose own length and version agree with it,
    and struct newah inside the packet."""
    m = bytes(packet_bytes)
    if skip % 4 or (skip != 40 if af6 else not 20 <= skip <= 60) or len(m) < skip + AhSecAssoc.rplen:
        return L.EINVAL, None, None
    if (m[0] >> 4 != 6) if af6 else (m[0] != 0x40 | skip >> 2):
        return L.EINVAL, None, None
    hl = 8 + m[skip + 1] * 4                                         # sizeof(struct ah) + ah_len * 4, :577
    ahsize = ah_hdrsiz(mlen, af6)
    if hl != ahsize:                                                 # :581
        return L.EACCES, None, None
    if skip + ahsize > len(m):                                       # :591
        return L.EACCES, None, None
    saved = m[:skip]
    if af6:
        if m[4:6] == b"\0\0":                                        # :404
            return L.EMSGSIZE, None, None
        hdr = ah_massage_ipv6(m, cleartos)
    else:
        try:
            hdr = ah_massage_ipv4(m, skip, 0, cleartos)
        except ValueError:
            return L.EINVAL, None, None
    return 0, hdr + m[skip:], saved


def ah_input_cb_decap(mode, af6, mlen, packet_bytes, saved, skip):
    """ah_input_cb after the compare and the window update (xform_ah.c:758-814)
    and ipsec4/6_common_input_cb (esp.ipsec_common_input_cb) with one packet
    that ah_input accepted: `packet_bytes` as ah_input left it, `saved` the
    first skip bytes it saved.  mode is saidx.mode (esp.IPSEC_MODE_*).
    Returns (status, resulting packet bytes, bytes key_sa_recordxfer books)."""
    from . import esp as E
    m = bytes(packet_bytes)
    ahsize = ah_hdrsiz(mlen, af6)
    nxt = m[skip]                                                    # ah_nxt, saved at :638
    ptr = bytearray(saved[:skip])
    protoff = 6 if af6 else 9
    ptr[protoff] = nxt                                               # :759
    m = bytes(ptr) + m[skip:]                                        # m_copyback, :762
    m = m[:skip] + m[skip + ahsize:]                                 # m_striphdr, :791
    return E.ipsec_common_input_cb(mode, af6, m, skip, nxt)


def ah_input_host(insa, mlen, buf, length, salt, hsave, at=0):
    """espgpu_ah_input, the engine's host rule, on a bytearray that holds the
    packet at `at`, an L.InSA and a bytearray save slot: returns the status."""
    import ctypes as C
    raw = (C.c_uint8 * (len(buf) - at)).from_buffer(buf, at) if len(buf) > at else None
    hs = (C.c_uint8 * len(hsave)).from_buffer(hsave)
    return L.lib().espgpu_ah_input(C.byref(insa), mlen, C.cast(raw, C.c_void_p), length, salt, C.cast(hs, C.c_void_p))


def ah_decap_host(insa, mlen, buf, length, salt, hsave, at=0):
    """espgpu_ah_decap, the engine's host rule: returns (status, out_off,
    out_len)."""
    import ctypes as C
    raw = (C.c_uint8 * (len(buf) - at)).from_buffer(buf, at)
    hs = (C.c_uint8 * len(hsave)).from_buffer(hsave)
    off, ln = C.c_uint32(0xdddddddd), C.c_uint32(0xdddddddd)
    rc = L.lib().espgpu_ah_decap(C.byref(insa), mlen, C.cast(raw, C.c_void_p), length, salt, C.cast(hs, C.c_void_p),
                                 C.byref(off), C.byref(ln))
    return rc, off.value, ln.value


# ---- the outbound AH stages of the device-resident batch path -------------------
# (include/espgpu.h, the outbound AH block)
#   ipsec_output_encap_ah()  ipsec4/6_perform_request, ipsec_encap, ah_output up
#                            to the AH header's first dword and padding, with
#                            ipsec_process_done's length fields
#                                 ipsec_output.c:221-242, :531-590, :720-770,
#                                 :882-992; xform_ah.c:855-935, :1020-1024
#   ah_output_seq()          ah_output's replay counter   xform_ah.c:928, :937-958, :1045-1048
#   ah_output()              the save and ah_massage_headers with out = 1
#                                 xform_ah.c:988, :1027, :291-422
#   ah_output_cb()           ah_output_cb's m_copyback    xform_ah.c:1120
def ipsec_output_encap_ah(tunnel, saf6, src, dst, ttl, dfbit, ecn, rfc6864, mlen, packet, headroom, ip_id):
    """What the stack does with a cleartext packet between ip_output and
    ah_output's replay counter: the transport-or-tunnel decision and
    ipsec_encap as esp.ipsec_output_encap restates them, then ah_output's size
    check (xform_ah.c:882), m_makespace (:907), the AH header's first dword
    (:925-927), the zeroed padding (:934) and the protocol field (:1020-1024),
    with ipsec_process_done's length fields and ip_output's checksum in the IP
    header in front of it.  Arguments as esp.ipsec_output_encap, mlen the ICV
    length.  Returns (status, front, wire, hs, nxt): the wire packet starts
    front bytes before where the cleartext packet started, `wire` holds it
    with None for every byte the step leaves to others (SPI, sequence number,
    ICV field), hs is the length of the IP header in front of the AH header
    and nxt is ah_nxt.  (status, 0, None, 0, 0) for a packet that is dropped.
    The lengths come from len(packet) (the reference adds ahsize to the field
    as it stands, :1001, :1012); a packet longer than 65535 bytes is EMSGSIZE
    and link-local SA addresses are ENOTSUP, as for ESP."""
    from . import esp as E
    m = bytes(packet)
    src, dst = bytes(src), bytes(dst)
    alen_a = 16 if saf6 else 4
    drop = lambda st: (st, 0, None, 0, 0)                            # noqa: E731
    if mlen % 4 or not 4 <= mlen <= 64:
        return drop(L.EINVAL)
    if saf6:
        if not any(src[:16]) or not any(dst[:16]):                   # ipsec_output.c:961-964
            return drop(L.EINVAL)
        if any(a[0] == 0xfe and a[1] & 0xc0 == 0x80 for a in (src, dst)):
            return drop(L.ENOTSUP)
    if len(m) < 20:
        return drop(L.EINVAL)
    v = m[0] >> 4
    if v == 4:
        skip = (m[0] & 0xf) << 2
        if skip < 20 or skip > len(m):
            return drop(L.EINVAL)
        protoff, pdst = 9, m[16:20]
    elif v == 6:
        if len(m) < 40:
            return drop(L.EINVAL)
        skip, protoff, pdst = 40, 6, m[24:40]                        # :574-581
    else:
        return drop(L.EAFNOSUPPORT)                                  # :932-933
    if len(m) > E.IP_MAXPACKET:
        return drop(L.EMSGSIZE)
    encap = (tunnel or saf6 != (v == 6) or                           # :224-228, :543-547
             (any(dst[:alen_a]) and dst[:alen_a] != pdst))
    if encap and not saf6 and (not any(src[:4]) or not any(dst[:4])):    # :938-941
        return drop(L.EINVAL)
    ahsize = ah_hdrsiz(mlen, saf6)
    oh = (40 if saf6 else 20) if encap else 0
    total = len(m) + ahsize + oh
    if total > E.IP_MAXPACKET:                                       # xform_ah.c:882
        return drop(L.EMSGSIZE)
    if ahsize + oh > headroom:                                       # ipsec_prepend, m_makespace (:907)
        return drop(L.ENOBUFS)
    m = bytearray(m)
    if encap:
        if v == 4:
            setdf = dfbit if dfbit in (0, 1) else int(m[6] & 0x40 != 0)          # :910-917
            itos, proto = m[1], E.IPPROTO_IPIP
            m[2:4] = struct.pack(">H", len(m))                       # :230
            m[10:12] = b"\0\0"                                       # :231
            m[10:12] = struct.pack(">H", E.in_cksum(bytes(m[:skip])))    # :232
        else:
            m[4:6] = struct.pack(">H", len(m) - 40)                  # :533
            itos, proto = (struct.unpack(">I", m[:4])[0] >> 20) & 0xff, E.IPPROTO_IPV6   # :925
            setdf = 1 if dfbit else 0                                # :926
        if not saf6:                                                 # :942-956
            ip_off = E.IP_DF if setdf else 0
            idv = 0 if rfc6864 and ip_off & E.IP_DF else ip_id & 0xffff          # ip_id.c:252
            outer = bytearray(struct.pack(">BBHHHBBH4s4s", 0x45, E.ip_ecn_ingress(ecn, itos), len(m) + 20, idv,
                                          ip_off, ttl, proto, 0, src[:4], dst[:4]))
        else:                                                        # :965-984
            outer = bytearray(struct.pack(">IHBB16s16s", 0x60000000 | E.ip_ecn_ingress(ecn, itos) << 20,
                                          len(m), proto, ttl, src[:16], dst[:16]))
        m = outer + m
        skip, protoff = (40, 6) if saf6 else (20, 9)                 # :568-582, :244-260
    nxt = m[protoff]                                                 # xform_ah.c:925
    ah = [nxt, (ahsize - 8) // 4, 0, 0] + [None] * 8 + [None] * mlen + [0] * (ahsize - 12 - mlen)   # :925-934
    wire = list(m[:skip]) + ah + list(m[skip:])                      # m_makespace(m, skip, ahsize), :907
    wire[protoff] = IPPROTO_AH                                       # :1020-1024
    assert len(wire) == total
    if saf6:                                                         # ipsec_process_done, :742
        wire[4:6] = list(struct.pack(">H", total - 40))
    else:
        wire[2:4] = list(struct.pack(">H", total))                   # :727
        wire[10:12] = [0, 0]
        wire[10:12] = list(struct.pack(">H", E.in_cksum(bytes(wire[:skip]))))    # ip_output.c:780-782
    return 0, oh + ahsize, wire, skip, nxt


def ah_output(saf6, wire, hs, cleartos=True):
    """ah_output's save (xform_ah.c:988) and ah_massage_headers with out = 1
    (:1027) on what ipsec_output_encap_ah returned.  Returns (status, the
    packet with its first hs bytes massaged, the first hs bytes in wire form),
    (EINVAL, None, None) where the option loop refuses.  A source-route option
    shorter than 4 bytes is refused too: the engine's deliberate difference."""
    saved = bytes(wire[:hs])
    if saf6:
        hdr = ah_massage_ipv6(saved, cleartos)                       # ip6_plen != 0: it holds ahsize at least
    else:
        try:
            hdr = ah_massage_ipv4(saved, hs, 1, cleartos)
        except ValueError:
            return L.EINVAL, None, None
        off = 20
        while off < hs and saved[off] != IPOPT_EOL:                  # the loop accepted these options
            if saved[off] == IPOPT_NOP:
                off += 1
                continue
            if saved[off] in (IPOPT_LSRR, IPOPT_SSRR) and saved[off + 1] < 4:
                return L.EINVAL, None, None
            off += saved[off + 1]
    return 0, list(hdr) + list(wire[hs:]), saved


def ah_output_seq(state, spi, packet, salt):
    """ah_output's replay counter (xform_ah.c:937-958) and SPI (:928) for the
    packet whose ICV field is at `salt`, and crp_esn (:1045-1048): `state` is
    an esp.OutState (count, flags as L.OUT_* bits; ah_output checks the wrap
    whatever OUT_WRAPCHECK says).  Returns (status, packet, esn_hi, advanced
    state); (EACCES, None, None, state) at the end of the number space."""
    st, f = state.copy(), state.flags
    if not f & L.OUT_CYCSEQ and (st.count == 2**64 - 1 or
                                 (not f & L.OUT_ESN and st.count & 0xffffffff == 0xffffffff)):   # :940-943
        return L.EACCES, None, None, state
    st.count = (st.count + 1) & (2**64 - 1)                          # :956
    out = list(packet)
    out[salt - 8:salt] = list(struct.pack(">II", spi, st.count & 0xffffffff))    # :928, :957
    return 0, out, (st.count >> 32 if f & L.OUT_ESN else 0), st


def ah_output_cb(packet, saved):
    """ah_output_cb's m_copyback (xform_ah.c:1120): the saved header, in wire
    form, back over the massaged one."""
    return list(saved) + list(packet[len(saved):])


def ah_encap_host(encsa, mlen, buf, at, length, headroom, ip_id, hsave):
    """espgpu_ah_encap, the engine's host rule, on a bytearray that holds the
    cleartext packet at `at`, an L.EncSA and a bytearray save slot: returns
    (status, front, total, salt)."""
    import ctypes as C
    raw = (C.c_uint8 * (len(buf) - at)).from_buffer(buf, at) if len(buf) > at else None
    hs = (C.c_uint8 * len(hsave)).from_buffer(hsave)
    res = [C.c_uint32(0xdddddddd) for _ in range(3)]
    rc = L.lib().espgpu_ah_encap(C.byref(encsa), mlen, C.cast(raw, C.c_void_p) if raw else None, length, headroom,
                                 ip_id & 0xffff, C.cast(hs, C.c_void_p), *[C.byref(r) for r in res])
    return (rc,) + tuple(r.value for r in res)


def ah_frame_host(outsa, buf, at, length, salt, esn_hi=0):
    """espgpu_ah_frame, the engine's host rule, on a bytearray that holds the
    wire packet at `at` and an L.OutSA: returns (status, esn_hi), esn_hi as
    passed in when refused."""
    import ctypes as C
    raw = (C.c_uint8 * (len(buf) - at)).from_buffer(buf, at)
    hi = C.c_uint32(esn_hi)
    rc = L.lib().espgpu_ah_frame(C.byref(outsa), C.cast(raw, C.c_void_p), length, salt, C.byref(hi))
    return rc, hi.value


def ah_sent_host(encsa, status, buf, at, length, salt, hsave):
    """espgpu_ah_sent, the engine's host rule: the restore on the bytearray
    that holds the wire packet at `at` and the booking on the L.EncSA."""
    import ctypes as C
    raw = (C.c_uint8 * (len(buf) - at)).from_buffer(buf, at)
    hs = (C.c_uint8 * len(hsave)).from_buffer(hsave)
    return L.lib().espgpu_ah_sent(C.byref(encsa), status, C.cast(raw, C.c_void_p), length, salt,
                                  C.cast(hs, C.c_void_p))
