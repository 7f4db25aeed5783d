"""ESP request builders, the caller side of the hot path (unchanged semantics).

  esp_csp()           esp_init           freebsd/netipsec/xform_esp.c:143-244
  esp_input_crp()     esp_input          xform_esp.c:260-463
  esp_output_crp()    esp_output         xform_esp.c:673-961 (padding :710-716, :810-843)
  esp_trailer_ok()    esp_input_cb tail  xform_esp.c:597-636
  ipsec_output_encap() ipsec4/6_perform_request, ipsec_encap  ipsec_output.c:221-242, :531-590, :882-992
Records are IPv4 packets with the ESP header at `skip` (tunnel mode: skip = IP
header length), in a bytearray (or an mbuf-like list of bytearrays).
"""
import struct

from . import _lib as L
from .opencrypto import crypto_session_params

GCM, CBC_SHA1 = "aes-gcm-16", "aes-cbc-hmac-sha1-96"
CBC_SHA256, CBC_SHA384, CBC_SHA512 = ("aes-cbc-hmac-sha2-256-128", "aes-cbc-hmac-sha2-384-192",
                                      "aes-cbc-hmac-sha2-512-256")
CTR_SHA1, CTR_SHA256 = "aes-ctr-hmac-sha1-96", "aes-ctr-hmac-sha2-256-128"   # RFC 3686
CTR_SHA384, CTR_SHA512 = "aes-ctr-hmac-sha2-384-192", "aes-ctr-hmac-sha2-512-256"
# ESP-NULL (SADB_EALG_NULL, key.c:588; RFC 2410) with HMAC: encrypt-then-MAC
# sessions whose cipher is CRYPTO_NULL_CBC (no key, no IV, blocksize 4)
NULL_SHA1, NULL_SHA256 = "null-hmac-sha1-96", "null-hmac-sha2-256-128"
NULL_SHA384, NULL_SHA512 = "null-hmac-sha2-384-192", "null-hmac-sha2-512-256"
# encryption without authentication (esp_init's CSP_MODE_CIPHER, xform_esp.c:230-231)
CBC, CTR = "aes-cbc", "aes-ctr"
# auth algorithm and ICV bytes (xform_ah_authsize, xform_ah.c:117-131: 12 for
# SHA1-96, hashsize/2 for SHA2 per RFC 4868)
_AUTH = {CBC_SHA1: (L.CRYPTO_SHA1_HMAC, 12), CTR_SHA1: (L.CRYPTO_SHA1_HMAC, 12),
         CBC_SHA256: (L.CRYPTO_SHA2_256_HMAC, 16), CTR_SHA256: (L.CRYPTO_SHA2_256_HMAC, 16),
         CBC_SHA384: (L.CRYPTO_SHA2_384_HMAC, 24), CTR_SHA384: (L.CRYPTO_SHA2_384_HMAC, 24),
         CBC_SHA512: (L.CRYPTO_SHA2_512_HMAC, 32), CTR_SHA512: (L.CRYPTO_SHA2_512_HMAC, 32),
         NULL_SHA1: (L.CRYPTO_SHA1_HMAC, 12), NULL_SHA256: (L.CRYPTO_SHA2_256_HMAC, 16),
         NULL_SHA384: (L.CRYPTO_SHA2_384_HMAC, 24), NULL_SHA512: (L.CRYPTO_SHA2_512_HMAC, 32)}
_CTR_ALGS = (CTR_SHA1, CTR_SHA256, CTR_SHA384, CTR_SHA512, CTR)
_NULL_ALGS = (NULL_SHA1, NULL_SHA256, NULL_SHA384, NULL_SHA512)
ETA_ALGS = tuple(_AUTH)
CIPHER_ALGS = (CBC, CTR)
IPPROTO_NONE = 59


class SecAssoc:
    """What key_setsaval leaves in struct secasvar for the two ESP transforms."""

    def __init__(self, spi, alg, key, auth_key=b"", esn=False, mlen=None):
        self.spi = spi
        self.alg = alg
        self.key = bytes(key)          # GCM: cipher key || 4-byte salt (RFC 4106 8.1)
        self.auth_key = bytes(auth_key)
        self.esn = esn
        # ICV bytes: xform_ah_authsize (GMAC 16, SHA1-HMAC 12, SHA2-HMAC
        # hashsize/2); a GCM SA may carry a truncated 12- or 8-byte ICV
        # (RFC 4106 s3.3, csp_auth_mlen)
        self.mlen = mlen if mlen is not None else (
            16 if alg == GCM else _AUTH[alg][1] if alg in _AUTH else 0)

    @property
    def ctr(self):
        return self.alg in _CTR_ALGS

    @property
    def null(self):
        return self.alg in _NULL_ALGS

    @property
    def auth(self):
        """An ICV to verify / compute (every transform but the CIPHER ones)."""
        return self.alg == GCM or self.alg in _AUTH

    @property
    def cipher_alg(self):
        return L.CRYPTO_AES_ICM if self.ctr else L.CRYPTO_NULL_CBC if self.null else L.CRYPTO_AES_CBC

    @property
    def auth_alg(self):
        return _AUTH[self.alg][0] if self.alg in _AUTH else 0

    @property
    def ivlen(self):
        # RFC 4106 / 3686: 8-byte IV; enc_xform_null: none; CBC: 16
        return 8 if self.alg == GCM or self.ctr else 0 if self.null else 16

    @property
    def hlen(self):
        return 8 + self.ivlen           # struct newesp + IV

    @property
    def alen(self):
        return self.mlen

    @property
    def blocksize(self):
        # enc_xform blocksize (ESP pads to 4 anyway): GCM / CTR 1, NULL 4, CBC 16
        return 1 if self.alg == GCM or self.ctr else 4 if self.null else 16

    @property
    def salt(self):
        # the 4-byte salt / nonce esp_init strips off the key (RFC 4106 8.1, RFC 3686 5.1)
        return self.key[-4:] if self.alg == GCM or self.ctr else b"\0\0\0\0"

    def csp(self):
        if self.alg == GCM:
            return crypto_session_params(
                csp_mode=L.CSP_MODE_AEAD,
                csp_flags=L.CSP_F_SEPARATE_AAD if self.esn else 0,
                csp_ivlen=12, csp_cipher_alg=L.CRYPTO_AES_NIST_GCM_16,
                csp_cipher_klen=len(self.key) - 4, csp_cipher_key=self.key[:-4],
                csp_auth_mlen=0 if self.mlen == 16 else self.mlen)
        ckey = self.key[:-4] if self.ctr else b"" if self.null else self.key
        ivsize = 0 if self.null else 16                      # csp_ivlen = txform->ivsize (:240)
        if not self.auth:                                     # esp_init :230-231
            return crypto_session_params(
                csp_mode=L.CSP_MODE_CIPHER, csp_ivlen=ivsize, csp_cipher_alg=self.cipher_alg,
                csp_cipher_klen=len(ckey), csp_cipher_key=ckey)
        return crypto_session_params(
            csp_mode=L.CSP_MODE_ETA, csp_flags=L.CSP_F_ESN if self.esn else 0,
            csp_ivlen=ivsize, csp_cipher_alg=self.cipher_alg, csp_cipher_klen=len(ckey),
            csp_cipher_key=ckey if ckey else None, csp_auth_alg=self.auth_alg,
            csp_auth_klen=len(self.auth_key), csp_auth_key=self.auth_key, csp_auth_mlen=self.mlen)


def _flat(buf):
    return bytes(buf) if not isinstance(buf, list) else b"".join(bytes(b) for b in buf)


def esp_input_crp(fw, ses, sa, pkt, skip, esn_hi=0):
    """Build the decrypt+verify cryptop exactly as esp_input does."""
    total = len(_flat(pkt))
    crp = fw.crypto_getreq(ses)
    seqh = struct.pack(">I", esn_hi)
    data = _flat(pkt)
    if sa.auth:                                                               # :364-405
        crp.crp_op = L.CRYPTO_OP_VERIFY_DIGEST
        crp.crp_aad_length = 8 if sa.alg == GCM else sa.hlen                  # :366-369
        if sa.alg == GCM and sa.esn:                                          # :372-397
            crp.crp_aad = data[skip:skip + 4] + seqh + data[skip + 4:skip + 8]
            crp.crp_aad_length = 12
        else:
            crp.crp_aad_start = skip
        if sa.alg != GCM and sa.esn:
            crp.crp_esn = seqh                                                # :400-402
        crp.crp_digest_start = total - sa.alen                                # :404
    crp.crp_op |= L.CRYPTO_OP_DECRYPT                                         # :420
    crp.crp_flags = L.CRYPTO_F_CBIFSYNC
    crp.crp_buf = pkt
    crp.crp_payload_start = skip + sa.hlen                                    # :424-425
    crp.crp_payload_length = total - (skip + sa.hlen + sa.alen)
    if sa.alg == GCM or sa.ctr:                                               # :430-458
        ctr0 = struct.pack(">I", 1) if sa.ctr else b"\0" * 4
        crp.crp_iv = bytearray(sa.salt + data[skip + sa.hlen - sa.ivlen:skip + sa.hlen] + ctr0)
        crp.crp_flags |= L.CRYPTO_F_IV_SEPARATE
    elif sa.ivlen:
        crp.crp_iv_start = skip + sa.hlen - sa.ivlen
    return crp


def esp_output_crp(fw, ses, sa, pkt, skip, esn_hi=0):
    """The encrypt cryptop esp_output builds over an already padded packet."""
    total = len(_flat(pkt))
    data = _flat(pkt)
    crp = fw.crypto_getreq(ses)
    crp.crp_op = L.CRYPTO_OP_ENCRYPT | (L.CRYPTO_OP_COMPUTE_DIGEST if sa.auth else 0)
    crp.crp_flags = L.CRYPTO_F_CBIFSYNC
    crp.crp_buf = pkt
    crp.crp_payload_start = skip + sa.hlen
    crp.crp_payload_length = total - (skip + sa.hlen + sa.alen)
    seqh = struct.pack(">I", esn_hi)
    if not sa.auth:                                                   # :862-887, no esph
        if sa.ctr:
            crp.crp_iv = bytearray(sa.salt + data[skip + 8:skip + 16] + struct.pack(">I", 1))
            crp.crp_flags |= L.CRYPTO_F_IV_SEPARATE
        elif sa.ivlen:
            crp.crp_iv_start = skip + 8
        return crp
    crp.crp_digest_start = total - sa.alen
    if sa.alg == GCM:
        if sa.esn:
            crp.crp_aad = data[skip:skip + 4] + seqh + data[skip + 4:skip + 8]
            crp.crp_aad_length = 12
        else:
            crp.crp_aad_start = skip
            crp.crp_aad_length = 8
        crp.crp_iv = bytearray(sa.salt + data[skip + 8:skip + 16] + b"\0" * 4)
        crp.crp_flags |= L.CRYPTO_F_IV_SEPARATE
    else:
        crp.crp_aad_start = skip
        crp.crp_aad_length = sa.hlen
        if sa.ctr:
            crp.crp_iv = bytearray(sa.salt + data[skip + 8:skip + 16] + struct.pack(">I", 1))
            crp.crp_flags |= L.CRYPTO_F_IV_SEPARATE
        elif sa.ivlen:
            crp.crp_iv_start = skip + 8
        if sa.esn:
            crp.crp_esn = seqh
    return crp


def esp_pad(inner, blocksize=4, next_header=4):
    """Self-describing padding 1,2,3,... + pad length + next header (xform_esp.c:810-843)."""
    rlen = len(inner)
    padding = ((blocksize - ((rlen + 2) % blocksize)) % blocksize) + 2
    pad = bytes(range(1, padding - 1)) + bytes([padding - 2, next_header])
    return bytes(inner) + pad


class OutState:
    """The outbound part of struct secasvar that esp_output advances under the
    SA lock: replay->count, cntr, and the SA's flags as L.OUT_* bits."""

    def __init__(self, count=0, cntr=0, flags=0):
        self.count, self.cntr, self.flags = count, cntr, flags

    def copy(self):
        return OutState(self.count, self.cntr, self.flags)


def esp_out_blks(sa, flags=0):
    """blks = MAX(4, blocksize), native_blocksize (16) for an AES-CTR SA under
    V_esp_ctr_compatibility (xform_esp.c:710-713)."""
    return 16 if sa.ctr and flags & L.OUT_CTRCOMPAT else max(4, sa.blocksize)


def esp_output_frame(sa_state, sa, payload, next_header, fill=0):
    """esp_output between m_makespace and crypto_dispatch (xform_esp.c:700-716,
    782-843, 867-887): returns (record, esn_hi, advanced state).  The record
    is SPI | sequence number | IV | payload | padding | pad length | next
    header | ICV field; what esp_output leaves to others -- a CBC SA's IV
    (arc4rand), the pad bytes without PAD_SEQ / PAD_ZERO, the ICV field -- is
    `fill`.  With OUT_WRAPCHECK the end of the number space is ah_output's
    (xform_ah.c:940-950): (None, None, sa_state unchanged)."""
    st, f = sa_state.copy(), sa_state.flags
    rlen = len(payload)
    blks = esp_out_blks(sa, f)
    padding = ((blks - ((rlen + 2) % blks)) % blks) + 2                        # :716
    if f & L.OUT_WRAPCHECK and not f & L.OUT_CYCSEQ and (
            st.count == 2**64 - 1 or (not f & L.OUT_ESN and st.count & 0xffffffff == 0xffffffff)):
        return None, None, sa_state
    st.count = (st.count + 1) & (2**64 - 1)                                    # :793
    esn_hi = st.count >> 32 if f & L.OUT_ESN else 0                            # :799
    hdr = struct.pack(">II", sa.spi, st.count & 0xffffffff)                    # :783-797
    if sa.alg == GCM or sa.ctr:                                                # :802-803, :869-881
        iv = struct.pack(">Q", st.cntr)
        st.cntr = (st.cntr + 1) & (2**64 - 1)
    else:
        iv = bytes([fill]) * sa.ivlen                                          # :884, the caller's
    if f & L.OUT_PAD_SEQ:                                                      # :824-835
        pad = bytes(range(1, padding - 1))
    elif f & L.OUT_PAD_ZERO:
        pad = bytes(padding - 2)
    else:
        pad = bytes([fill]) * (padding - 2)
    pad += bytes([padding - 2, next_header])                                   # :838-839
    return hdr + iv + bytes(payload) + pad + bytes([fill]) * sa.alen, esn_hi, st


def esp_frame_shape(sa, flags=0):
    """espgpu_esp_frame_shape for the SA's session parameters: an L.EShape."""
    import ctypes as C
    p, _keep = sa.csp()._c()
    shape = L.EShape()
    rc = L.lib().espgpu_esp_frame_shape(C.byref(p), flags, C.byref(shape))
    if rc:
        raise ValueError("espgpu_esp_frame_shape: %d" % rc)
    return shape


def esp_frame_host(outsa, shape, rec, rlen, next_header, esn_hi=0):
    """espgpu_esp_frame, the engine's host rule, on a bytearray record and an
    L.OutSA: returns (status, esn_hi), esn_hi as passed in when refused."""
    import ctypes as C
    buf = (C.c_uint8 * max(len(rec), 1)).from_buffer(rec) if len(rec) else None
    hi = C.c_uint32(esn_hi)
    rc = L.lib().espgpu_esp_frame(C.byref(outsa), C.byref(shape), C.cast(buf, C.c_void_p) if buf else None,
                                  len(rec), rlen, next_header, C.byref(hi))
    return rc, hi.value


IPPROTO_ESP, IPPROTO_AH = 50, 51
IP_MF, IP_OFFMASK = 0x2000, 0x1fff


def in_cksum(data):
    """The Internet checksum of `data` (in_cksum): 0 for a header whose
    checksum field is right."""
    s = sum(struct.unpack(">%dH" % (len(data) // 2), bytes(data)))
    while s >> 16:
        s = (s & 0xffff) + (s >> 16)
    return ~s & 0xffff


def ipsec_input_classify(sadb, pkt, off4=0, ipcsum=False):
    """What the stack does with a received packet up to esp_input's first
    lines, for the packets the device path takes: ip_input's header checks
    (ip_input.c:488-561, :807), ipsec_common_input's length check, SPI and
    destination (ipsec_input.c:141-208), key_allocsa (key.c:1091-1133) and
    esp_input's alignment check (xform_esp.c:279-284); ip6_input /
    ipsec6_input for IPv6.  sadb maps an SPI to (sa, proto, af, dst bytes,
    salt): one SPI namespace for all protocols.  Returns (status, (off4, len,
    sa, esn_hi, salt)), the descriptor of the ESP record on status 0 and
    (off4, 0, 0xffff, 0, 0) otherwise.  ENOTSUP marks the packets that go on
    in the host stack: fragments (ip_reass), other protocols, IPv6 jumbograms
    and link-local destinations."""
    pkt = bytes(pkt)
    n = len(pkt)

    def drop(status):
        return status, (off4, 0, 0xffff, 0, 0)

    if n < 20:                                                       # m_pullup, ips_toosmall
        return drop(L.EINVAL)
    v = pkt[0] >> 4
    if v == 4:
        hlen = (pkt[0] & 0xf) << 2
        if hlen < 20 or hlen > n:                                    # ips_badhlen
            return drop(L.EINVAL)
        if ipcsum and in_cksum(pkt[:hlen]) != 0:                     # ips_badsum
            return drop(L.EINVAL)
        ip_len, ip_off = struct.unpack(">H", pkt[2:4])[0], struct.unpack(">H", pkt[6:8])[0]
        if ip_len < hlen or n < ip_len:                              # ips_badlen, ips_tooshort
            return drop(L.EINVAL)
        pkt = pkt[:ip_len]                                           # the trim, :555-561
        if ip_off & (IP_MF | IP_OFFMASK):                            # ip_reass: the host's
            return drop(L.ENOTSUP)
        if pkt[9] != IPPROTO_ESP:
            return drop(L.ENOTSUP)
        af, skip, dst = 4, hlen, pkt[16:20]
    elif v == 6:
        if n < 40:
            return drop(L.EINVAL)
        plen = struct.unpack(">H", pkt[4:6])[0]
        if plen == 0:                                                # jumbo payload option
            return drop(L.ENOTSUP)
        if n - 40 < plen:                                            # ip6s_tooshort
            return drop(L.EINVAL)
        pkt = pkt[:40 + plen]
        if pkt[6] != IPPROTO_ESP:                                    # extension headers: the host's
            return drop(L.ENOTSUP)
        af, skip, dst = 6, 40, pkt[24:40]
        if dst[0] == 0xfe and dst[1] & 0xc0 == 0x80:                 # IN6_IS_SCOPE_LINKLOCAL
            return drop(L.ENOTSUP)
    else:                                                            # ips_badvers
        return drop(L.EINVAL)
    if len(pkt) - skip < 8:                                          # ipsec_input.c:141
        return drop(L.EINVAL)
    if skip % 4 or len(pkt) % 4:                                     # xform_esp.c:279
        return drop(L.EINVAL)
    spi = struct.unpack(">I", pkt[skip:skip + 4])[0]
    sav = sadb.get(spi) if spi else None                             # SAVHASH_HASH(spi)
    if sav is None:
        return drop(L.ENOENT)                                        # notdb
    sa, proto, saf, sdst, salt = sav
    if proto != IPPROTO_ESP or saf != af or bytes(sdst)[:len(dst)] != dst:   # key.c:1110-1118
        return drop(L.ENOENT)
    return 0, (off4 + skip // 4, len(pkt) - skip, sa, 0, salt)


def esp_classify_host(table, pkt, off4=0, flags=0):
    """espgpu_esp_classify, the engine's host rule, on a SAD_DTYPE table
    (batch.sad_build) and a packet's bytes: (status, (off4, len, sa, esn_hi,
    salt))."""
    import ctypes as C
    pkt = bytes(pkt)
    d = L.Desc(0xdddddddd, 0xdddd, 0xdddd, 0xdddddddd, 0xdddddddd)
    rc = L.lib().espgpu_esp_classify(table.ctypes.data, len(table), pkt, len(pkt), off4, flags, C.byref(d))
    return rc, (d.off4, d.len, d.sa, d.esn_hi, d.salt)


IPSEC_MODE_ANY, IPSEC_MODE_TRANSPORT, IPSEC_MODE_TUNNEL = 0, 1, 2    # netipsec/ipsec.h
IPPROTO_IPIP, IPPROTO_IPV6 = 4, 41


def esp_input_decap(mode, af6, prand, ivlen, alen, packet_bytes, skip):
    """What esp_input_cb does after the window update (xform_esp.c:581-648)
    and ipsec4_common_input_cb / ipsec6_common_input_cb up to netisr_queue
    (ipsec_input.c:298-417, :531-638) with one packet, on bytes: the outer IP
    header of `skip` bytes and the decrypted ESP record behind it.  mode is
    saidx.mode, af6 whether saidx.dst is AF_INET6, prand SADB_X_EXT_PRAND.
    Returns (status, resulting packet bytes, bytes key_sa_recordxfer books),
    (status, None, 0) for a packet that is dropped.  What the callers of these
    functions guarantee is checked first, with EINVAL: skip as ip_input /
    ip6_input leave it, at least the two trailer bytes of payload, and in
    transport mode a header whose own length and version agree with skip."""
    m = bytes(packet_bytes)
    hlen = 8 + ivlen                                                 # sizeof(struct newesp) + ivlen, :585
    if skip % 4 or (skip != 40 if af6 else not 20 <= skip <= 60):
        return L.EINVAL, None, 0
    if len(m) - skip - hlen - alen < 2:
        return L.EINVAL, None, 0
    m = m[:len(m) - alen]                                            # m_adj(m, -alen), :548
    m = m[:skip] + m[skip + hlen:]                                   # m_striphdr(m, skip, hlen), :588
    lastthree = m[len(m) - 3:]                                       # :598
    if lastthree[1] + 2 > len(m) - skip:                             # :601
        return L.EINVAL, None, 0
    if not prand and lastthree[1] != lastthree[0] and lastthree[1] != 0:   # :613-614
        return L.EINVAL, None, 0
    if lastthree[2] == IPPROTO_NONE:                                 # :629
        return L.ENODATA, None, 0
    m = m[:len(m) - (lastthree[1] + 2)]                              # m_adj, :633
    protoff = 6 if af6 else 9                                        # ip6_nxt / ip_p
    m = m[:protoff] + lastthree[2:3] + m[protoff + 1:]               # m_copyback, :636
    return ipsec_common_input_cb(mode, af6, m, skip, lastthree[2])


def ipsec_common_input_cb(mode, af6, m, skip, prot):
    """ipsec4_common_input_cb / ipsec6_common_input_cb up to netisr_queue
    (ipsec_input.c:298-417, :531-638) on the packet `m` as the transform's
    callback hands it over: the outer header of `skip` bytes with its protocol
    field already `prot`, and the payload behind it.  Shared by esp_input_decap
    and ah.ah_input_cb_decap.  Returns (status, resulting packet bytes, bytes
    key_sa_recordxfer books)."""
    if not af6:                                                      # ipsec4_common_input_cb
        ip = bytearray(m[:skip])
        ip[2:4] = struct.pack(">H", len(m) & 0xffff)                 # ip_len, :312
        ip[10:12] = b"\0\0"                                          # :313
        ip[10:12] = struct.pack(">H", in_cksum(bytes(ip)))           # :314
        fixed = bytes(ip) + m[skip:]
        if prot == IPPROTO_IPIP and mode != IPSEC_MODE_TRANSPORT:    # :334-343
            if len(m) - skip < 20:
                return L.EINVAL, None, 0
            fixed = fixed[skip:]                                     # m_striphdr(m, 0, ip_hl << 2)
        elif prot == IPPROTO_IPV6 and mode != IPSEC_MODE_TRANSPORT:  # :346-355
            if len(m) - skip < 40:
                return L.EINVAL, None, 0
            fixed = fixed[skip:]
        else:
            if prot != IPPROTO_IPV6 and mode == IPSEC_MODE_ANY:      # :357-365
                prot = IPPROTO_IPIP
            if mode == IPSEC_MODE_TRANSPORT:                         # :395-396
                prot = IPPROTO_IPIP
            if prot != IPPROTO_IPIP:                                 # :400-417
                return L.EPFNOSUPPORT, None, 0
            if m[0] != 0x40 | skip >> 2:                             # ip_input's, for the header in_cksum read
                return L.EINVAL, None, 0
        return 0, fixed, len(fixed)                                  # key_sa_recordxfer, :389
    ip6 = bytearray(m[:40])                                          # ipsec6_common_input_cb
    ip6[4:6] = struct.pack(">H", (len(m) - 40) & 0xffff)             # ip6_plen, :532
    fixed = bytes(ip6) + m[40:]
    if prot == IPPROTO_IPV6 and mode != IPSEC_MODE_TRANSPORT:        # :539-549
        if len(m) - skip < 40:
            return L.EINVAL, None, 0
        fixed = fixed[skip:]
    elif prot == IPPROTO_IPIP and mode != IPSEC_MODE_TRANSPORT:      # :552-562
        if len(m) - skip < 20:
            return L.EINVAL, None, 0
        fixed = fixed[skip:]
    elif m[0] >> 4 != 6:                                             # ip6_input's
        return L.EINVAL, None, 0
    return 0, fixed, len(fixed)                                      # :590; the protocol loop goes on in place


def esp_decap_host(insa, shape, buf, skip, rlen, trailer, at=0):
    """espgpu_esp_decap, the engine's host rule, on a bytearray that holds the
    outer header at `at` and the decrypted record behind it, and an L.InSA:
    returns (status, out_off, out_len)."""
    import ctypes as C
    raw = (C.c_uint8 * (len(buf) - at)).from_buffer(buf, at)
    off, ln = C.c_uint32(0xdddddddd), C.c_uint32(0xdddddddd)
    rc = L.lib().espgpu_esp_decap(C.byref(insa), C.byref(shape), C.cast(raw, C.c_void_p), skip, rlen, trailer,
                                  C.byref(off), C.byref(ln))
    return rc, off.value, ln.value


IP_DF, IP_MAXPACKET = 0x4000, 65535
ECN_ALLOWED, ECN_FORBIDDEN, ECN_NOCARE = 1, 0, -1                    # netinet/ip_ecn.h


def ip_ecn_ingress(mode, inner):
    """The outer TOS / traffic class for an inner one (ip_ecn.c:97-122)."""
    outer = inner
    if mode == ECN_ALLOWED:
        if inner & 3 == 3:                                           # CE inside: ECT(0) outside
            outer &= ~1
    elif mode == ECN_FORBIDDEN:
        outer &= ~3
    return outer & 0xff


def ipsec_output_encap(tunnel, saf6, src, dst, ttl, dfbit, ecn, rfc6864, ivlen, blks, alen, packet, headroom,
                       tailroom, ip_id):
    """What the stack does with a cleartext packet between ip_output and
    crypto_dispatch and after crypto_done, except the bytes esp_output_frame
    covers: ipsec4_perform_request / ipsec6_perform_request
    (ipsec_output.c:221-242, :531-590), ipsec_encap (:882-992) with
    ip_ecn_ingress and ip_fillid's RFC 6864 rule (ip_id.c:252), esp_output's
    size check, m_makespace, m_pad and protocol field (xform_esp.c:703-718,
    :747, :772, :810, :839-843) and ipsec_process_done's length fields
    (:722-745), with ip_output's checksum of a tunnel's outer IPv4 header
    (ip_output.c:780-782) and a recomputed one for a transport header.  tunnel
    is sp->req[idx]->saidx.mode == IPSEC_MODE_TUNNEL; saf6, src, dst describe
    saidx (4 or 16 address bytes); ttl is V_ip_defttl / V_ip6_defhlim, dfbit
    V_ip4_ipsec_dfbit (0, 1, 2), ecn V_ip4_ipsec_ecn / V_ip6_ipsec_ecn (-1, 0,
    1), rfc6864 V_ip_rfc6864; ivlen, blks, alen are esp_output's; headroom and
    tailroom stand for what m_makespace / ipsec_prepend and m_pad can get.
    Returns (status, front, wire, nxt): the wire packet starts front bytes
    before where the cleartext packet started, and `wire` holds it with None
    for every byte the step leaves to framing and encryption (ESP header, IV,
    padding, trailer, ICV); nxt is the byte m_copydata puts into the trailer.
    (status, 0, None, 0) for a packet that is dropped.  A packet longer than
    65535 bytes is EMSGSIZE for both families (the reference: ENXIO for IPv6,
    :548-552, no check for IPv4), and link-local SA addresses are ENOTSUP:
    their scope embedding (:975-981) needs the host's zone ids."""
    m = bytes(packet)
    src, dst = bytes(src), bytes(dst)
    alen_a = 16 if saf6 else 4
    hlen = 8 + ivlen
    drop = lambda st: (st, 0, None, 0)                               # noqa: E731
    if saf6:
        if not any(src[:16]) or not any(dst[:16]):                   # :961-964
            return drop(L.EINVAL)
        if any(a[0] == 0xfe and a[1] & 0xc0 == 0x80 for a in (src, dst)):
            return drop(L.ENOTSUP)
    if len(m) < 20:                                                  # ip_output's own header
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
        skip, protoff, pdst = 40, 6, m[24:40]                        # :580-581
    else:
        return drop(L.EAFNOSUPPORT)                                  # :932-933
    if len(m) > IP_MAXPACKET:
        return drop(L.EMSGSIZE)
    front = 0
    encap = (tunnel or saf6 != (v == 6) or                           # :224-228, :543-547
             (any(dst[:alen_a]) and dst[:alen_a] != pdst))
    if encap:
        if not saf6 and (not any(src[:4]) or not any(dst[:4])):      # :938-941
            return drop(L.EINVAL)
    # esp_output's lengths, before anything is written
    oh = (40 if saf6 else 20) if encap else 0
    eskip = oh if encap else skip
    rlen = len(m) + oh - eskip                                       # m_pkthdr.len - skip, xform_esp.c:703
    padding = ((blks - ((rlen + 2) % blks)) % blks) + 2              # :716
    total = eskip + hlen + rlen + padding + alen
    if total > IP_MAXPACKET:                                         # :747
        return drop(L.EMSGSIZE)
    if hlen + oh > headroom or padding + alen > tailroom:            # ipsec_prepend, m_makespace, m_pad
        return drop(L.ENOBUFS)
    m = bytearray(m)
    if encap:
        if v == 4:
            setdf = dfbit if dfbit in (0, 1) else int(m[6] & 0x40 != 0)          # :910-917
            itos, proto = m[1], IPPROTO_IPIP
            m[2:4] = struct.pack(">H", len(m))                       # :230
            m[10:12] = b"\0\0"                                       # :231
            m[10:12] = struct.pack(">H", in_cksum(bytes(m[:skip])))  # :232
        else:
            m[4:6] = struct.pack(">H", len(m) - 40)                  # :533
            itos, proto = (struct.unpack(">I", m[:4])[0] >> 20) & 0xff, IPPROTO_IPV6   # :925
            setdf = 1 if dfbit else 0                                # :926
        if not saf6:                                                 # :942-956
            ip_off = IP_DF if setdf else 0
            idv = 0 if rfc6864 and ip_off & IP_DF else ip_id & 0xffff            # ip_id.c:252
            outer = bytearray(struct.pack(">BBHHHBBH4s4s", 0x45, ip_ecn_ingress(ecn, itos), len(m) + 20, idv,
                                          ip_off, ttl, proto, 0, src[:4], dst[:4]))
        else:                                                        # :965-984
            outer = bytearray(struct.pack(">IHBB16s16s", 0x60000000 | ip_ecn_ingress(ecn, itos) << 20,
                                          len(m), proto, ttl, src[:16], dst[:16]))
        m = outer + m
        front = oh
        skip, protoff = (40, 6) if saf6 else (20, 9)                 # :568-582, :244-260
    # esp_output: m_makespace(m, skip, hlen), m_pad(m, padding + alen)
    wire = list(m[:skip]) + [None] * hlen + list(m[skip:]) + [None] * (padding + alen)
    front += hlen
    nxt = wire[protoff]                                              # :839
    wire[protoff] = IPPROTO_ESP                                      # :842-843
    assert len(wire) == total
    if saf6:                                                         # ipsec_process_done, :742
        wire[4:6] = list(struct.pack(">H", total - 40))
    else:
        wire[2:4] = list(struct.pack(">H", total))                   # :727
        wire[10:12] = [0, 0]
        wire[10:12] = list(struct.pack(">H", in_cksum(bytes(wire[:skip]))))      # ip_output.c:780-782
    return 0, front, wire, nxt


def esp_encap_host(encsa, shape, buf, at, length, headroom, tailroom, ip_id):
    """espgpu_esp_encap, the engine's host rule, on a bytearray that holds the
    cleartext packet at `at` and an L.EncSA: returns (status, front, total,
    reclen, frame)."""
    import ctypes as C
    raw = (C.c_uint8 * (len(buf) - at)).from_buffer(buf, at) if len(buf) > at else None
    res = [C.c_uint32(0xdddddddd) for _ in range(4)]
    rc = L.lib().espgpu_esp_encap(C.byref(encsa), C.byref(shape), C.cast(raw, C.c_void_p) if raw else None, length,
                                  headroom, tailroom, ip_id, *[C.byref(r) for r in res])
    return (rc,) + tuple(r.value for r in res)


def esp_sent_host(encsa, status, length):
    """espgpu_esp_sent: key_sa_recordxfer for one wire packet on an L.EncSA."""
    import ctypes as C
    return L.lib().espgpu_esp_sent(C.byref(encsa), status, length)


# ---- NAT-T: ESP in UDP (netipsec/udpencap.c) ------------------------------------
IPPROTO_TCP, IPPROTO_UDP = 6, 17


def _reduce16(total):
    """REDUCE16 with ADDCARRY (amd64/in_cksum.c:61-73) on a 64-bit sum."""
    l = sum((total >> (16 * k)) & 0xffff for k in range(4))             # q_util.s[0..3]
    total = (l & 0xffff) + (l >> 16)                                    # l_util.s[0] + l_util.s[1]
    if total > 65535:                                                   # ADDCARRY
        total -= 65535
    return total


def in_addword(a, b):
    """in_addword (in_cksum.c:174-181) on two 16-bit values as the host
    loaded them."""
    total = a + b
    if total > 65535:                                                   # ADDCARRY
        total -= 65535
    return total


def in_pseudo(a, b, c):
    """in_pseudo (in_cksum.c:183-193): a and b are the addresses as 32-bit
    loads of their network-order bytes on the little-endian host, c what
    htons() gave."""
    return _reduce16(a + b + c)


def _in_cksumdata(buf):
    """in_cksumdata (in_cksum.c:93-172) for a 4-byte aligned buffer on the
    little-endian host: the dwords, the tail under in_masks, REDUCE32."""
    buf = bytes(buf)
    nw = len(buf) // 4
    total = sum(struct.unpack("<%dI" % nw, buf[:4 * nw]))
    if len(buf) % 4:                                                    # :168-169
        total += int.from_bytes(buf[4 * nw:], "little")
    return sum((total >> (16 * k)) & 0xffff for k in range(4))          # REDUCE32


def in_cksum_skip(m, length, skip):
    """in_cksum_skip (in_cksum.c:195-234) on one contiguous mbuf whose byte
    `skip` is 4-byte aligned."""
    return ~_reduce16(_in_cksumdata(bytes(m)[skip:length])) & 0xffff


def in_delayed_cksum(m, udp, csum_data):
    """in_delayed_cksum (ip_output.c:1059-1091) on a bytearray packet: udp is
    csum_flags & CSUM_UDP, csum_data the field's offset in the transport
    header.  The 16-bit values are the little-endian host's loads."""
    offset = (m[0] & 0xf) << 2                                          # :1066
    if udp:
        cklen = struct.unpack(">H", m[offset + 4:offset + 6])[0]        # ntohs(uh->uh_ulen), :1076
        csum = in_cksum_skip(m, cklen + offset, offset)                 # :1078
        if csum == 0:
            csum = 0xffff                                               # :1079-1080
    else:
        cklen = struct.unpack(">H", m[2:4])[0]                          # ntohs(ip->ip_len), :1082
        csum = in_cksum_skip(m, cklen, offset)                          # :1083
    offset += csum_data                                                 # :1085
    m[offset:offset + 2] = struct.pack("<H", csum)                      # :1087-1090


def udp_ipsec_adjust_cksum(packet, natt_cksum, proto, skip, policy):
    """udp_ipsec_adjust_cksum (udpencap.c:245-293) on a decapsulated packet's
    bytes: natt_cksum is sav->natt->cksum as the host holds it, proto 6 or 17,
    skip the IP header's length, policy V_natt_cksum_policy.  Returns (packet
    bytes, valid): valid stands for csum_flags |= CSUM_DATA_VALID |
    CSUM_PSEUDO_HDR with csum_data 0xffff (:274-276).  What the reference
    leaves to its callers is decided here as the engine decides it: a packet
    too short to hold the field, and under the recompute policy a UDP length
    outside [8, len - skip] or a TCP packet whose ip_len is not the packet's
    length (the reference would sum past the mbuf), come back unchanged."""
    m = bytearray(packet)
    assert proto in (IPPROTO_TCP, IPPROTO_UDP)                          # :253
    off = 6 if proto == IPPROTO_UDP else 16                             # :256-259
    if len(m) - skip < off + 2:
        return bytes(m), False
    at = skip + off
    if policy == 0:                                                     # auto, :261
        if natt_cksum != 0:
            cksum = struct.unpack("<H", m[at:at + 2])[0]                # m_copydata, :264
            if proto == IPPROTO_UDP and cksum == 0:                     # :267-268
                return bytes(m), False
            cksum = in_addword(cksum, natt_cksum)                       # :269
        else:
            if proto == IPPROTO_TCP:                                    # :272-278
                return bytes(m), True
            cksum = 0                                                   # :279
        m[at:at + 2] = struct.pack("<H", cksum)                         # m_copyback, :281
        return bytes(m), False
    if proto == IPPROTO_UDP:
        ulen = struct.unpack(">H", m[skip + 4:skip + 6])[0]
        if ulen < 8 or ulen > len(m) - skip:
            return bytes(m), False
    elif struct.unpack(">H", m[2:4])[0] != len(m):
        return bytes(m), False
    src, dst = struct.unpack("<II", m[12:20])
    htons = lambda x: struct.unpack("<H", struct.pack(">H", x & 0xffff))[0]   # noqa: E731
    cksum = in_pseudo(src, dst, htons(len(m) - skip + proto))           # :284-285
    m[at:at + 2] = struct.pack("<H", cksum)                             # :286
    in_delayed_cksum(m, proto == IPPROTO_UDP, off)                      # :287-290
    return bytes(m), False


def udp_input_encap_checks(pkt, hlen, port):
    """udp_input's way to the UF_ESPINUDP socket for an IPv4 non-fragment
    datagram already trimmed to ip_len (udp_usrreq.c:335-339, :460-475,
    :489-520), as far as the device path follows it: the datagram must be for
    `port`, its length fields sane (:468-472, the trim :474), and its checksum
    field 0: a nonzero one would be verified over the whole datagram, which
    stays the host's.  Returns (status, trimmed packet)."""
    if len(pkt) - hlen < 8:                                             # udps_hdrops: the host's error
        return L.ENOTSUP, pkt
    sport, dport, ulen, uh_sum = struct.unpack(">HHHH", pkt[hlen:hlen + 8])
    if dport != port:                                                   # another socket's
        return L.ENOTSUP, pkt
    if ulen != len(pkt) - hlen:                                         # :468
        if ulen > len(pkt) - hlen or ulen < 8:                          # :469-471
            return L.EINVAL, pkt
        pkt = pkt[:hlen + ulen]                                         # m_adj, :474
    if uh_sum != 0:                                                     # :489-520
        return L.ENOTSUP, pkt
    return 0, pkt


def udp_ipsec_input(sadb, pkt, hlen):
    """udp_ipsec_input (udpencap.c:115-210) for AF_INET: pkt is the datagram
    as udp_input_encap_checks left it, sadb maps an SPI to (sa, proto, af, dst
    bytes, salt, natt) with natt None or (sport, dport).  Returns (status,
    sav): 0 with the SA's tuple for a packet IPsec consumes, ENOTSUP where the
    function returns 0 (the socket gets the datagram: keepalive, IKE)."""
    off = hlen + 8
    if len(pkt) < off + 8:                                              # :131-132
        return L.ENOTSUP, None
    spi = struct.unpack(">I", pkt[off:off + 4])[0]                      # :134
    if spi == 0:                                                        # :135-136
        return L.ENOTSUP, None
    if (len(pkt) - off) % 4:                                            # xform_esp.c:279, before the lookup as the engine's
        return L.EINVAL, None
    sav = sadb.get(spi)                                                 # key_allocsa, :166
    if sav is None:
        return L.ENOENT, None
    sa, proto, saf, sdst, salt = sav[:5]
    natt = sav[5] if len(sav) > 5 else None
    if proto != IPPROTO_ESP or saf != 4 or bytes(sdst)[:4] != pkt[16:20]:      # key.c:1110-1118
        return L.ENOENT, None
    sport, dport = struct.unpack(">HH", pkt[hlen:hlen + 4])
    if natt is None or natt[0] != sport or natt[1] != dport:            # :173-181
        return L.ENOENT, None
    return 0, sav


def ipsec_input_classify_natt(sadb, pkt, off4=0, ipcsum=False, port=0):
    """ipsec_input_classify with the UDP-encapsulation socket on `port`
    (0: none, and the result is ipsec_input_classify's except for the last
    point).  sadb's tuples may carry a sixth member, natt: None or (sport,
    dport).  An IPv4 non-fragment with ip_p 17 goes through
    udp_input_encap_checks and udp_ipsec_input; accepted, the descriptor is
    the ESP record behind the UDP header.  One deliberate difference from the
    reference: a plain ip_p 50 packet whose SA has natt is ENOTSUP, the host
    stack's (ipsec_common_input would take it)."""
    raw = bytes(pkt)
    plain = {spi: tuple(v[:5]) for spi, v in sadb.items()}
    st, d = ipsec_input_classify(plain, raw, off4, ipcsum)
    if st == 0:
        spi = struct.unpack(">I", raw[(d[0] - off4) * 4:(d[0] - off4) * 4 + 4])[0]
        if len(sadb[spi]) > 5 and sadb[spi][5] is not None:
            return L.ENOTSUP, (off4, 0, 0xffff, 0, 0)
        return st, d
    if not port or st != L.ENOTSUP or len(raw) < 20 or raw[0] >> 4 != 4 or raw[9] != IPPROTO_UDP:
        return st, d
    ip_off = struct.unpack(">H", raw[6:8])[0]
    if ip_off & (IP_MF | IP_OFFMASK):
        return st, d
    hlen = (raw[0] & 0xf) << 2
    raw = raw[:struct.unpack(">H", raw[2:4])[0]]                        # the trim, ip_input.c:555-561
    st, raw = udp_input_encap_checks(raw, hlen, port)
    if st == 0:
        st, sav = udp_ipsec_input(sadb, raw, hlen)
    if st:
        return st, (off4, 0, 0xffff, 0, 0)
    return 0, (off4 + (hlen + 8) // 4, len(raw) - hlen - 8, sav[0], 0, sav[4])


def esp_input_decap_natt(mode, prand, ivlen, alen, packet_bytes, skip):
    """esp_input_decap for a packet that came through udp_ipsec_input: `skip`
    covers the IP header and the 8 UDP bytes.  The UDP header is stripped and
    ip_p set first (udpencap.c:149, :196), then esp_input runs with the IP
    header's length as its skip (:208).  Returns esp_input_decap's triple."""
    m = bytes(packet_bytes)
    if skip % 4 or not 28 <= skip <= 68:
        return L.EINVAL, None, 0
    hl = skip - 8
    m = m[:hl] + m[skip:]                                               # m_striphdr(m, hlen, sizeof(*udp)), :196
    m = m[:9] + bytes([IPPROTO_ESP]) + m[10:]                           # :149
    return esp_input_decap(mode, False, prand, ivlen, alen, m, hl)


def udp_ipsec_output(wire, sport, dport):
    """udp_ipsec_output (udpencap.c:212-243) on the wire packet of
    ipsec_output_encap (a list with None for the bytes left to framing and
    encryption), AF_INET: the UDP header behind the IP header, ip_len and
    ip_p; then ip_output's checksum over the finished header
    (ip_output.c:780-782)."""
    hlen = (wire[0] & 0xf) << 2                                         # :226
    total = len(wire) + 8
    udp = struct.pack(">HHHH", sport, dport, total - hlen, 0)           # :233-237
    wire = wire[:hlen] + list(udp) + wire[hlen:]                        # m_makespace, :227
    wire[2:4] = list(struct.pack(">H", total))                          # :240
    wire[9] = IPPROTO_UDP                                               # :241
    wire[10:12] = [0, 0]
    wire[10:12] = list(struct.pack(">H", in_cksum(bytes(wire[:hlen]))))
    return wire


def ipsec_output_encap_natt(tunnel, saf6, src, dst, ttl, dfbit, ecn, rfc6864, ivlen, blks, alen, packet, headroom,
                            tailroom, ip_id, sport, dport):
    """ipsec_output_encap for an SA with natt: ipsec_process_done calls
    udp_ipsec_output on the finished ESP packet (ipsec_output.c:804-813).  An
    AF_INET6 SA is EAFNOSUPPORT (udpencap.c:222-223; decided first here, with
    the SA's other checks).  A wire packet of more than 65535 bytes is
    EMSGSIZE (the reference lets ip_len wrap, :240), and the 8 bytes count
    against the headroom (ENOBUFS, :227-231).  Returns ipsec_output_encap's
    four, front and wire with the UDP header."""
    if saf6:
        return L.EAFNOSUPPORT, 0, None, 0
    st, front, wire, nxt = ipsec_output_encap(tunnel, saf6, src, dst, ttl, dfbit, ecn, rfc6864, ivlen, blks, alen,
                                              packet, headroom, tailroom, ip_id)
    if st:
        return st, front, wire, nxt
    if len(wire) + 8 > IP_MAXPACKET:
        return L.EMSGSIZE, 0, None, 0
    if front + 8 > headroom:
        return L.ENOBUFS, 0, None, 0
    return 0, front + 8, udp_ipsec_output(wire, sport, dport), nxt


def esp_natt_cksum_host(insa, buf, at, length, trailer, policy):
    """espgpu_esp_natt_cksum, the engine's host rule, on a bytearray that
    holds the decapsulated packet at `at` and an L.InSA: returns (status,
    cflags)."""
    import ctypes as C
    raw = (C.c_uint8 * (len(buf) - at)).from_buffer(buf, at)
    cf = C.c_uint8(0xdd)
    rc = L.lib().espgpu_esp_natt_cksum(C.byref(insa), C.cast(raw, C.c_void_p), length, trailer, policy, C.byref(cf))
    return rc, cf.value


def trailer_word(plain_payload):
    """The 32-bit word the kernels' fused trailer check produces for a
    decrypted payload (espgpu_decrypt_batch_trailer, include/espgpu.h):
    next header | pad length << 8 | TR_* flags | TR_VALID."""
    from . import _lib as L
    p = bytes(plain_payload)
    l0, padlen, nh = p[-3], p[-2], p[-1]
    t = nh | (padlen << 8) | L.TR_VALID
    if padlen + 2 > len(p):
        t |= L.TR_BADLEN
    if padlen != l0 and padlen != 0:
        t |= L.TR_BADPAD
    if nh == IPPROTO_NONE:
        t |= L.TR_NONE
    return t


def trailer_accepts(word, prand=False):
    """esp_input_cb's verdict (xform_esp.c:597-630) from a trailer word:
    True = keep the packet.  prand: the SA uses random padding
    (SADB_X_EXT_PRAND), which skips the pad-content check."""
    from . import _lib as L
    if not word & L.TR_VALID or word & (L.TR_BADLEN | L.TR_NONE):
        return False
    return prand or not word & L.TR_BADPAD


def esp_trailer_ok(plain_payload):
    """The checks esp_input_cb makes on the last three plaintext bytes
    (xform_esp.c:597-630, default SADB_X_EXT_PSEQ padding)."""
    p = bytes(plain_payload)
    last = p[-3:]
    if last[1] + 2 > len(p):
        return False
    if last[1] != last[0] and last[1] != 0:
        return False
    return last[2] != IPPROTO_NONE
