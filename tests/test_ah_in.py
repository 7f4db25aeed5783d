"""Inbound AH on the host: the AH branch of espgpu_esp_classify (ESPGPU_CLS_AH),
espgpu_ah_input and espgpu_ah_decap (csrc/classify.h, ah_in.h) against ah.py's
restatements of ipsec_common_input, ah_input, ah_massage_headers and
ah_input_cb.  Every packet sits in a buffer with guard bytes, every save slot
starts random, and the whole of both is compared."""
import struct

import numpy as np
import pytest

import ah_in_helpers as H
import classify_helpers as CH
from espgpu import _lib as L
from espgpu import ah as A
from espgpu import esp as E
from espgpu.batch import sad_build

EINVAL, EACCES, ENOTSUP, ENOENT, EMSGSIZE, EPFNOSUPPORT = L.EINVAL, L.EACCES, L.ENOTSUP, L.ENOENT, L.EMSGSIZE, 96
ANY, TRANSPORT, TUNNEL = E.IPSEC_MODE_ANY, E.IPSEC_MODE_TRANSPORT, E.IPSEC_MODE_TUNNEL


def test_header_and_library_say_ah_batch_is_built():
    src = open(L.HEADER).read()
    assert "#define ESPGPU_HAS_AH_BATCH 1" in src and "#define ESPGPU_ABI_VERSION 6" in src
    names = {"espgpu_ah_input", "espgpu_ah_input_batch", "espgpu_ah_decap", "espgpu_ah_decap_batch"}
    assert names <= set(L.header_symbols())
    assert all(hasattr(L.lib(), s) for s in names) and L.lib().espgpu_abi_version() == 6
    for name, val in (("ESPGPU_CLS_AH", L.CLS_AH), ("ESPGPU_REPLAY_AH", L.REPLAY_AH), ("ESPGPU_IN_AH", L.IN_AH),
                      ("ESPGPU_IN_AH_KEEPTOS", L.IN_AH_KEEPTOS)):
        assert "#define %s " % name in src and ("0x%x" % val) in src.split("#define %s " % name)[1][:12].lower()


# ---- classification -------------------------------------------------------------
@pytest.fixture(scope="module")
def db():
    rng = np.random.default_rng(5101)
    d = CH.Sadb(rng, nesp4=6, nesp6=6, nah=12)
    return d, sad_build(d.entries, 64)


def _cls(db, pkt, flags=L.CLS_AH, off4=77):
    """Host rule == restatement; returns (status, descriptor)."""
    d, table = db
    got = E.esp_classify_host(table, pkt, off4, flags)
    ipcsum = bool(flags & L.CLS_IPCSUM)
    if flags & L.CLS_AH:
        want = A.ipsec_input_classify_ah(d.ref, pkt, off4, ipcsum)
    else:
        want = E.ipsec_input_classify(d.ref, pkt, off4, ipcsum)
    assert got == want, (got, want, bytes(pkt[:48]).hex())
    return got


def _ah4(rng, e, ihl=5, n=24, **kw):
    opts = H.good_options(rng, ihl * 4 - 20)
    body = bytes([6, 4, 0, 0]) + struct.pack(">I", int(e["spi"])) + rng.integers(0, 256, 64, dtype=np.uint8).tobytes()
    return CH.ipv4(CH.dst_of(e), body[:n], ihl=ihl, proto=51, opts=opts, **kw)


def _ah6(rng, e, n=24, **kw):
    body = bytes([6, 4, 0, 0]) + struct.pack(">I", int(e["spi"])) + rng.integers(0, 256, 64, dtype=np.uint8).tobytes()
    return CH.ipv6(CH.dst_of(e), body[:n], nxt=51, **kw)


def test_classify_ah_packets_with_and_without_the_flag(db):
    rng = np.random.default_rng(5102)
    d = db[0]
    seen = set()
    for rep in range(60):
        e4, e6 = d.pick(rng, proto=51, af=4), d.pick(rng, proto=51, af=6)
        ihl = 5 + rep % 11
        n = int(rng.integers(12, 60))                      # no & 3 rule for AH
        for p, e, skip in ((_ah4(rng, e4, ihl, n), e4, ihl * 4), (_ah6(rng, e6, n), e6, 40)):
            for extra in (0, L.CLS_IPCSUM):
                st, desc = _cls(db, p, L.CLS_AH | extra)
                assert st == 0 and desc == (77, skip + n, int(e["sa"]), 0, skip + 12), (st, desc)
                # the flag off: today's answer for the same packet
                assert _cls(db, p, extra) == (ENOTSUP, (77, 0, 0xffff, 0, 0))
            seen.add(n & 3)
    assert seen == {0, 1, 2, 3}


def test_classify_ah_length_rows(db):
    rng = np.random.default_rng(5103)
    d = db[0]
    e4, e6 = d.pick(rng, proto=51, af=4), d.pick(rng, proto=51, af=6)
    for ihl in (5, 8, 15):
        assert _cls(db, _ah4(rng, e4, ihl, 11))[0] == EINVAL
        assert _cls(db, _ah4(rng, e4, ihl, 12))[0] == 0
        assert _cls(db, _ah4(rng, e4, ihl, 7))[0] == EINVAL
    assert _cls(db, _ah6(rng, e6, 11))[0] == EINVAL
    assert _cls(db, _ah6(rng, e6, 12))[0] == 0
    # bytes past ip_len / plen are trimmed: the record is the IP packet
    st, desc = _cls(db, _ah4(rng, e4, 6, 40, tail=b"x" * 9))
    assert st == 0 and desc[1] == 64
    st, desc = _cls(db, _ah6(rng, e6, 40, tail=b"x" * 9))
    assert st == 0 and desc[1] == 80
    # IPv6: 40 + plen at the descriptor's limit
    body = bytes([6, 4, 0, 0]) + struct.pack(">I", int(e6["spi"])) + bytes(65535 - 40 - 8)
    p = CH.ipv6(CH.dst_of(e6), body, nxt=51)
    assert len(p) == 65535
    st, desc = _cls(db, p)
    assert st == 0 and desc == (77, 65535, int(e6["sa"]), 0, 52)
    st, desc = _cls(db, CH.ipv6(CH.dst_of(e6), body + b"\0", nxt=51))
    assert (st, desc) == (ENOTSUP, (77, 0, 0xffff, 0, 0))
    # earlier rows still decide first: fragments, link-local, jumbogram, a short buffer
    assert _cls(db, _ah4(rng, e4, 5, 24, off=0x2000))[0] == ENOTSUP
    ll = bytearray(_ah6(rng, e6, 11))
    ll[24:26] = b"\xfe\x80"
    assert _cls(db, bytes(ll))[0] == ENOTSUP               # fe80::/10 before the length row
    assert _cls(db, _ah6(rng, e6, 24, plen=0))[0] == ENOTSUP
    assert _cls(db, _ah6(rng, e6, 24, plen=25))[0] == EINVAL
    assert _cls(db, _ah4(rng, e4, 5, 24, bad_sum=True), L.CLS_AH | L.CLS_IPCSUM)[0] == EINVAL


def test_classify_ah_lookup_rows(db):
    rng = np.random.default_rng(5104)
    d = db[0]
    a4, a6 = d.pick(rng, proto=51, af=4), d.pick(rng, proto=51, af=6)
    s4, s6 = d.pick(rng, proto=50, af=4), d.pick(rng, proto=50, af=6)
    # an ESP entry's SPI in an AH packet, and the reverse
    assert _cls(db, _ah4(rng, s4))[0] == ENOENT and _cls(db, _ah6(rng, s6))[0] == ENOENT
    for e in (a4, a6):
        p = CH.esp_payload(rng, int(e["spi"]), 24)
        esp = CH.ipv4(CH.dst_of(e), p) if e["af"] == 4 else CH.ipv6(CH.dst_of(e), p)
        assert _cls(db, esp)[0] == ENOENT
    # ESP packets are classified as ever under the flag
    for kind, (build, _) in CH.KINDS.items():
        for _ in range(4):
            p = build(rng, d)
            if len(p) >= 20 and ((p[0] >> 4 == 4 and p[9] == 51) or (p[0] >> 4 == 6 and len(p) >= 40 and p[6] == 51)):
                continue
            assert _cls(db, p, L.CLS_AH) == _cls(db, p, 0), kind
    # an unknown SPI, SPI 0, a wrong destination, the other family
    for bad in (d.unknown_spi(rng), 0):
        q = bytearray(_ah4(rng, a4))
        q[24:28] = struct.pack(">I", bad)
        assert _cls(db, bytes(q))[0] == ENOENT
    q = bytearray(_ah4(rng, a4))
    q[19] ^= 1
    assert _cls(db, bytes(q))[0] == ENOENT
    body = bytes([6, 4, 0, 0]) + struct.pack(">I", int(a6["spi"])) + bytes(16)
    assert _cls(db, CH.ipv4(CH.dst_of(a6)[:4], body, proto=51))[0] == ENOENT
    # the SPI is read at skip + 4, not at skip: an AH SPI in the first dword finds nothing
    q = bytearray(_ah4(rng, a4))
    q[20:24], q[24:28] = q[24:28], struct.pack(">I", d.unknown_spi(rng))
    assert _cls(db, bytes(q))[0] == ENOENT
    # unknown flag bits stay refused
    assert E.esp_classify_host(db[1], _ah4(rng, a4), 0, 0x8)[0] == EINVAL
    assert E.esp_classify_host(db[1], _ah4(rng, a4), 0, 0x2)[0] == EINVAL


# ---- espgpu_ah_input -------------------------------------------------------------
def test_input_every_header_length_and_icv_length():
    rng = np.random.default_rng(5110)
    for mlen in H.MLENS:
        for ihl in range(5, 16):
            for rep in range(6):
                opts = H.good_options(rng, ihl * 4 - 20)
                p, skip = H.ah_packet4(rng, ihl, opts, 6, mlen, int(rng.integers(0, 50)))
                for keeptos in (False, True):
                    st, after, _ = H.check_input(rng, H.ah_flags(int(rng.integers(3)), False, keeptos), mlen, p, skip)
                    assert st == 0
                    assert (after[1] == p[1]) if keeptos else (after[1] == 0)
                    assert after[8] == 0 and after[6:8] == b"\0\0" and after[10:12] == b"\0\0"
                    assert after[:1] + after[2:6] + after[9:10] + after[12:20] == p[:1] + p[2:6] + p[9:10] + p[12:20]
        for rep in range(6):
            p, skip = H.ah_packet6(rng, 6, mlen, int(rng.integers(0, 50)))
            st, after, _ = H.check_input(rng, H.ah_flags(int(rng.integers(3)), True), mlen, p, 40)
            assert st == 0 and after[:4] == b"\x60\0\0\0" and after[7] == 0 and after[4:7] == p[4:7]
            assert after[8:40] == p[8:40]


def test_input_options_kept_and_zeroed():
    rng = np.random.default_rng(5111)
    for t in H.KEEP:
        body = rng.integers(1, 256, 6, dtype=np.uint8).tobytes()
        opts = bytes([1, t, 8]) + body + bytes([1, 1, 1])
        p, skip = H.ah_packet4(rng, 8, opts, 6, 12, 20)
        st, after, _ = H.check_input(rng, H.ah_flags(), 12, p, skip)
        assert st == 0 and after[20:32] == opts
    for t in (A.IPOPT_LSRR, A.IPOPT_SSRR, 0x44, 0x07, 0xde):
        body = rng.integers(1, 256, 9, dtype=np.uint8).tobytes()
        opts = bytes([t, 11]) + body + bytes([1])
        p, skip = H.ah_packet4(rng, 8, opts, 6, 12, 20)
        st, after, _ = H.check_input(rng, H.ah_flags(), 12, p, skip)
        assert st == 0 and after[20:32] == bytes(11) + b"\x01"
        assert after[16:20] == p[16:20]                    # inbound: the destination stays (out = 0)
    # a kept and a zeroed option side by side, across dword boundaries
    opts = bytes([0x94, 4, 0, 0, 0x44, 7, 1, 2, 3, 4, 5, 0x82, 5, 9, 9, 9])
    p, skip = H.ah_packet4(rng, 9, opts, 6, 12, 8)
    st, after, _ = H.check_input(rng, H.ah_flags(), 12, p, skip)
    assert st == 0 and after[20:36] == bytes([0x94, 4, 0, 0]) + bytes(7) + bytes([0x82, 5, 9, 9, 9])
    # EOL in the middle: whatever follows is neither parsed nor zeroed
    opts = bytes([1, 0, 0x83, 0, 0x44, 1, 0xff, 0xff])
    p, skip = H.ah_packet4(rng, 7, opts, 6, 12, 8)
    st, after, _ = H.check_input(rng, H.ah_flags(), 12, p, skip)
    assert st == 0 and after[20:28] == opts
    # an option that ends exactly at the header's end
    opts = bytes([1, 1, 0x83, 6, 1, 2, 3, 4])
    p, skip = H.ah_packet4(rng, 7, opts, 6, 12, 8)
    st, after, _ = H.check_input(rng, H.ah_flags(), 12, p, skip)
    assert st == 0 and after[20:28] == bytes([1, 1]) + bytes(6)
    # a 40-byte option over the whole area
    opts = bytes([0x44, 40]) + rng.integers(1, 256, 38, dtype=np.uint8).tobytes()
    p, skip = H.ah_packet4(rng, 15, opts, 6, 12, 8)
    st, after, _ = H.check_input(rng, H.ah_flags(), 12, p, skip)
    assert st == 0 and after[20:60] == bytes(40)


def test_input_option_refusals():
    rng = np.random.default_rng(5112)
    for ihl in range(6, 16):
        for kind in ("lone", "len0", "len1", "past"):
            for rep in range(4):
                opts = H.bad_options(rng, ihl * 4 - 20, kind)
                p, skip = H.ah_packet4(rng, ihl, opts, 6, 12, 16)
                assert H.check_input(rng, H.ah_flags(), 12, p, skip)[0] == EINVAL, (ihl, kind, opts.hex())
    # EOL and NOP in the header's last byte are fine
    for last in (0, 1):
        p, skip = H.ah_packet4(rng, 6, bytes([1, 1, 1, last]), 6, 12, 16)
        assert H.check_input(rng, H.ah_flags(), 12, p, skip)[0] == 0
    # a long option that would run far past the header
    p, skip = H.ah_packet4(rng, 6, bytes([0x83, 255, 1, 1]), 6, 12, 300)
    assert H.check_input(rng, H.ah_flags(), 12, p, skip)[0] == EINVAL


def test_input_flags_and_skip_refusals():
    rng = np.random.default_rng(5113)
    p4, _ = H.ah_packet4(rng, 6, bytes([1, 1, 1, 1]), 6, 12, 16)
    p6, _ = H.ah_packet6(rng, 6, 12, 16)
    good4, good6 = H.ah_flags(), H.ah_flags(af6=True)
    for f in (good4 & ~L.IN_AH, good4 | L.IN_PAD_RAND, good4 | L.IN_NATT, good4 | 0x10, good4 | 0x100,
              good4 | 0x80000000, good4 | L.IN_TRANSPORT | L.IN_TUNNEL, L.IN_AH_KEEPTOS, 0):
        assert H.check_input(rng, f, 12, p4, 24, want=EINVAL)[0] == EINVAL, hex(f)
    # the SA's family against the packet's
    assert H.check_input(rng, good6, 12, p4, 24, want=EINVAL)[0] == EINVAL
    assert H.check_input(rng, good4, 12, p6, 40)[0] == EINVAL
    assert H.check_input(rng, good6, 12, p6, 40)[0] == 0
    # salt below 32, an unaligned skip, ip_hl against skip, IPv6 with another skip
    insa = L.InSA(0, 0, good4, 0)
    for salt in (0, 4, 11, 12, 28, 31, 33, 34, 35, 32, 40, 76):
        buf, slot = bytearray(p4), bytearray(64)
        assert A.ah_input_host(insa, 12, buf, len(p4), salt, slot) == EINVAL, salt
        assert bytes(buf) == p4 and bytes(slot) == bytes(64)
    insa6 = L.InSA(0, 0, good6, 0)
    for salt in (32, 48, 56, 60):
        buf, slot = bytearray(p6), bytearray(64)
        assert A.ah_input_host(insa6, 12, buf, len(p6), salt, slot) == EINVAL, salt
    # len < skip + 12
    for ln in (0, 1, 20, 24, 35):
        assert H.check_input(rng, good4, 12, p4, 24, length=ln)[0] == EINVAL
    assert H.check_input(rng, good6, 12, p6, 40, length=51)[0] == EINVAL
    # mlen the engine has no session for; null pointers
    for mlen in (0, 2, 10, 68, 1 << 20):
        assert A.ah_input_host(insa, mlen, bytearray(p4), len(p4), 36, bytearray(64)) == EINVAL
    lib = L.lib()
    assert lib.espgpu_ah_input(None, 12, p4, len(p4), 36, bytes(64)) == EINVAL
    assert lib.espgpu_ah_input(insa, 12, None, len(p4), 36, bytes(64)) == EINVAL
    assert lib.espgpu_ah_input(insa, 12, p4, len(p4), 36, None) == EINVAL


def test_input_header_length_rows():
    rng = np.random.default_rng(5114)
    for af6 in (False, True):
        for mlen in H.MLENS:
            flags = H.ah_flags(af6=af6)
            ahsize = A.ah_hdrsiz(mlen, af6)
            assert ahsize == {(False, 12): 24, (False, 16): 28, (False, 24): 36, (False, 32): 44,
                              (True, 12): 24, (True, 16): 32, (True, 24): 40, (True, 32): 48}[(af6, mlen)]
            right = (ahsize - 8) // 4
            mk = (lambda **kw: H.ah_packet6(rng, 6, mlen, 0, **kw)) if af6 else \
                 (lambda **kw: H.ah_packet4(rng, 7, H.good_options(rng, 8), 6, mlen, 0, **kw))
            for ah_len, st in ((right, 0), (right - 1, EACCES), (right + 1, EACCES), (0, EACCES), (255, EACCES)):
                p, skip = mk(ah_len=ah_len)
                assert H.check_input(rng, flags, mlen, p, skip)[0] == st
            # skip + ahsize == len passes; one byte less is refused (xform_ah.c:591)
            p, skip = mk()
            assert len(p) == skip + ahsize and H.check_input(rng, flags, mlen, p, skip)[0] == 0
            assert H.check_input(rng, flags, mlen, p, skip, length=len(p) - 1)[0] == EACCES
            # ah_len is checked before the length (:581 before :591)
            p, skip = mk(ah_len=right + 1)
            assert H.check_input(rng, flags, mlen, p, skip, length=len(p) - 1)[0] == EACCES
    # the header-length rows come before the massage: a bad option behind a bad ah_len
    p, skip = H.ah_packet4(rng, 6, bytes([0x83, 1, 1, 1]), 6, 12, 8, ah_len=9)
    assert H.check_input(rng, H.ah_flags(), 12, p, skip)[0] == EACCES


def test_input_ipv6_rows():
    rng = np.random.default_rng(5115)
    flags = H.ah_flags(af6=True)
    # mlen 16: ahsize 32, four padding bytes behind the ICV stay in the hashed packet
    p, _ = H.ah_packet6(rng, 6, 16, 24)
    st, after, slot = H.check_input(rng, flags, 16, p, 40)
    assert st == 0 and after[40:] == p[40:] and len(p) == 40 + 32 + 24
    # jumbogram
    p, _ = H.ah_packet6(rng, 6, 12, 24, plen=0)
    assert H.check_input(rng, flags, 12, p, 40)[0] == EMSGSIZE
    # link-local source, destination, both: the embedded scope id goes; fec0::/10 and ff02:: stay
    for src, dst, zs, zd in ((b"\xfe\x80\x12\x34", None, True, False), (None, b"\xfe\xbf\x00\x07", False, True),
                             (b"\xfe\x9a\xff\xff", b"\xfe\x80\x00\x01", True, True),
                             (b"\xfe\xc0\x12\x34", b"\xff\x02\x00\x05", False, False)):
        tail = rng.integers(1, 256, 12, dtype=np.uint8).tobytes()
        p, _ = H.ah_packet6(rng, 6, 12, 24, src=src + tail if src else None, dst=dst + tail if dst else None)
        st, after, _ = H.check_input(rng, flags, 12, p, 40)
        assert st == 0
        assert after[10:12] == (b"\0\0" if zs else p[10:12]) and after[26:28] == (b"\0\0" if zd else p[26:28])
        assert after[8:10] == p[8:10] and after[12:26] == p[12:26] and after[28:40] == p[28:40]
    # the traffic class and flow label go, whatever KEEPTOS says
    p, _ = H.ah_packet6(rng, 6, 12, 24)
    st, after, _ = H.check_input(rng, flags | L.IN_AH_KEEPTOS, 12, p, 40)
    assert st == 0 and after[:4] == b"\x60\0\0\0"


# ---- espgpu_ah_decap -------------------------------------------------------------
def _through_input(rng, flags, mlen, p, skip):
    st, after, slot = H.check_input(rng, flags, mlen, p, skip)
    assert st == 0
    return after, slot


@pytest.mark.parametrize("af6", [False, True], ids=["inet", "inet6"])
def test_decap_modes_next_headers_and_limits(af6):
    rng = np.random.default_rng(5120 + af6)
    seen = set()
    for mode in (ANY, TRANSPORT, TUNNEL):
        for nxt in (4, 41, 6, 17, 50):
            for mlen in H.MLENS:
                for q in (0, 19, 20, 39, 40, 41, int(rng.integers(0, 400))):
                    flags = H.ah_flags(mode, af6, keeptos=bool(q & 1))
                    if af6:
                        p, skip = H.ah_packet6(rng, nxt, mlen, q)
                    else:
                        ihl = int(rng.integers(5, 16))
                        p, skip = H.ah_packet4(rng, ihl, H.good_options(rng, ihl * 4 - 20), nxt, mlen, q)
                    after, slot = _through_input(rng, flags, mlen, p, skip)
                    b0, p0 = int(rng.integers(0, 2**40)), int(rng.integers(0, 2**30))
                    st, res = H.check_decap(rng, flags, mlen, after, slot, skip, b0, p0)
                    inner = (nxt == 4 or nxt == 41) and mode != TRANSPORT
                    if inner:
                        want = EINVAL if q < (20 if nxt == 4 else 40) else 0
                    else:
                        want = EPFNOSUPPORT if (mode == TUNNEL and not af6) else 0
                    assert st == want, (mode, nxt, mlen, q, st, want)
                    seen.add((st, inner))
                    if st:
                        continue
                    off, out = res
                    ahsize = A.ah_hdrsiz(mlen, af6)
                    if inner:                              # tunnel: the payload, untouched
                        assert off == skip + ahsize and out == p[skip + ahsize:]
                    else:                                  # transport: the original header, fixed, then the payload
                        assert off == ahsize and len(out) == skip + q and out[skip:] == p[skip + ahsize:]
                        if af6:
                            assert out[:4] == p[:4] and out[7] == p[7] and out[6] == nxt and out[8:40] == p[8:40]
                            assert struct.unpack(">H", out[4:6])[0] == q
                        else:
                            assert out[9] == nxt and struct.unpack(">H", out[2:4])[0] == skip + q
                            assert out[1] == p[1] and out[8] == p[8] and out[4:8] == p[4:8] and out[12:skip] == p[12:skip]
                            assert E.in_cksum(out[:skip]) == 0
                            h = bytearray(out[:skip])
                            h[10:12] = b"\0\0"
                            assert out[10:12] == struct.pack(">H", E.in_cksum(bytes(h)))
    assert seen >= {(0, True), (0, False), (EINVAL, True)} and (af6 or (EPFNOSUPPORT, False) in seen)


def test_decap_refusals_and_counters():
    rng = np.random.default_rng(5125)
    flags = H.ah_flags(TRANSPORT)
    p, skip = H.ah_packet4(rng, 6, bytes([1, 1, 1, 1]), 6, 12, 40)
    after, slot = _through_input(rng, flags, 12, p, skip)
    for f in (flags & ~L.IN_AH, flags | L.IN_PAD_RAND, flags | L.IN_NATT, flags | 0x10, flags | L.IN_TUNNEL,
              flags | 0x100):
        assert H.check_decap(rng, f, 12, after, slot, skip, want=EINVAL)[0] == EINVAL, hex(f)
    # the SA's family against the saved header; a slot that holds no such header
    assert H.check_decap(rng, H.ah_flags(TRANSPORT, af6=True), 12, after, slot, skip, want=EINVAL)[0] == EINVAL
    bad = bytearray(slot)
    bad[0] = 0x45
    assert H.check_decap(rng, flags, 12, after, bytes(bad), skip, want=EINVAL)[0] == EINVAL
    # a packet shorter than its AH header (espgpu_ah_input would have refused it)
    assert H.check_decap(rng, flags, 12, after[:skip + 23], slot, skip, want=EINVAL)[0] == EINVAL
    # the counters wrap like the reference's uint64_t
    st, _ = H.check_decap(rng, flags, 12, after, slot, skip, bytes0=2**64 - 10, packets0=2**32 - 1)
    assert st == 0
    lib, insa = L.lib(), L.InSA(0, 0, flags, 0)
    import ctypes as C
    off, ln = C.c_uint32(5), C.c_uint32(5)
    assert lib.espgpu_ah_decap(None, 12, after, len(after), skip + 12, slot, C.byref(off), C.byref(ln)) == EINVAL
    assert (off.value, ln.value) == (0, 0)
    assert lib.espgpu_ah_decap(C.byref(insa), 12, after, len(after), skip + 12, None, C.byref(off), C.byref(ln)) == EINVAL
    assert lib.espgpu_ah_decap(C.byref(insa), 10, after, len(after), skip + 12, slot, C.byref(off), C.byref(ln)) == EINVAL


def test_esp_decap_still_refuses_the_ah_flags():
    import decap_helpers as DH
    rng = np.random.default_rng(5126)
    p, skip, rlen = DH.packet(rng, False, 8, 16, 40, 6)
    for f in (L.IN_AH, L.IN_AH_KEEPTOS, L.IN_AH | L.IN_TRANSPORT):
        assert DH.check_one(rng, f, 8, 16, p, skip, rlen, want=EINVAL) == EINVAL
