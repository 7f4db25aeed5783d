"""espgpu_ah_encap, espgpu_ah_frame and espgpu_ah_sent, the host rules of the
outbound AH block (csrc/ah_out.h), against ah.py's restatements of
ipsec4/6_perform_request, ipsec_encap, ah_output with ah_massage_headers (out =
1) and ah_output_cb.  Every packet sits in a buffer with guard bytes and, where
the test does not set it, exactly the headroom it needs; the whole buffer and
the save slot are compared, so a byte written outside the named ones fails."""
import struct

import numpy as np
import pytest

import ah_in_helpers as H
import ah_out_helpers as O
from encap_helpers import addr, encsa
from espgpu import _lib as L
from espgpu import ah as A
from espgpu import esp as E

EINVAL, EACCES, ENOTSUP, EMSGSIZE, EAFNOSUPPORT, ENOBUFS = O.EINVAL, O.EACCES, O.ENOTSUP, O.EMSGSIZE, O.EAFNOSUPPORT, O.ENOBUFS


def _sa(rng, saf6, dst=None, keeptos=False, **kw):
    return encsa(O.ah_enc_flags(af6=saf6, keeptos=keeptos, **kw), int(rng.integers(1, 256)), addr(rng, saf6),
                 dst or addr(rng, saf6))


def test_has_ah_out_symbols_and_flags():
    lib = L.lib()
    for name in ("espgpu_ah_encap", "espgpu_ah_frame", "espgpu_ah_sent", "espgpu_ah_encap_batch",
                 "espgpu_ah_frame_batch", "espgpu_ah_sent_batch"):
        assert hasattr(lib, name), name
    hdr = open(L.HEADER).read()
    assert "#define ESPGPU_HAS_AH_OUT 1" in hdr
    assert (L.ENC_AH, L.ENC_AH_KEEPTOS) == (0x80, 0x100)
    for name in ("espgpu_ah_encap", "espgpu_ah_frame", "espgpu_ah_sent"):
        assert name in L.header_symbols()


@pytest.mark.parametrize("saf6", [False, True], ids=["sa4", "sa6"])
@pytest.mark.parametrize("v6", [False, True], ids=["pkt4", "pkt6"])
def test_every_ip_hl_mlen_family_mode_and_the_proxy_case(saf6, v6):
    rng = np.random.default_rng(7100 + 2 * saf6 + v6)
    seen = set()
    for ihl in ([5] if v6 else range(5, 16)):
        for mlen in O.MLENS:
            for tunnel in (False, True):
                for proxy in ("same", "other"):
                    pdst = addr(rng, v6)
                    sdst = pdst if proxy == "same" and saf6 == v6 else addr(rng, saf6)
                    e = _sa(rng, saf6, dst=sdst, tunnel=tunnel, keeptos=bool(ihl & 1))
                    plen = int(rng.integers(0, 90))
                    p = O.clear6(rng, plen, dst=pdst) if v6 else O.clear4(rng, ihl, O.good_options(rng, ihl * 4 - 20),
                                                                        plen, dst=pdst)
                    st, front, hashed, slot, hs = O.check_encap(rng, e, mlen, p, ip_id=int(rng.integers(65536)))
                    assert st == 0
                    ahsize = A.ah_hdrsiz(mlen, saf6)
                    encap = front > ahsize
                    assert encap == (tunnel or saf6 != v6 or proxy == "other")
                    assert front == ahsize + ((40 if saf6 else 20) if encap else 0)
                    assert hs == ((40 if saf6 else 20) if encap else (40 if v6 else ihl * 4))
                    seen.add((encap, proxy, tunnel))
                    # the saved header is the wire header: protocol 51, the final length, a checksum that verifies
                    if saf6:
                        assert slot[6] == 51 and struct.unpack(">H", slot[4:6])[0] == len(hashed) - 40
                    else:
                        assert slot[9] == 51 and struct.unpack(">H", slot[2:4])[0] == len(hashed)
                        assert E.in_cksum(slot[:hs]) == 0
                    assert hashed[hs + 1] == (ahsize - 8) // 4 and hashed[hs + 2:hs + 4] == b"\0\0"
                    assert hashed[hs] == ((41 if v6 else 4) if encap else p[6 if v6 else 9])
                    if encap and not v6:                             # the inner header verifies
                        assert E.in_cksum(hashed[front:front + ihl * 4]) == 0
                        assert struct.unpack(">H", hashed[front + 2:front + 4])[0] == len(p)
    assert len(seen) == 4 and {s[0] for s in seen} == ({False, True} if saf6 == v6 else {True}), seen


def test_the_proxy_case_with_an_unspecified_sa_destination():
    rng = np.random.default_rng(7105)
    for tunnel in (False, True):
        e = _sa(rng, False, dst=bytes(4), tunnel=tunnel)
        p = O.clear4(rng, 6, O.good_options(rng, 4), 30)
        st, front, _, _, _ = O.check_encap(rng, e, 12, p)
        assert (st, front) == ((EINVAL, 0) if tunnel else (0, 24))   # ipsec_output.c:938-941; transport
    e = _sa(rng, True)
    e.dst[:] = [0] * 16
    assert O.check_encap(rng, e, 12, O.clear6(rng, 9))[0] == EINVAL      # :961-964


@pytest.mark.parametrize("v6", [False, True], ids=["inner4", "inner6"])
def test_df_policy_ecn_and_rfc6864(v6):
    rng = np.random.default_rng(7106 + v6)
    for dfbit in (0, 1, 2):
        for idf in (False, True):
            for ecn in (0, 1, -1):
                for iecn in range(4):
                    for rfc in (False, True):
                        for saf6 in (False, True):
                            tos = int(rng.integers(64)) << 2 | iecn
                            e = _sa(rng, saf6, tunnel=True, dfbit=dfbit, ecn=ecn, rfc6864=rfc)
                            p = O.clear6(rng, 33, tc=tos) if v6 else O.clear4(rng, 6, O.good_options(rng, 4), 33,
                                                                             df=idf, tos=tos)
                            st, front, hashed, slot, hs = O.check_encap(rng, e, 16, p, ip_id=0xbeef)
                            assert st == 0
                            otos = slot[1] if not saf6 else (struct.unpack(">I", slot[:4])[0] >> 20) & 0xff
                            assert otos >> 2 == tos >> 2
                            assert otos & 3 == {0: 0, 1: 2 if iecn == 3 else iecn, -1: iecn}[ecn]
                            if not saf6:
                                df = bool(slot[6] & 0x40)
                                assert df == {0: False, 1: True, 2: idf if not v6 else True}[dfbit]
                                assert slot[4:6] == (b"\0\0" if rfc and df else b"\xbe\xef")
                                assert slot[8] == e.ttl and slot[9] == 51 and E.in_cksum(slot[:20]) == 0
                                # hashed: tos, off, ttl and sum zeroed; id, protocol, addresses kept
                                assert hashed[1] == 0 and hashed[6:9] == b"\0\0\0" and hashed[10:12] == b"\0\0"
                                assert hashed[4:6] == slot[4:6] and hashed[12:20] == slot[12:20]
                            else:
                                assert slot[7] == e.ttl and slot[6] == 51
                                assert hashed[:4] == b"\x60\0\0\0" and hashed[7] == 0 and hashed[4:7] == slot[4:7]


def _transport4(rng, opts, keeptos=False, mlen=12, plen=21, want=None):
    ihl = 5 + len(opts) // 4
    pdst = addr(rng, False)
    e = _sa(rng, False, dst=pdst, keeptos=keeptos)
    p = O.clear4(rng, ihl, opts, plen, dst=pdst)
    return (p,) + O.check_encap(rng, e, mlen, p, want=want)


def test_every_kept_and_every_zeroed_option_and_keeptos():
    rng = np.random.default_rng(7108)
    for typ in H.KEEP + H.ZEROED + (0x99, 0x02):
        for ln in (2, 3, 4, 7, 8, 11, 39):
            if typ in (0x83, 0x89) and ln < 4:
                continue
            body = bytes([typ, ln]) + rng.integers(1, 255, ln - 2, dtype=np.uint8).tobytes()
            opts = bytes([1]) + body + bytes([1]) * ((-1 - ln) % 4)
            for keeptos in (False, True):
                p, st, front, hashed, slot, hs = _transport4(rng, opts, keeptos)
                assert st == 0 and hs == 20 + len(opts)
                got = hashed[21:21 + ln]
                assert got == (body if typ in H.KEEP else bytes(ln)), (hex(typ), ln)
                assert hashed[20] == 1 and hashed[1] == (p[1] if keeptos else 0)
                assert slot[20:hs] == opts and slot[1] == p[1]      # the wire header keeps them all


def test_eol_mid_header_ends_the_loop():
    rng = np.random.default_rng(7109)
    tail = bytes([0x83, 1, 0x44, 0, 7, 200, 9])                     # never looked at
    opts = bytes([0x44, 4, 5, 6, 0]) + tail
    p, st, front, hashed, slot, hs = _transport4(rng, opts)
    assert st == 0 and hashed[20:24] == bytes(4) and hashed[24:32] == bytes([0]) + tail
    assert hashed[16:20] == p[16:20]


def test_each_option_refusal_at_the_last_byte_writes_nothing():
    rng = np.random.default_rng(7110)
    for room in (4, 8, 20, 40):
        for kind in ("lone", "len0", "len1", "past"):
            for _ in range(6):
                _, st, *_ = _transport4(rng, H.bad_options(rng, room, kind))
                assert st == EINVAL, (room, kind)
    # in tunnel mode the inner header's options are not walked
    e = _sa(rng, False, tunnel=True)
    p = O.clear4(rng, 7, H.bad_options(rng, 8, "len0"), 12)
    assert O.check_encap(rng, e, 12, p)[0] == 0


@pytest.mark.parametrize("typ", [0x83, 0x89], ids=["lsrr", "ssrr"])
def test_source_route_destination_swap(typ):
    rng = np.random.default_rng(7111 + typ)
    for ln in (2, 3):                                                # the deliberate difference
        opts = O.sr_option(rng, typ, ln) + bytes([1]) * (4 - ln)
        # (the restatement refuses it too; `want` pins the code itself)
        assert _transport4(rng, opts, want=EINVAL)[1] == EINVAL
        assert _transport4(rng, opts)[1] == EINVAL
    for ln in (4, 7, 11):
        for lead in (0, 1, 2):
            o = O.sr_option(rng, typ, ln)
            opts = bytes([1]) * lead + o
            opts += bytes([1]) * (-len(opts) % 4)
            p, st, front, hashed, slot, hs = _transport4(rng, opts)
            assert st == 0
            assert hashed[16:20] == o[ln - 4:ln] != p[16:20]         # the hashed ip_dst: the option's last address
            assert slot[16:20] == p[16:20] and slot[20:hs] == opts   # the wire header: untouched
            assert hashed[20 + lead:20 + lead + ln] == bytes(ln)


def test_two_source_route_options_the_last_one_wins():
    rng = np.random.default_rng(7113)
    for t1, t2 in ((0x83, 0x89), (0x89, 0x83), (0x83, 0x83)):
        a, b = O.sr_option(rng, t1, 7), O.sr_option(rng, t2, 11)
        opts = a + bytes([1]) + b + bytes([1])
        p, st, front, hashed, slot, hs = _transport4(rng, opts)
        assert st == 0 and hashed[16:20] == b[7:11] and hashed[20:40] == bytes(7) + b"\x01" + bytes(11) + b"\x01"
    # a second one that is too short refuses the packet although the first was good
    opts = O.sr_option(rng, 0x83, 7) + bytes([1]) + O.sr_option(rng, 0x89, 3) + bytes([1])
    assert _transport4(rng, opts)[1] == EINVAL


def test_ipv6_padding_flow_and_link_local_packet_addresses():
    rng = np.random.default_rng(7114)
    for mlen, pad in ((12, 0), (16, 4), (24, 4), (32, 4), (20, 0)):
        for ll in (False, True):
            src = bytes([0xfe, 0x80 | int(rng.integers(64)), 0x12, 0x34]) + addr(rng, True)[4:] if ll else None
            pdst = addr(rng, True)      # (a link-local destination cannot go by transport: the SA's would match it)
            e = _sa(rng, True, dst=pdst)
            p = O.clear6(rng, 17, dst=pdst, src=src)
            st, front, hashed, slot, hs = O.check_encap(rng, e, mlen, p)
            assert st == 0 and hs == 40 and front == 12 + mlen + pad == A.ah_hdrsiz(mlen, True)
            assert hashed[40 + 12 + mlen:40 + front] == bytes(pad)   # written, and hashed
            assert hashed[:4] == b"\x60\0\0\0" and hashed[7] == 0
            assert hashed[10:12] == (b"\0\0" if ll else p[10:12]) and hashed[24:40] == p[24:40]
            assert slot[8:40] == p[8:40] and slot[:4] == p[:4] and slot[7] == p[7]


def test_lengths_at_the_limit_and_headroom_one_byte_short():
    rng = np.random.default_rng(7115)
    for saf6, v6, tunnel in ((False, False, False), (False, False, True), (True, True, False), (True, False, True)):
        for mlen in (12, 32):
            over = A.ah_hdrsiz(mlen, saf6) + ((40 if saf6 else 20) if tunnel else 0)
            hdr = 40 if v6 else 24
            for total, want in ((65535, 0), (65536, EMSGSIZE)):
                plen = total - over - hdr
                pdst = addr(rng, v6)
                e = _sa(rng, saf6, dst=pdst if saf6 == v6 else None, tunnel=tunnel)
                p = O.clear6(rng, plen, dst=pdst) if v6 else O.clear4(rng, 6, O.good_options(rng, 4), plen, dst=pdst)
                st, front, hashed, _, _ = O.check_encap(rng, e, mlen, p, headroom=over)
                assert st == want and (st or len(hashed) == 65535)
            p = O.clear6(rng, 5, dst=pdst) if v6 else O.clear4(rng, 6, O.good_options(rng, 4), 5, dst=pdst)
            assert O.check_encap(rng, e, mlen, p, headroom=over)[0] == 0
            assert O.check_encap(rng, e, mlen, p, headroom=over - 1)[0] == ENOBUFS
            assert O.check_encap(rng, e, mlen, p, headroom=0)[0] == ENOBUFS
    e = _sa(rng, False)
    assert O.check_encap(rng, e, 12, O.clear4(rng, 5, b"", 65516, consistent=False))[0] == EMSGSIZE    # len 65536 itself
    # the packet checks of the ESP rule
    assert O.check_encap(rng, e, 12, O.clear4(rng, 5, b"", 0)[:19])[0] == EINVAL
    assert O.check_encap(rng, e, 12, b"\x44" + O.clear4(rng, 5, b"", 9)[1:])[0] == EINVAL
    assert O.check_encap(rng, e, 12, O.clear4(rng, 9, O.good_options(rng, 16), 0)[:35])[0] == EINVAL
    assert O.check_encap(rng, e, 12, b"\x60" + O.clear4(rng, 5, b"", 19)[1:])[0] == EINVAL
    assert O.check_encap(rng, e, 12, b"\x75" + O.clear4(rng, 5, b"", 30)[1:])[0] == EAFNOSUPPORT


def test_sa_flags_mlen_and_link_local_sa_addresses():
    rng = np.random.default_rng(7116)
    p4, p6 = O.clear4(rng, 5, b"", 40), O.clear6(rng, 40)
    ok = _sa(rng, False)
    assert O.check_encap(rng, ok, 12, p4)[0] == 0
    for bad in (ok.flags & ~L.ENC_AH, ok.flags | L.ENC_NATT, ok.flags | L.ENC_NATT | L.ENC_AF6, ok.flags | 0x400,
                ok.flags | 0x80000000, ok.flags | L.ENC_DF_SET | L.ENC_DF_COPY,
                ok.flags | L.ENC_ECN_ALLOWED | L.ENC_ECN_NOCARE):
        e = encsa(bad, 64, addr(rng, bool(bad & L.ENC_AF6)), addr(rng, bool(bad & L.ENC_AF6)))
        assert O.check_encap(rng, e, 12, p4, want=EINVAL)[0] == EINVAL, hex(bad)
    # an AH entry stays EINVAL for the ESP entry point, as before
    from encap_helpers import check_one
    assert check_one(rng, ok, 8, 4, 16, p4, want=EINVAL)[0] == EINVAL
    for mlen in (0, 2, 13, 18, 68, 0xffffffff):
        assert O.check_encap(rng, ok, mlen, p4)[0] == EINVAL, mlen
    for mlen in (4, 8, 64):
        assert O.check_encap(rng, ok, mlen, p4)[0] == 0, mlen
    for which in ("src", "dst"):
        for tunnel in (False, True):
            e = _sa(rng, True, tunnel=tunnel)
            getattr(e, which)[:2] = [0xfe, 0x80 | int(rng.integers(64))]
            assert O.check_encap(rng, e, 12, p6)[0] == ENOTSUP
    # null pointers
    lib = L.lib()
    import ctypes as C
    buf, r = (C.c_uint8 * 256)(), C.c_uint32()
    args = [C.byref(ok), 12, C.cast(buf, C.c_void_p), 60, 64, 1, C.cast(buf, C.c_void_p), C.byref(r), C.byref(r),
            C.byref(r)]
    for k in (0, 2, 6, 7, 8, 9):
        a = list(args)
        a[k] = None
        assert lib.espgpu_ah_encap(*a) == EINVAL, k


# ---- framing ----------------------------------------------------------------------
def _frame_one(rng, count, flags, salt=32, ln=80, spi=0xa1b2c3d4):
    o = L.OutSA(count, 0x1111222233334444, spi, 0x55667788, flags, 0x99aabbcc)
    pkt = rng.integers(0, 256, ln, dtype=np.uint8).tobytes()
    buf = bytearray(b"\xee" * 8 + pkt + b"\xee" * 8)
    st, hi = A.ah_frame_host(o, buf, 8, ln, salt, esn_hi=0x5a5a5a5a)
    wst, wpk, whi, wstate = A.ah_output_seq(E.OutState(count, 0, flags), spi, list(pkt), salt)
    assert st == wst, (st, wst, hex(count), hex(flags))
    assert (o.cntr, o.spi, o.salt, o.flags, o.pad_) == (0x1111222233334444, spi, 0x55667788, flags, 0x99aabbcc)
    if st:
        assert hi == 0x5a5a5a5a and o.count == count and bytes(buf) == b"\xee" * 8 + pkt + b"\xee" * 8
    else:
        assert hi == whi and o.count == wstate.count and bytes(buf) == b"\xee" * 8 + bytes(wpk) + b"\xee" * 8
        assert bytes(buf[8 + salt - 8:8 + salt]) == struct.pack(">II", spi, o.count & 0xffffffff)
    return st, hi, o.count


def test_frame_numbers_esn_cycseq_and_the_wrap():
    rng = np.random.default_rng(7120)
    E32, E64 = 2**32, 2**64
    for salt in (32, 36, 52, 72):
        assert _frame_one(rng, 7, 0, salt=salt) == (0, 0, 8)
    assert _frame_one(rng, 5 * E32 + 7, L.OUT_ESN) == (0, 5, 5 * E32 + 8)
    assert _frame_one(rng, 5 * E32 + 7, 0) == (0, 0, 5 * E32 + 8)
    # the end of the number space: always checked, with or without OUT_WRAPCHECK
    for wc in (0, L.OUT_WRAPCHECK):
        assert _frame_one(rng, E32 - 2, wc) == (0, 0, E32 - 1)
        assert _frame_one(rng, E32 - 1, wc)[0] == EACCES
        assert _frame_one(rng, 3 * E32 + E32 - 1, wc)[0] == EACCES           # the low word alone decides
        assert _frame_one(rng, E32 - 1, wc | L.OUT_ESN) == (0, 1, E32)
        assert _frame_one(rng, E64 - 2, wc | L.OUT_ESN) == (0, E32 - 1, E64 - 1)
        assert _frame_one(rng, E64 - 1, wc | L.OUT_ESN)[0] == EACCES
        assert _frame_one(rng, E64 - 1, wc)[0] == EACCES
        assert _frame_one(rng, E32 - 1, wc | L.OUT_CYCSEQ) == (0, 0, E32)
        assert _frame_one(rng, E64 - 1, wc | L.OUT_CYCSEQ | L.OUT_ESN) == (0, 0, 0)
    # the bits that mean nothing here
    assert _frame_one(rng, 9, L.OUT_CTRCOMPAT | L.OUT_PAD_SEQ | L.OUT_PAD_ZERO | L.OUT_PAD_RAND) == (0, 0, 10)


def test_frame_refuses_records_that_take_no_part():
    rng = np.random.default_rng(7121)
    for salt, ln in ((8, 80), (0, 80), (34, 80), (84, 80), (32, 0), (12, 11)):
        o = L.OutSA(7, 1, 2, 3, 0, 4)
        buf = bytearray(rng.integers(0, 256, 100, dtype=np.uint8).tobytes())
        before = bytes(buf)
        assert A.ah_frame_host(o, buf, 4, ln, salt, esn_hi=77) == (EINVAL, 77)
        assert bytes(buf) == before and o.count == 7
    o = L.OutSA(7, 1, 2, 3, 0, 4)
    buf = bytearray(16)
    assert A.ah_frame_host(o, buf, 0, 12, 12) == (0, 0) and bytes(buf[4:12]) == struct.pack(">II", 2, 8)
    assert A.ah_frame_host(o, buf, 0, 16, 16) == (0, 0) and bytes(buf[8:16]) == struct.pack(">II", 2, 9)


# ---- sent -------------------------------------------------------------------------
def test_sent_restores_the_wire_header_and_books():
    rng = np.random.default_rng(7122)
    for saf6, v6, tunnel in ((False, False, False), (False, False, True), (True, True, False), (True, False, True),
                             (False, True, True)):
        pdst = addr(rng, v6)
        e = _sa(rng, saf6, dst=pdst if saf6 == v6 else None, tunnel=tunnel)
        e.bytes, e.packets = 2**32 - 10, 2**32 - 1
        opts = O.sr_option(rng, 0x83, 7) + bytes([1])
        p = O.clear6(rng, 33, dst=pdst) if v6 else O.clear4(rng, 7, opts, 33, dst=pdst)
        st, front, hashed, slot, hs = O.check_encap(rng, e, 16, p)
        assert st == 0 and hashed[:hs] != slot[:hs]
        total = len(hashed)
        for status in (0, 13, 22, 74):
            buf = bytearray(b"\xee" * 4 + hashed + b"\xee" * 4)
            b0, p0 = e.bytes, e.packets
            assert A.ah_sent_host(e, status, buf, 4, total, hs + 12, bytearray(slot)) == 0
            if status:
                assert bytes(buf) == b"\xee" * 4 + hashed + b"\xee" * 4 and (e.bytes, e.packets) == (b0, p0)
            else:
                want = A.ah_output_cb(list(hashed), slot[:hs])
                assert bytes(buf) == b"\xee" * 4 + bytes(want) + b"\xee" * 4
                assert bytes(buf[4:4 + hs]) == slot[:hs] and (e.bytes, e.packets) == (b0 + total, p0 + 1)
        # a slot of the other version, an impossible salt: EINVAL, written nowhere, booked nowhere
        bad = bytearray(slot)
        bad[0] ^= 0x20
        for s, salt in ((bad, hs + 12), (slot, 28), (slot, hs + 14), (slot, 76), (slot, total + 4)) + \
                (((slot, 36),) if saf6 else ()):
            buf = bytearray(hashed)
            b0, p0 = e.bytes, e.packets
            assert A.ah_sent_host(e, 0, buf, 0, total, salt, bytearray(s)) == EINVAL, salt
            assert bytes(buf) == hashed and (e.bytes, e.packets) == (b0, p0)
        # an ESP SA's entry: passed over
        x = encsa(e.flags & ~L.ENC_AH, 64, bytes(e.src), bytes(e.dst), 5, 6)
        buf = bytearray(hashed)
        assert A.ah_sent_host(x, 0, buf, 0, total, hs + 12, bytearray(slot)) == 0
        assert bytes(buf) == hashed and (x.bytes, x.packets) == (5, 6)


def test_outbound_then_inbound_gives_the_packet_back():
    """The host rules alone, with hashlib's HMAC: encap, frame, sign, restore,
    then the inbound rules on the wire packet."""
    import hashlib
    import hmac as pyhmac
    rng = np.random.default_rng(7123)
    key = rng.integers(0, 256, 32, dtype=np.uint8).tobytes()
    for saf6, v6, tunnel in ((False, False, False), (False, False, True), (True, True, False), (True, True, True)):
        pdst = addr(rng, v6)
        e = _sa(rng, saf6, dst=pdst, tunnel=tunnel)
        opts = bytes([0x94, 4, 0, 0, 0x44, 8, 5, 0, 1, 2, 3, 4])     # router alert kept, timestamp zeroed
        p = O.clear6(rng, 33, dst=pdst) if v6 else O.clear4(rng, 8, opts, 33, dst=pdst)
        st, front, hashed, slot, hs = O.check_encap(rng, e, 16, p)
        buf = bytearray(hashed)
        o = L.OutSA(41, 0, 0x01020304, 0, 0, 0)
        assert A.ah_frame_host(o, buf, 0, len(buf), hs + 12) == (0, 0)
        buf[hs + 12:hs + 28] = bytes(16)
        buf[hs + 12:hs + 28] = pyhmac.new(key, bytes(buf), hashlib.sha256).digest()[:16]
        assert A.ah_sent_host(e, 0, buf, 0, len(buf), hs + 12, bytearray(slot)) == 0
        wire = bytes(buf)
        # inbound
        ins = L.InSA(0, 0, H.ah_flags(E.IPSEC_MODE_TUNNEL if tunnel else E.IPSEC_MODE_TRANSPORT, saf6), 0)
        rbuf, rslot = bytearray(wire), bytearray(64)
        assert A.ah_input_host(ins, 16, rbuf, len(rbuf), hs + 12, rslot) == 0
        icv = bytes(rbuf[hs + 12:hs + 28])
        rbuf[hs + 12:hs + 28] = bytes(16)
        assert pyhmac.new(key, bytes(rbuf), hashlib.sha256).digest()[:16] == icv
        rc, off, ln = A.ah_decap_host(ins, 16, rbuf, len(rbuf), hs + 12, rslot)
        assert rc == 0 and bytes(rbuf[off:off + ln]) == p
