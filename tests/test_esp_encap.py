"""espgpu_esp_encap and espgpu_esp_sent, the host rules of the outbound
encapsulation (csrc/encap.h), against esp.ipsec_output_encap, the restatement
of ipsec4/6_perform_request, ipsec_encap, esp_output's header work and
ipsec_process_done.  Every packet sits in a buffer with guard bytes and, where
the test does not set them, exactly the rooms it needs; the whole buffer is
compared, so a byte written outside the named header bytes fails the test."""
import struct

import numpy as np
import pytest

from decap_helpers import trailer_of
from encap_helpers import (ALENS, EAFNOSUPPORT, EINVAL, EMSGSIZE, ENOBUFS, ENOTSUP, IVLENS, ROOM, addr, check_one,
                           enc_flags, encsa, inner4, inner6, reference)
from espgpu import _lib as L
from espgpu import esp as E
from frame_helpers import sa_kinds
from helpers import EtaSA, GcmSA


def _sa(rng, saf6, flags_kw=None, dst=None, **kw):
    return encsa(enc_flags(af6=saf6, **(flags_kw or {})), int(rng.integers(1, 256)), addr(rng, saf6),
                 dst or addr(rng, saf6), **kw)


def _pkt(rng, v6, plen, dst=None, ihl=5, **kw):
    return inner6(rng, plen, dst=dst, **kw) if v6 else inner4(rng, ihl, plen, dst=dst, **kw)


@pytest.mark.parametrize("saf6", [False, True], ids=["sa4", "sa6"])
@pytest.mark.parametrize("v6", [False, True], ids=["pkt4", "pkt6"])
def test_families_modes_proxy_and_shapes(saf6, v6):
    """SA family x packet family x mode x (SA dst = packet dst, another, or
    unspecified) over every ip_hl, every shape and 36 consecutive payload
    lengths: both results of the decision occur in every cell that allows
    them, and every padding."""
    rng = np.random.default_rng(41 + 2 * saf6 + v6)
    seen, pads = set(), set()
    rl0 = 0
    for tunnel in (False, True):
        for proxy in ("same", "other", "any"):
            for ivlen in IVLENS:
                for blks in (4, 16):
                    for alen in ALENS:
                        ihl = int(rng.integers(5, 16))
                        for plen in range(rl0, rl0 + 36, 5 if (alen != 16) else 1):
                            pdst = addr(rng, v6)
                            sdst = {"same": pdst if saf6 == v6 else addr(rng, saf6), "other": addr(rng, saf6),
                                    "any": bytes(16 if saf6 else 4)}[proxy]
                            if proxy == "any" and saf6:
                                continue                             # unspecified: refused, below
                            e = _sa(rng, saf6, dict(tunnel=tunnel), dst=sdst)
                            if proxy == "any":
                                e.src[:] = [0] * 16
                            p = _pkt(rng, v6, plen, dst=pdst, ihl=ihl)
                            st, front, wire = check_one(rng, e, ivlen, blks, alen, p, ip_id=int(rng.integers(65536)))
                            if proxy == "any" and (tunnel or v6):
                                assert st == EINVAL                  # ipsec_output.c:938-941
                                continue
                            assert st == 0
                            encap = front > 8 + ivlen
                            assert encap == (tunnel or saf6 != v6 or proxy == "other")
                            seen.add((tunnel, proxy, encap))
                            rlen = len(p) if encap else plen
                            pads.add(((blks - ((rlen + 2) % blks)) % blks, blks))
                            if encap and not saf6:
                                assert E.in_cksum(wire[:20]) == 0
                            if not encap and not v6:
                                assert E.in_cksum(wire[:ihl * 4]) == 0
                        rl0 = (rl0 + 7) % 23
    assert len(seen) == (5 if not saf6 and not v6 else 4), seen
    assert pads == {(k, 4) for k in range(4)} | {(k, 16) for k in range(16)}


def test_every_ip_hl_with_options_every_hlen():
    rng = np.random.default_rng(45)
    for ihl in range(5, 16):
        for ivlen in IVLENS:
            for tunnel in (False, True):
                for plen in (0, 1, 37):
                    pdst = addr(rng, False)
                    e = _sa(rng, False, dict(tunnel=tunnel), dst=pdst)
                    st, front, wire = check_one(rng, e, ivlen, 16 if ivlen == 16 else 4, 12,
                                                inner4(rng, ihl, plen, dst=pdst))
                    assert st == 0 and front == 8 + ivlen + (20 if tunnel else 0)
                    assert E.in_cksum(wire[:20 if tunnel else ihl * 4]) == 0
                    if tunnel:                                       # the inner header verifies too
                        assert E.in_cksum(wire[front:front + ihl * 4]) == 0


@pytest.mark.parametrize("v6", [False, True], ids=["inner4", "inner6"])
def test_df_policy_ecn_and_rfc6864(v6):
    rng = np.random.default_rng(46 + v6)
    for dfbit in (0, 1, 2):
        for idf in (False, True):
            for ecn in (0, 1, -1):
                for iecn in range(4):
                    for rfc in (False, True):
                        for saf6 in (False, True):
                            tos = int(rng.integers(64)) << 2 | iecn
                            e = _sa(rng, saf6, dict(tunnel=True, dfbit=dfbit, ecn=ecn, rfc6864=rfc))
                            p = inner6(rng, 33, tc=tos) if v6 else inner4(rng, 6, 33, df=idf, tos=tos)
                            st, front, wire = check_one(rng, e, 8, 4, 16, p, ip_id=0xbeef)
                            assert st == 0
                            otos = wire[1] if not saf6 else (struct.unpack(">I", wire[:4])[0] >> 20) & 0xff
                            assert otos >> 2 == tos >> 2
                            assert otos & 3 == {0: 0, 1: 2 if iecn == 3 else iecn, -1: iecn}[ecn]
                            if not saf6:
                                df = bool(wire[6] & 0x40)
                                assert df == {0: False, 1: True, 2: idf if not v6 else True}[dfbit]
                                assert wire[6] & 0xbf == 0 and wire[7] == 0
                                assert wire[4:6] == (b"\0\0" if rfc and df else b"\xbe\xef")
                                assert E.in_cksum(wire[:20]) == 0
                                assert wire[8] == e.ttl and wire[9] == 50
                            else:
                                assert wire[7] == e.ttl and wire[6] == 50


def test_header_sums_to_ffff_before_the_checksum():
    """The one's-complement sum of the header without the checksum is 0xffff:
    the field must end as 0x0000 (in_cksum's result), in a transport header,
    a tunnel's fixed inner header and its outer header."""
    rng = np.random.default_rng(48)
    for ihl in (5, 9, 15):
        pdst = addr(rng, False)
        e = _sa(rng, False, dst=pdst)
        plen = 51
        total = ihl * 4 + 16 + plen + ((4 - (plen + 2) % 4) % 4 + 2) + 12
        p = inner4(rng, ihl, plen, dst=pdst, fold_ffff=True, total=total)
        st, front, wire = check_one(rng, e, 8, 4, 12, p)
        assert st == 0 and len(wire) == total and wire[10:12] == b"\0\0" and E.in_cksum(wire[:ihl * 4]) == 0
    # tunnel: search the ip_id that makes the outer header fold, and an inner id likewise
    e = _sa(rng, False, dict(tunnel=True))
    p = bytearray(inner4(rng, 7, 40))
    t = bytearray(p[:28])
    t[2:4], t[10:12], t[4:6] = struct.pack(">H", len(p)), b"\0\0", b"\0\0"
    p[4:6] = struct.pack(">H", E.in_cksum(bytes(t)))
    st, front, wire0 = check_one(rng, e, 16, 16, 32, bytes(p), ip_id=0)
    assert st == 0 and wire0[front + 10:front + 12] == b"\0\0"
    ident = struct.unpack(">H", wire0[10:12])[0]          # the checksum with id 0 is the id that folds it
    st, front, wire = check_one(rng, e, 16, 16, 32, bytes(p), ip_id=ident)
    assert wire[4:6] == struct.pack(">H", ident) and wire[10:12] == b"\0\0" and E.in_cksum(wire[:20]) == 0


def test_flag_errors_and_sa_addresses():
    rng = np.random.default_rng(49)
    p4, p6 = inner4(rng, 5, 40), inner6(rng, 40)
    for bad in (0x80, 0x100, 1 << 31, L.ENC_DF_SET | L.ENC_DF_COPY, L.ENC_ECN_ALLOWED | L.ENC_ECN_NOCARE,
                0x0c | L.ENC_AF6, 0x30 | L.ENC_TUNNEL):
        for p in (p4, p6):
            saf6 = bool(bad & L.ENC_AF6)
            e = encsa(bad, 64, addr(rng, saf6), addr(rng, saf6))
            assert check_one(rng, e, 8, 4, 16, p, want=EINVAL)[0] == EINVAL
    for which in ("src", "dst"):
        # AF6: unspecified is refused whatever the mode, before the packet is looked at
        for tunnel in (False, True):
            e = _sa(rng, True, dict(tunnel=tunnel))
            getattr(e, which)[:] = [0] * 16
            for p in (p4, p6, b"\x40" * 8):
                assert check_one(rng, e, 8, 4, 16, p)[0] == EINVAL
            e = _sa(rng, True, dict(tunnel=tunnel))
            for hi in (0x80, 0xbf):
                getattr(e, which)[0:2] = [0xfe, hi]
                assert check_one(rng, e, 8, 4, 16, p6)[0] == ENOTSUP
            getattr(e, which)[0:2] = [0xfe, 0xc0]            # fec0::/10 is not link-local
            assert check_one(rng, e, 8, 4, 16, p6)[0] == 0
        # AF_INET: zero only matters where ipsec_encap runs
        e = _sa(rng, False, dst=p4[16:20])
        getattr(e, which)[:4] = [0] * 4
        assert check_one(rng, e, 8, 4, 16, p4)[0] == 0           # transport: dst any is the wildcard, src is not read
        e.flags |= L.ENC_TUNNEL
        assert check_one(rng, e, 8, 4, 16, p4)[0] == EINVAL
        e.flags &= ~L.ENC_TUNNEL
        assert check_one(rng, e, 8, 4, 16, p6)[0] == EINVAL      # family mismatch: encapsulated
    # an AF_INET address that starts fe 80 is nobody's link-local
    e = encsa(L.ENC_TUNNEL, 9, b"\xfe\x80\x01\x02", b"\xfe\x81\x01\x02")
    assert check_one(rng, e, 8, 4, 16, p4)[0] == 0


def test_versions_and_short_packets():
    rng = np.random.default_rng(50)
    for saf6 in (False, True):
        e = _sa(rng, saf6, dict(tunnel=True))
        for ver in (0, 5, 7, 15):
            p = bytearray(inner4(rng, 5, 30))
            p[0] = ver << 4 | 5
            assert check_one(rng, e, 8, 4, 16, bytes(p))[0] == EAFNOSUPPORT
        p4, p6 = inner4(rng, 5, 30), inner6(rng, 30)
        for n in (0, 1, 19):
            assert check_one(rng, e, 8, 4, 16, p4[:n])[0] == EINVAL
        assert check_one(rng, e, 8, 4, 16, p4[:20])[0] == 0
        for n in (20, 39):
            assert check_one(rng, e, 8, 4, 16, p6[:n])[0] == EINVAL
        assert check_one(rng, e, 8, 4, 16, p6[:40])[0] == 0
        for ihl in (0, 4):
            p = bytearray(p4)
            p[0] = 0x40 | ihl
            assert check_one(rng, e, 8, 4, 16, bytes(p))[0] == EINVAL
        p = inner4(rng, 12, 0)
        assert check_one(rng, e, 8, 4, 16, p)[0] == 0 and check_one(rng, e, 8, 4, 16, p[:47])[0] == EINVAL
    # null pointers and unusable shapes
    import ctypes as C
    lib = L.lib()
    e, buf, r = _sa(rng, False), (C.c_uint8 * 128)(), [C.c_uint32(7) for _ in range(4)]
    ok = [C.byref(e), C.byref(L.EShape(8, 4, 16)), C.cast(buf, C.c_void_p), 40, 32, 32, 1] + [C.byref(x) for x in r]
    for k in (0, 1, 2, 7, 8, 9, 10):
        a = list(ok)
        a[k] = None
        assert lib.espgpu_esp_encap(*a) == EINVAL
    for shape in ((4, 4, 16), (8, 0, 16), (8, 8, 16), (8, 4, 65536)):
        a = list(ok)
        a[1] = C.byref(L.EShape(*shape))
        assert lib.espgpu_esp_encap(*a) == EINVAL and [x.value for x in r] == [0, 0, 0, 0]
    assert lib.espgpu_esp_sent(None, 0, 5) == EINVAL


def test_total_at_the_limit():
    """total 65535 passes and 65536 is EMSGSIZE, for every way total is made.
    rlen + padding is a multiple of blks and the headers are multiples of 4,
    so the ICV length decides the last bytes: the same packet passes with alen
    and is refused with alen + 1, and one payload byte more is refused too.  A
    packet longer than 65535 is EMSGSIZE whatever it holds."""
    rng = np.random.default_rng(51)
    for saf6, v6, tunnel in ((False, False, False), (False, False, True), (True, True, False), (True, True, True),
                             (True, False, False), (False, True, False)):
        for ivlen, blks in ((8, 4), (16, 16), (0, 4), (8, 16)):
            encap = tunnel or saf6 != v6
            skip = 40 if v6 else 24
            fixed = ((40 if saf6 else 20) if encap else skip) + 8 + ivlen
            m = (65535 - fixed - 3) // blks * blks               # rlen + padding, with padding 2
            alen = 65535 - fixed - m
            assert 3 <= alen < 3 + blks
            q = m - 2 - (skip if encap else 0)
            pdst = addr(rng, v6)
            e = _sa(rng, saf6, dict(tunnel=tunnel), dst=pdst if saf6 == v6 else None)
            p = _pkt(rng, v6, q, dst=pdst, ihl=6)
            st, front, wire = check_one(rng, e, ivlen, blks, alen, p)
            assert st == 0 and len(wire) == 65535, (saf6, v6, tunnel, ivlen, blks)
            assert check_one(rng, e, ivlen, blks, alen + 1, p)[0] == EMSGSIZE
            p = _pkt(rng, v6, q + 1, dst=pdst, ihl=6)
            assert check_one(rng, e, ivlen, blks, alen, p)[0] == EMSGSIZE
    for n in (65536, 70000):
        assert check_one(rng, _sa(rng, False), 8, 4, 16, inner4(rng, 5, n - 20))[0] == EMSGSIZE
        assert check_one(rng, _sa(rng, True, dict(tunnel=True)), 8, 4, 16, inner6(rng, n - 40))[0] == EMSGSIZE


def test_rooms_exact_and_one_short():
    rng = np.random.default_rng(52)
    for saf6, v6, tunnel in ((False, False, False), (False, False, True), (True, True, True), (True, False, False),
                             (False, True, False), (True, True, False)):
        for ivlen, blks, alen in ((8, 4, 16), (16, 16, 32), (0, 4, 0), (16, 16, 0)):
            pdst = addr(rng, v6)
            e = _sa(rng, saf6, dict(tunnel=tunnel), dst=pdst if saf6 == v6 else None)
            p = _pkt(rng, v6, int(rng.integers(0, 90)), dst=pdst)
            st, front, wire, _ = reference(e, ivlen, blks, alen, p, 1 << 20, 1 << 20, 0)
            head, tail = front, len(wire) - front - len(p)
            assert st == 0 and head >= 8 and tail >= 2
            assert check_one(rng, e, ivlen, blks, alen, p, head, tail)[0] == 0
            assert check_one(rng, e, ivlen, blks, alen, p, head - 1, tail)[0] == ENOBUFS
            assert check_one(rng, e, ivlen, blks, alen, p, head, tail - 1)[0] == ENOBUFS
            assert check_one(rng, e, ivlen, blks, alen, p, 0, 0)[0] == ENOBUFS
            assert check_one(rng, e, ivlen, blks, alen, p, *ROOM)[0] == 0


def _kinds(rng):
    """Every session kind the oracle serves."""
    return [sa for _, sa, _ in sa_kinds(rng)] + [GcmSA(rng, mlen=12), EtaSA(rng, sha=384), EtaSA(rng, sha=512),
                                                 EtaSA(rng, null=True, sha=512), EtaSA(rng, esn=True),
                                                 GcmSA(rng, esn=True)]


@pytest.mark.parametrize("tunnel", [False, True], ids=["transport", "tunnel"])
@pytest.mark.parametrize("v6", [False, True], ids=["v4", "v6"])
def test_round_trip_through_the_oracle(tunnel, v6):
    """host encap -> espgpu_esp_frame -> the oracle's encrypt -> its decrypt
    -> the trailer word -> espgpu_esp_decap gives the original packet back,
    with ip_len and ip_sum (ip6_plen) as the reference leaves them."""
    rng = np.random.default_rng(53 + 2 * tunnel + v6)
    for sa in _kinds(rng):
        esa = sa.esp_sa()
        shape = E.esp_frame_shape(esa, L.OUT_PAD_SEQ)
        ivlen, blks, alen = shape.ivlen, shape.blks, shape.alen
        for plen in (0, 1, 13, 64, 255):
            pdst = addr(rng, v6)
            e = _sa(rng, v6, dict(tunnel=tunnel), dst=pdst)
            ihl = int(rng.integers(5, 16))
            p = _pkt(rng, v6, plen, dst=pdst, ihl=ihl)
            head, tail = ROOM
            buf = bytearray(rng.integers(0, 256, head, dtype=np.uint8).tobytes() + p +
                            rng.integers(0, 256, tail, dtype=np.uint8).tobytes())
            st, front, total, reclen, frame = E.esp_encap_host(e, shape, buf, head, len(p), head, tail, 77)
            assert st == 0
            hlen = 8 + ivlen
            skip = total - reclen
            assert skip == (front - hlen if tunnel else (40 if v6 else ihl * 4))
            w0 = head - front
            rec = bytearray(buf[w0 + skip:w0 + total])
            outsa = L.OutSA(41, 9000, sa.spi, int.from_bytes(esa.salt, "little"), L.OUT_PAD_SEQ, 0)
            rc, esn_hi = E.esp_frame_host(outsa, shape, rec, frame & 0xffff, frame >> 16)
            assert rc == 0
            wire = bytearray(buf[w0:w0 + skip]) + rec
            assert len(wire) == total
            rc, ct = sa.oracle.esp_encrypt(bytes(rec), esn_hi)
            assert rc == 0
            rlen = frame & 0xffff
            assert esa.null or rlen < 8 or ct[hlen:hlen + rlen] != bytes(rec[hlen:hlen + rlen])
            rc, dec = sa.oracle.esp_decrypt(ct, esn_hi)
            assert rc == 0
            pt = bytes(wire[:skip]) + dec
            tr = trailer_of(pt, skip, reclen, ivlen, alen)
            insa = L.InSA(0, 0, (L.IN_TUNNEL if tunnel else L.IN_TRANSPORT) | (L.IN_AF6 if v6 else 0), 0)
            got = bytearray(pt)
            st, off, ln = E.esp_decap_host(insa, L.EShape(ivlen, blks, alen), got, skip, reclen, tr)
            assert st == 0
            back = bytes(got[off:off + ln])
            want = bytearray(p)
            if v6:
                want[4:6] = struct.pack(">H", len(p) - 40)               # ipsec_output.c:533 / ipsec_input.c:532
            else:
                want[2:4] = struct.pack(">H", len(p))                    # :230 / ipsec_input.c:312
                want[10:12] = b"\0\0"
                want[10:12] = struct.pack(">H", E.in_cksum(bytes(want[:ihl * 4])))
            assert back == bytes(want), (sa.esp_sa().alg, plen)


def test_sent_counters():
    e = encsa(L.ENC_TUNNEL, 64, b"\x0a\0\0\1", b"\x0a\0\0\2", bytes0=2**64 - 100, packets0=2**32 - 1)
    before = bytes(e)[16:]
    assert E.esp_sent_host(e, 0, 60) == 0 and (e.bytes, e.packets) == (2**64 - 40, 2**32)
    assert E.esp_sent_host(e, 0, 65535) == 0 and (e.bytes, e.packets) == (65535 - 40, 2**32 + 1)   # wraps
    for st in (EINVAL, 74, 1, 255):
        assert E.esp_sent_host(e, st, 1500) == 0 and (e.bytes, e.packets) == (65535 - 40, 2**32 + 1)
    assert E.esp_sent_host(e, 0, 0) == 0 and (e.bytes, e.packets) == (65535 - 40, 2**32 + 2)
    assert bytes(e)[16:] == before
