"""NAT-T (ESP in UDP) on the host: espgpu_sad_build's flag, the classification,
decapsulation and encapsulation rules with it, espgpu_esp_sent's booking and
espgpu_esp_natt_cksum (csrc/classify.h, decap.h, encap.h, natt.h), against
esp.py's restatements of udp_input, udp_ipsec_input, udp_ipsec_output,
udp_ipsec_adjust_cksum and in_delayed_cksum.  Every packet sits in a buffer
with guard bytes and the whole buffer is compared."""
import struct

import numpy as np
import pytest

import classify_helpers as CH
import decap_helpers as DH
import encap_helpers as EH
import natt_helpers as NH
from espgpu import _lib as L
from espgpu import esp as E
from espgpu.batch import SAD_DTYPE, sad_build

EINVAL, ENOTSUP, ENOENT = L.EINVAL, L.ENOTSUP, L.ENOENT
PORT = NH.PORT


def test_header_and_library_say_natt_is_built():
    src = open(L.HEADER).read()
    assert "#define ESPGPU_HAS_NATT 1" in src and "#define ESPGPU_ABI_VERSION 6" in src
    assert {"espgpu_esp_natt_cksum", "espgpu_esp_natt_cksum_batch"} <= set(L.header_symbols())
    assert hasattr(L.lib(), "espgpu_esp_natt_cksum_batch") and L.lib().espgpu_abi_version() == 6


# ---- the SA table ---------------------------------------------------------------
def _entry(spi=0x1000, sa=1, proto=50, af=4, dst=None, flags=0):
    e = np.zeros(1, dtype=SAD_DTYPE)[0]
    e["spi"], e["sa"], e["proto"], e["af"], e["flags"] = spi, sa, proto, af, flags
    e["dst"] = dst if dst is not None else ([10, 1, 2, 3] + [0] * 12 if af == 4 else list(range(0x20, 0x30)))
    return e


def test_sad_build_takes_the_natt_flag_only_where_the_reference_has_natt():
    ports = [10, 1, 2, 3, 0x11, 0x94, 0x11, 0x95] + [0] * 8
    t = sad_build(np.array([_entry(flags=L.SAD_NATT, dst=ports)]), 4)
    slot = [s for s in t if s["spi"] == 0x1000][0]
    assert slot["flags"] == L.SAD_NATT and list(slot["dst"]) == ports
    sad_build(np.array([_entry(flags=L.SAD_NATT)]), 4)               # ports 0: nothing forbids them
    for bad in (_entry(flags=1), _entry(flags=3), _entry(flags=4), _entry(flags=L.SAD_NATT | 0x10),
                _entry(flags=0x80000000), _entry(flags=L.SAD_NATT, af=6), _entry(flags=L.SAD_NATT, proto=51),
                _entry(flags=L.SAD_NATT, dst=ports[:8] + [0] * 7 + [1]),
                _entry(flags=L.SAD_NATT, dst=ports[:8] + [1] + [0] * 7),
                _entry(flags=0, dst=ports)):                          # without the flag: today's rule
        with pytest.raises(ValueError):
            sad_build(np.array([bad]), 4)


# ---- classification -------------------------------------------------------------
@pytest.fixture(scope="module")
def db():
    rng = np.random.default_rng(1201)
    d = NH.NattSadb(rng)
    return d, sad_build(d.entries, 128)


def _both(db, pkt, port, off4=77, ipcsum=False):
    d, table = db
    flags = L.CLS_NATT_PORT(port) | (L.CLS_IPCSUM if ipcsum else 0)
    got = E.esp_classify_host(table, pkt, off4, flags)
    want = E.ipsec_input_classify_natt(d.ref, pkt, off4, ipcsum, port)
    assert got == want, (got, want, pkt[:40].hex())
    return got


def test_every_classification_row_in_order(db):
    """One packet per row of the header's 2a, each built from a packet the row
    before accepts; host rule == restatement == the row's status."""
    rng = np.random.default_rng(1202)
    for rep in range(40):
        for kind, st in NH.NATT_KINDS.items():
            p = NH.natt_packet(rng, db[0], PORT, kind)
            got = _both(db, p, PORT, ipcsum=bool(rep & 1))
            assert got[0] == st, (kind, got)
            if st == 0:
                hlen = (p[0] & 0xf) * 4
                ulen = struct.unpack(">H", p[hlen + 4:hlen + 6])[0]
                spi = struct.unpack(">I", p[hlen + 8:hlen + 12])[0]
                assert got[1] == (77 + (hlen + 8) // 4, ulen - 8, db[0].ref[spi][0], 0, db[0].ref[spi][4]), kind
            else:
                assert got[1] == (77, 0, 0xffff, 0, 0)
            # port 0 is today's rule: every UDP packet is the host's
            off = _both(db, p, 0)
            assert off[0] == (ENOTSUP if p[9] == 17 else st), kind


def test_check_order_first_check_decides(db):
    """Two faults in one packet: the earlier row's status comes out."""
    rng = np.random.default_rng(1203)
    d = db[0]
    e = NH._port_entry(rng, d, PORT)
    sport, dport = NH.ports_of(e)
    dst = CH.dst_of(e)
    good = CH.esp_payload(rng, int(e["spi"]), 24)
    cases = [
        (NH.udp4(dst, sport, dport ^ 1, good, ulen=3), ENOTSUP),                 # port before uh_ulen
        (NH.udp4(dst, sport, dport, good, ulen=40, uh_sum=5), EINVAL),           # uh_ulen before uh_sum
        (NH.udp4(dst, sport, dport, b"\xff", uh_sum=5), ENOTSUP),                # uh_sum before the keepalive
        (NH.udp4(dst, sport, dport, bytes(4) + good[4:] + b"\0"), ENOTSUP),      # SPI 0 before the alignment
        (NH.udp4(dst, sport, dport, CH.esp_payload(rng, d.unknown_spi(rng), 25)), EINVAL),   # alignment before the lookup
        (NH.udp4(dst, sport ^ 1, dport, CH.esp_payload(rng, d.unknown_spi(rng), 24)), ENOENT),
    ]
    for p, st in cases:
        assert _both(db, p, PORT)[0] == st
    # a plain SA's packet and the existing kinds are untouched by the port
    for kind, (build, _) in CH.KINDS.items():
        for _ in range(6):
            p = build(rng, d)
            a, b = _both(db, p, PORT), _both(db, p, 0)
            assert a == b, kind


def test_classify_reads_nothing_past_udp_header_and_spi(db):
    rng = np.random.default_rng(1204)
    p = bytearray(NH.natt_packet(rng, db[0], PORT, "good"))
    hlen = (p[0] & 0xf) * 4
    want = _both(db, bytes(p), PORT)
    p[hlen + 12:] = bytes(len(p) - hlen - 12)
    assert _both(db, bytes(p), PORT) == want and want[0] == 0


# ---- decapsulation ----------------------------------------------------------------
def _check_decap(rng, flags, ivlen, alen, pkt, skip, rlen, want=None, bytes0=5, packets0=7):
    trailer = DH.trailer_of(pkt, skip, rlen, ivlen, alen)
    G = DH.GUARD
    buf = bytearray(rng.integers(0, 256, G, dtype=np.uint8).tobytes() + pkt +
                    rng.integers(0, 256, G, dtype=np.uint8).tobytes())
    before = bytes(buf)
    insa = L.InSA(bytes0, packets0, flags, 0x1234)
    st, off, ln = E.esp_decap_host(insa, DH.shape_of(ivlen, alen), buf, skip, rlen, trailer, at=G)
    if want is None:
        mode, _, prand = DH.flags_mode(flags & ~L.IN_NATT)
        want, res, booked = E.esp_input_decap_natt(mode, prand, ivlen, alen, pkt[:skip + rlen], skip)
    else:
        res, booked = None, 0
    ctx = (hex(flags), ivlen, alen, skip, rlen)
    assert st == want, (st, want) + ctx
    assert (insa.flags, insa.pad_) == (flags, 0x1234)
    if st:
        assert (off, ln) == (0, 0) and bytes(buf) == before and (insa.bytes, insa.packets) == (bytes0, packets0), ctx
        return st, None
    assert ln == len(res) == booked, (ln, len(res), booked) + ctx
    a = G + off
    assert bytes(buf[a:a + ln]) == res, ctx
    assert bytes(buf[:a]) == before[:a] and bytes(buf[a + ln:]) == before[a + ln:], ("outside the result",) + ctx
    assert (insa.bytes, insa.packets) == (bytes0 + booked, packets0 + 1), ctx
    return 0, (off, ln)


def test_decap_every_ip_hl_ivlen_and_mode():
    rng = np.random.default_rng(1210)
    kinds = set()
    for ihl in range(5, 16):
        for ivlen in DH.IVLENS:
            for mode in DH.MODES:
                for nxt in (6, 17, 4, 41, 50):
                    for q in (0, 20, 40, 57):
                        alen = int(rng.choice(DH.ALENS))
                        pkt, skip, rlen = NH.natt_in_packet(rng, ivlen, alen, q, nxt, ihl=ihl)
                        st, r = _check_decap(rng, NH.in_flags(mode), ivlen, alen, pkt, skip, rlen)
                        hlen = 8 + ivlen
                        if st == 0:
                            tunnel = r[0] == skip + hlen
                            assert r == ((skip + hlen, q) if tunnel else (hlen + 8, skip - 8 + q))
                            kinds.add((mode, "tunnel" if tunnel else "transport"))
                        else:
                            kinds.add((mode, st))
    assert {(m, k) for m in DH.MODES for k in ("tunnel", "transport")} - kinds == {
        (E.IPSEC_MODE_TRANSPORT, "tunnel"), (E.IPSEC_MODE_TUNNEL, "transport")}, kinds
    assert (E.IPSEC_MODE_TUNNEL, L.EPFNOSUPPORT) in kinds


def test_decap_refusals_of_the_flag():
    rng = np.random.default_rng(1211)
    pkt, skip, rlen = NH.natt_in_packet(rng, 8, 16, 40, 6, ihl=6)
    f = NH.in_flags(E.IPSEC_MODE_TRANSPORT)
    assert _check_decap(rng, f, 8, 16, pkt, skip, rlen)[0] == 0
    assert _check_decap(rng, f | L.IN_AF6, 8, 16, pkt, skip, rlen, want=EINVAL)[0] == EINVAL
    for bad in (0x10, 0x40, 0x100, 0x80000000):
        assert _check_decap(rng, f | bad, 8, 16, pkt, skip, rlen, want=EINVAL)[0] == EINVAL
    # skip 20 and 24 are legal without the flag and too short with it; 64 and 68 the other way round
    body = DH.record(rng, 8, 16, 40, 3, 6)
    for s, natt_ok, plain_ok in ((20, False, True), (24, False, True), (28, True, True), (60, True, True),
                                 (64, True, False), (68, True, False), (72, False, False), (30, False, False)):
        for natt, ok in ((True, natt_ok), (False, plain_ok)):
            hl = s - 8 if natt else s
            if ok:
                hdr = DH.outer4(rng, hl // 4, s + len(body), proto=17 if natt else 50) + (bytes(8) if natt else b"")
            else:
                hdr = (DH.outer4(rng, 5, s + len(body)) + bytes(64))[:s]
            fl = f if natt else f & ~L.IN_NATT
            if natt:
                st, _ = _check_decap(rng, fl, 8, 16, hdr + body, s, len(body), want=None if ok else EINVAL)
            else:
                st = DH.check_one(rng, fl, 8, 16, hdr + body, s, len(body), want=None if ok else EINVAL)
            assert (st == 0) == ok, (s, natt, st)
    # ip_hl that does not agree with skip - 8
    p = bytearray(pkt)
    p[0] = 0x45
    assert _check_decap(rng, f, 8, 16, bytes(p), skip, rlen)[0] == EINVAL


# ---- encapsulation ------------------------------------------------------------------
def _natt_sa(rng, tunnel, sport=0x1194, dport=0x1195, dst=None, **kw):
    e = EH.encsa(EH.enc_flags(tunnel=tunnel, **kw) | L.ENC_NATT, int(rng.integers(1, 256)), EH.addr(rng, False),
                 dst or EH.addr(rng, False))
    e.dst[4:8] = list(struct.pack(">HH", sport, dport))
    return e


def _reference(e, ivlen, blks, alen, pkt, headroom, tailroom, ip_id):
    tunnel, af6, dfbit, ecn, rfc = EH.flags_policy(e.flags)
    sport, dport = struct.unpack(">HH", bytes(e.dst[4:8]))
    return E.ipsec_output_encap_natt(tunnel, af6, bytes(e.src), bytes(e.dst), e.ttl, dfbit, ecn, rfc, ivlen, blks,
                                     alen, pkt, headroom, tailroom, ip_id, sport, dport)


def _check_encap(rng, e, ivlen, blks, alen, pkt, headroom=None, tailroom=None, ip_id=0x4321, want=None):
    """EH.check_one with the NAT-T restatement as the reference."""
    pkt = bytes(pkt)
    if want is None and (headroom is None or tailroom is None):
        st0, front0, wire0, _ = _reference(e, ivlen, blks, alen, pkt, 1 << 20, 1 << 20, ip_id)
        need = (front0, len(wire0) - front0 - len(pkt)) if st0 == 0 else (EH.ROOM[0] + 8, EH.ROOM[1])
        headroom = need[0] if headroom is None else headroom
        tailroom = need[1] if tailroom is None else tailroom
    elif headroom is None:
        headroom, tailroom = EH.ROOM[0] + 8, EH.ROOM[1]
    at = EH.GUARD + headroom
    buf = bytearray(rng.integers(0, 256, at, dtype=np.uint8).tobytes() + pkt +
                    rng.integers(0, 256, tailroom + EH.GUARD, dtype=np.uint8).tobytes())
    before, sa0 = bytes(buf), bytes(e)
    st, front, total, reclen, frame = E.esp_encap_host(e, L.EShape(ivlen, blks, alen), buf, at, len(pkt), headroom,
                                                       tailroom, ip_id)
    ctx = (hex(e.flags), ivlen, blks, alen, len(pkt), headroom, tailroom)
    assert bytes(e) == sa0
    if want is None:
        want, wfront, wire, nxt = _reference(e, ivlen, blks, alen, pkt, headroom, tailroom, ip_id)
    assert st == want, (st, want) + ctx
    if st:
        assert (front, total, reclen, frame) == (0, 0, 0, 0) and bytes(buf) == before, ctx
        return st, 0, None
    assert (front, total) == (wfront, len(wire)), (front, total, wfront, len(wire)) + ctx
    hlen, rlen = 8 + ivlen, frame & 0xffff
    assert frame >> 16 == nxt, ctx
    assert reclen == hlen + rlen + ((blks - ((rlen + 2) % blks)) % blks) + 2 + alen, ctx
    exp = bytearray(before)
    for k, b in enumerate(wire):
        if b is not None:
            exp[at - front + k] = b
    # the record is the wire packet's last reclen bytes, where the restatement left the ESP header open
    assert wire[total - reclen] is None and wire[total - reclen - 1] is not None, ctx
    if bytes(buf) != bytes(exp):
        bad = [k - at for k in range(len(buf)) if buf[k] != exp[k]]
        raise AssertionError(("bytes differ at (relative to the packet)", bad[:16]) + ctx)
    return 0, front, bytes(buf[at - front:at - front + total])


def test_encap_modes_families_and_every_ip_hl():
    rng = np.random.default_rng(1220)
    seen = set()
    for tunnel in (False, True):
        for v6 in (False, True):
            for ihl in range(5, 16):
                for ivlen in EH.IVLENS:
                    blks, alen = (16 if ivlen == 16 else 4), int(rng.choice(EH.ALENS))
                    plen = int(rng.integers(0, 90))
                    pdst = EH.addr(rng, v6)
                    e = _natt_sa(rng, tunnel, dst=None if (tunnel or v6) else pdst, dfbit=int(rng.integers(3)),
                                 ecn=int(rng.integers(-1, 2)))
                    p = EH.inner6(rng, plen, dst=pdst) if v6 else EH.inner4(rng, ihl, plen, dst=pdst)
                    st, front, wire = _check_encap(rng, e, ivlen, blks, alen, p)
                    assert st == 0
                    encap = tunnel or v6
                    oh = 20 if encap else 0
                    assert front == 8 + ivlen + oh + 8
                    hl = 20 if encap else ihl * 4
                    assert wire[9] == 17 and E.in_cksum(wire[:hl]) == 0
                    assert struct.unpack(">HHHH", wire[hl:hl + 8]) == (0x1194, 0x1195, len(wire) - hl, 0)
                    assert struct.unpack(">H", wire[2:4])[0] == len(wire)
                    seen.add((tunnel, v6))
                    # headroom exactly enough (above) and one byte short
                    assert _check_encap(rng, e, ivlen, blks, alen, p, headroom=front - 1,
                                        tailroom=EH.ROOM[1])[0] == L.ENOBUFS
    assert len(seen) == 4


def test_encap_total_limit_and_flag_refusals():
    rng = np.random.default_rng(1221)
    # transport, ivlen 8, blks 4, 65470 payload bytes: total = 20 + 16 + 65472 + alen.  Real shapes give
    # multiples of 4; the host rule takes any alen, which reaches both sides of the limit exactly
    for alen, want_total, st in ((19, 65527, 0), (20, 65528, L.EMSGSIZE)):
        e = _natt_sa(rng, False)
        p = EH.inner4(rng, 5, 65470, dst=bytes(e.dst[:4]))
        st0, _, wire0, _ = E.ipsec_output_encap(False, False, bytes(e.src), bytes(e.dst), e.ttl, 0, 0, False, 8, 4,
                                                alen, p, 1 << 20, 1 << 20, 0)
        assert st0 == 0 and len(wire0) == want_total
        got = _check_encap(rng, e, 8, 4, alen, p)
        assert got[0] == st and (st or len(got[2]) == 65535)
    # and in tunnel mode: total = 20 + 16 + (20 + 65448 + 4) + alen
    for alen, st in ((19, 0), (20, L.EMSGSIZE)):
        got = _check_encap(rng, _natt_sa(rng, True), 8, 4, alen, EH.inner4(rng, 5, 65448))
        assert got[0] == st and (st or len(got[2]) == 65535)
    p = EH.inner4(rng, 5, 40)
    e = _natt_sa(rng, True)
    e.flags |= L.ENC_AF6
    assert _check_encap(rng, e, 8, 4, 16, p)[0] == L.EAFNOSUPPORT
    for k in list(range(4, 16)):
        e = _natt_sa(rng, True)
        e.src[k] = 1
        assert _check_encap(rng, e, 8, 4, 16, p, want=EINVAL)[0] == EINVAL
    for k in range(8, 16):
        e = _natt_sa(rng, True)
        e.dst[k] = 1
        assert _check_encap(rng, e, 8, 4, 16, p, want=EINVAL)[0] == EINVAL
    for bad in (0x80, 0x100, 0x400, 1 << 31):
        e = _natt_sa(rng, True)
        e.flags |= bad
        assert _check_encap(rng, e, 8, 4, 16, p, want=EINVAL)[0] == EINVAL


def test_sent_books_the_packet_without_its_udp_header():
    rng = np.random.default_rng(1222)
    e = _natt_sa(rng, True)
    e.bytes, e.packets = 1000, 10
    assert E.esp_sent_host(e, 0, 156) == 0 and (e.bytes, e.packets) == (1148, 11)
    assert E.esp_sent_host(e, 22, 156) == 0 and (e.bytes, e.packets) == (1148, 11)
    plain = EH.encsa(EH.enc_flags(tunnel=True), 64, EH.addr(rng, False), EH.addr(rng, False))
    assert E.esp_sent_host(plain, 0, 156) == 0 and (plain.bytes, plain.packets) == (156, 1)


# ---- the checksum fix -----------------------------------------------------------------
def _check_cksum(rng, pkt, proto, policy, delta, natt=True):
    """One packet through espgpu_esp_natt_cksum against the restatement:
    cflags and the whole buffer.  Returns (packet after, cflags)."""
    G = 16
    buf = bytearray(rng.integers(0, 256, G, dtype=np.uint8).tobytes() + pkt +
                    rng.integers(0, 256, G, dtype=np.uint8).tobytes())
    before = bytes(buf)
    insa = L.InSA(3, 4, L.IN_TRANSPORT | (L.IN_NATT if natt else 0), delta | 0xabcd0000)
    rc, cf = E.esp_natt_cksum_host(insa, buf, G, len(pkt), L.TR_VALID | 0x300 | proto, policy)
    assert rc == 0 and (insa.bytes, insa.packets, insa.pad_) == (3, 4, delta | 0xabcd0000)
    if natt and proto in (6, 17):
        want, valid = E.udp_ipsec_adjust_cksum(pkt, delta, proto, (pkt[0] & 0xf) * 4, policy)
    else:
        want, valid = pkt, False
    ctx = (proto, policy, hex(delta), len(pkt), pkt[0] & 0xf)
    assert bytes(buf[G:G + len(pkt)]) == want, ctx
    assert bytes(buf[:G]) == before[:G] and bytes(buf[G + len(pkt):]) == before[G + len(pkt):], ctx
    assert cf == (L.NATT_CSUM_VALID if valid else 0), ctx
    return want, cf


def _csum_ok(pkt, proto):
    """The checksum a receiver verifies: pseudo-header and segment sum to 0."""
    ihl = (pkt[0] & 0xf) * 4
    seg = pkt[ihl:ihl + struct.unpack(">H", pkt[ihl + 4:ihl + 6])[0]] if proto == 17 else pkt[ihl:]
    ph = pkt[12:20] + struct.pack(">BBH", 0, proto, len(seg))
    data = ph + seg + (b"\0" if len(seg) & 1 else b"")
    return E.in_cksum(data) == 0


@pytest.mark.parametrize("proto", [6, 17])
@pytest.mark.parametrize("policy", [0, 1])
def test_cksum_every_segment_length(proto, policy):
    rng = np.random.default_rng(1230 + proto + policy)
    changed = 0
    for seglen in list(range(0, 41)) + [255, 256, 257, 1480]:
        for ihl in (5, 6, 15):
            for delta in (0, int(rng.integers(1, 65536))):
                pkt = NH.tpacket(rng, proto, seglen, ihl=ihl)
                after, cf = _check_cksum(rng, pkt, proto, policy, delta)
                changed += after != pkt
                if policy and after != pkt:
                    assert _csum_ok(after, proto), (seglen, ihl)
                if seglen < (8 if proto == 17 else 18):
                    assert after == pkt and cf == 0               # too short to hold the field
                # not a NAT-T SA, or another protocol: nothing happens
                _check_cksum(rng, pkt, proto, policy, delta, natt=False)
                _check_cksum(rng, pkt, 50 if proto == 6 else 4, policy, delta)
    assert changed > 60                                           # (TCP under auto moves only with a delta)


def test_cksum_auto_policy_values():
    rng = np.random.default_rng(1240)
    off = {6: 16, 17: 6}
    # (field, delta) -> in_addword: plain, 0xffff reached exactly, the carry, 0x1fffe
    for field, delta, want in ((0x1234, 0x0101, 0x1335), (0xff00, 0x00ff, 0xffff), (0xffff, 0x0001, 0x0001),
                               (0xffff, 0xffff, 0xffff), (0x8000, 0x8000, 0x0001), (0x0001, 0xfffe, 0xffff)):
        for proto in (6, 17):
            pkt = NH.tpacket(rng, proto, 40, field=field)
            after, cf = _check_cksum(rng, pkt, proto, 0, delta)
            at = 20 + off[proto]
            assert struct.unpack("<H", after[at:at + 2])[0] == want and cf == 0
    # field 0: UDP stays, TCP is adjusted
    u, _ = _check_cksum(rng, NH.tpacket(rng, 17, 40, field=0), 17, 0, 0x0203)
    assert u[26:28] == b"\0\0"
    t, _ = _check_cksum(rng, NH.tpacket(rng, 6, 40, field=0), 6, 0, 0x0203)
    assert t[36:38] == b"\x03\x02"
    # delta 0: UDP is reset, TCP untouched and marked valid
    pkt = NH.tpacket(rng, 17, 40, field=0x7777)
    u, cf = _check_cksum(rng, pkt, 17, 0, 0)
    assert u[26:28] == b"\0\0" and cf == 0 and u[:26] + u[28:] == pkt[:26] + pkt[28:]
    pkt = NH.tpacket(rng, 6, 40, field=0x7777)
    t, cf = _check_cksum(rng, pkt, 6, 0, 0)
    assert t == pkt and cf == L.NATT_CSUM_VALID


def test_cksum_recompute_folds_and_lengths():
    rng = np.random.default_rng(1241)
    zero = {6: 0, 17: 0}
    for proto in (6, 17):
        for seglen in (20, 21, 38, 39, 257):
            for _ in range(4):
                # the sum folds to 0xffff: TCP stores 0x0000, UDP 0xffff instead
                base = NH.tpacket(rng, proto, seglen, ihl=int(rng.integers(5, 16)))
                ihl = (base[0] & 0xf) * 4
                pkt = NH.force_result_zero(base, proto, ihl + (8 if proto == 17 else 0))
                if pkt is None:
                    continue
                after, _ = _check_cksum(rng, pkt, proto, 1, 0x1111)
                at = ihl + (6 if proto == 17 else 16)
                assert after[at:at + 2] == (b"\xff\xff" if proto == 17 else b"\0\0"), (proto, seglen)
                assert _csum_ok(after, proto)
                zero[proto] += 1
    assert zero[6] >= 10 and zero[17] >= 10
    # in_pseudo alone folds to 0xffff: source address chosen so that src + dst + htons(len + proto) = 0 mod 65535
    for proto in (6, 17):
        p = bytearray(NH.tpacket(rng, proto, 36))
        p[12:14] = b"\0\0"
        src, dst = struct.unpack("<II", p[12:20])
        c = struct.unpack("<H", struct.pack(">H", 36 + proto))[0]
        rest = E.in_pseudo(src, dst, c)
        p[12:14] = struct.pack("<H", 0xffff - rest)
        assert E.in_pseudo(*struct.unpack("<II", p[12:20]), c) == 0xffff
        after, _ = _check_cksum(rng, bytes(p), proto, 1, 0)
        assert after != bytes(p)
    # uh_ulen short, equal, shorter than the packet, and too long
    for ulen, moves in ((0, False), (7, False), (8, True), (23, True), (40, True), (41, False), (65535, False)):
        pkt = NH.tpacket(rng, 17, 40, ulen=ulen)
        after, _ = _check_cksum(rng, pkt, 17, 1, 0)
        assert (after != pkt) == moves or (moves and after[26:28] == pkt[26:28]), ulen
        if ulen == 40:                                 # (a shorter uh_ulen: the pseudo-header still says len - skip, :285)
            assert _csum_ok(after, 17), ulen
    # a TCP packet whose ip_len is not its length is left alone
    pkt = NH.tpacket(rng, 6, 40, ip_len=64)
    assert _check_cksum(rng, pkt, 6, 1, 0)[0] == pkt
    # a field of 0, and of 0xffff, before the recompute: the same result
    a = NH.tpacket(rng, 6, 33, field=0)
    b = a[:36] + b"\xff\xff" + a[38:]
    assert _check_cksum(rng, a, 6, 1, 0)[0] == _check_cksum(rng, b, 6, 1, 0)[0]
