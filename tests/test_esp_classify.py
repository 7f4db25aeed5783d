"""Inbound classification, host side: espgpu_esp_classify (the rule that defines
espgpu_esp_classify_batch) against esp.py's restatement of ip_input /
ipsec_common_input / key_allocsa / esp_input's first lines, on a directed
packet either side of every limit of the rule and on random packets of every
kind; and espgpu_sad_build's table.  No GPU."""
import numpy as np
import pytest

from classify_helpers import (EINVAL, ENOENT, ENOTSUP, KINDS, Sadb, chain_spis, dst_of, esp_payload, expected_status, ipv4, ipv6,
                              random_packets)
from espgpu import _lib as L
from espgpu import esp as E
from espgpu import shard
from espgpu.batch import SAD_DTYPE, sad_build

RNG = np.random.default_rng(50)
DB = Sadb(RNG)
TABLE = sad_build(DB.entries, 128)
OFF4 = 0x00345678


def both(pkt, flags=0, table=TABLE, db=DB, off4=OFF4):
    """(status, descriptor) of the host rule, after checking it against the restatement."""
    got = E.esp_classify_host(table, pkt, off4, flags)
    want = E.ipsec_input_classify(db.ref, pkt, off4, ipcsum=bool(flags & L.CLS_IPCSUM))
    assert got == want, (bytes(pkt).hex(), got, want)
    if got[0]:
        assert got[1] == (off4, 0, 0xffff, 0, 0)
    return got


def accepted(e, skip, rlen, off4=OFF4):
    return 0, (off4 + skip // 4, rlen, int(e["sa"]), 0, int(e["salt"]))


E4, E6, EAH = DB.pick(RNG, af=4), DB.pick(RNG, af=6), DB.pick(RNG, proto=51)


def rec4(n=24):
    return esp_payload(RNG, int(E4["spi"]), n)


def rec6(n=24):
    return esp_payload(RNG, int(E6["spi"]), n)


def test_structs_match_the_header():
    import ctypes as C
    assert C.sizeof(L.Pkt) == 8 and C.sizeof(L.SadEntry) == 32 and SAD_DTYPE.itemsize == 32
    for f in ("spi", "sa", "proto", "af", "salt", "flags", "dst"):
        assert getattr(L.SadEntry, f).offset == SAD_DTYPE.fields[f][1]
    assert L.lib().espgpu_abi_version() == 6


@pytest.mark.parametrize("flags", [0, L.CLS_IPCSUM])
def test_ipv4_limits(flags):
    d4 = dst_of(E4)
    good = ipv4(d4, rec4())
    assert both(good, flags) == accepted(E4, 20, 24)
    # 1. len < 20; the version nibble
    assert both(good[:19], flags)[0] == EINVAL and both(b"", flags)[0] == EINVAL
    assert both(ipv4(d4, b"", ip_len=20), flags)[0] == EINVAL          # 20 bytes: read, then no room for ESP
    for v in (0, 3, 5, 7, 15):
        assert both(bytes([v << 4 | 5]) + good[1:], flags)[0] == EINVAL
    # 2. hlen < 20; hlen > len
    assert both(bytes([0x44]) + good[1:], flags)[0] == EINVAL
    assert both(bytes([0x40]) + good[1:], flags)[0] == EINVAL
    p6 = ipv4(d4, rec4(), ihl=6)
    assert both(p6, flags) == accepted(E4, 24, 24)
    assert both(p6[:23], flags)[0] == EINVAL                             # hlen 24 > len 23
    assert both(ipv4(d4, b"", ihl=6, ip_len=48)[:24], flags)[0] == EINVAL   # hlen == len, ip_len > len
    # ip_len against hlen and len
    assert both(ipv4(d4, rec4(), ihl=6, ip_len=23), flags)[0] == EINVAL
    assert both(ipv4(d4, rec4(), ihl=6, ip_len=24), flags)[0] == EINVAL   # ip_len == hlen: no ESP header
    assert both(good[:43], flags)[0] == EINVAL                           # ip_len 44 > len 43
    assert both(ipv4(d4, rec4(), ip_len=45), flags)[0] == EINVAL
    # fragments
    for off in (0x2000, 0x0001, 0x1fff, 0x6000):
        assert both(ipv4(d4, rec4(), off=off), flags)[0] == ENOTSUP
    assert both(ipv4(d4, rec4(), off=0x4000), flags) == accepted(E4, 20, 24)   # DF alone
    assert both(ipv4(d4, rec4(), off=0x8000), flags) == accepted(E4, 20, 24)   # the reserved bit
    # protocol
    for p in (49, 51, 6, 17, 108):
        assert both(ipv4(d4, rec4(), proto=p), flags)[0] == ENOTSUP
    # a short AH packet is the host's, not EINVAL
    assert both(ipv4(d4, rec4(4), proto=51), flags)[0] == ENOTSUP
    # ip_len - hlen < 8; ip_len & 3
    assert both(ipv4(d4, rec4(7)), flags)[0] == EINVAL
    assert both(ipv4(d4, rec4(4)), flags)[0] == EINVAL
    assert both(ipv4(d4, rec4(8)), flags) == accepted(E4, 20, 8)
    for n in (9, 10, 11, 25, 27):
        assert both(ipv4(d4, rec4(n)), flags)[0] == EINVAL
    assert both(ipv4(d4, rec4(12)), flags) == accepted(E4, 20, 12)
    # the largest packet: ip_len 65532
    assert both(ipv4(d4, rec4(65532 - 20)), flags) == accepted(E4, 20, 65512)


@pytest.mark.parametrize("ihl", range(5, 16))
def test_ipv4_header_lengths(ihl):
    opts = RNG.integers(0, 256, ihl * 4 - 20, dtype=np.uint8).tobytes()
    for flags in (0, L.CLS_IPCSUM):
        p = ipv4(dst_of(E4), rec4(40), ihl=ihl, opts=opts)
        assert both(p, flags) == accepted(E4, ihl * 4, 40)
        assert both(p[:ihl * 4 - 1], flags)[0] == EINVAL
        bad = ipv4(dst_of(E4), rec4(40), ihl=ihl, opts=opts, bad_sum=True)
        assert both(bad, flags) == ((EINVAL, (OFF4, 0, 0xffff, 0, 0)) if flags else accepted(E4, ihl * 4, 40))
        if ihl > 5:                                   # a flipped option bit breaks the sum too
            q = bytearray(p)
            q[ihl * 4 - 1] ^= 0x10
            assert both(bytes(q), L.CLS_IPCSUM)[0] == EINVAL


def test_checksum_edges():
    """The sum is checked before ip_len, over the header alone, and its carries fold."""
    d4 = dst_of(E4)
    p = ipv4(d4, rec4(), ip_len=45, bad_sum=True)
    assert both(p, L.CLS_IPCSUM)[0] == EINVAL and both(p, 0)[0] == EINVAL
    p = bytearray(ipv4(d4, rec4()))
    p[30] ^= 0xff                                     # payload bytes are not summed
    assert both(bytes(p), L.CLS_IPCSUM)[0] == 0
    # all-ones options: every dword carries
    p = ipv4(d4, rec4(), ihl=15, opts=b"\xff" * 40)
    assert both(p, L.CLS_IPCSUM) == accepted(E4, 60, 24)
    # a checksum field of zeros where one is due
    z = bytearray(ipv4(d4, rec4()))
    z[10:12] = b"\0\0"
    assert both(bytes(z), L.CLS_IPCSUM)[0] == EINVAL and both(bytes(z), 0)[0] == 0
    # fragment and protocol are answered only with a right sum
    assert both(ipv4(d4, rec4(), off=0x2000, bad_sum=True), L.CLS_IPCSUM)[0] == EINVAL
    assert both(ipv4(d4, rec4(), proto=6, bad_sum=True), L.CLS_IPCSUM)[0] == EINVAL


def test_ipv6_limits():
    d6 = dst_of(E6)
    good = ipv6(d6, rec6())
    assert both(good) == accepted(E6, 40, 24)
    assert both(good, L.CLS_IPCSUM) == accepted(E6, 40, 24)              # no header checksum in IPv6
    assert both(good[:39])[0] == EINVAL and both(good[:20])[0] == EINVAL
    assert both(ipv6(d6, rec6(), plen=0))[0] == ENOTSUP                  # jumbogram
    assert both(ipv6(d6, b"", plen=0))[0] == ENOTSUP                     # exactly 40 bytes
    assert both(good[:63])[0] == EINVAL                                  # 40 + plen > len
    assert both(ipv6(d6, rec6(), plen=25))[0] == EINVAL
    assert both(ipv6(d6, rec6(), plen=65535))[0] == EINVAL
    for nxt in (0, 43, 44, 51, 60, 17):
        assert both(ipv6(d6, rec6(), nxt=nxt))[0] == ENOTSUP
    assert both(ipv6(d6, rec6(25), nxt=44))[0] == ENOTSUP                # the host's before the alignment
    # fe80::/10 and its neighbours
    for b0, b1, st in ((0xfe, 0x80, ENOTSUP), (0xfe, 0xbf, ENOTSUP), (0xfe, 0x7f, ENOENT), (0xfe, 0xc0, ENOENT),
                       (0xff, 0x80, ENOENT), (0xfc, 0x80, ENOENT)):
        assert both(ipv6(bytes([b0, b1]) + d6[2:], rec6()))[0] == st
    assert both(ipv6(bytes([0xfe, 0x80]) + d6[2:], rec6(5)))[0] == ENOTSUP
    for n in (1, 4, 7, 9, 10, 11, 27):
        assert both(ipv6(d6, rec6(n)))[0] == EINVAL
    assert both(ipv6(d6, rec6(8))) == accepted(E6, 40, 8)
    assert both(ipv6(d6, rec6(65532))) == accepted(E6, 40, 65532)


def test_trailing_bytes_are_trimmed():
    for t in (1, 2, 3, 4, 17, 1000):
        assert both(ipv4(dst_of(E4), rec4(), tail=b"\xee" * t)) == accepted(E4, 20, 24)
        assert both(ipv6(dst_of(E6), rec6(), tail=b"\xee" * t)) == accepted(E6, 40, 24)
    # an unaligned ip_len stays unaligned however the buffer is padded
    assert both(ipv4(dst_of(E4), rec4(25), tail=b"\0\0\0"))[0] == EINVAL


def test_lookup():
    d4, d6 = dst_of(E4), dst_of(E6)
    assert both(ipv4(d4, esp_payload(RNG, 0, 24)))[0] == ENOENT
    assert both(ipv4(d4, esp_payload(RNG, DB.unknown_spi(RNG), 24)))[0] == ENOENT
    # an AH SA's SPI in an ESP packet to that SA's destination
    ah = esp_payload(RNG, int(EAH["spi"]), 24)
    assert both(ipv4(dst_of(EAH), ah) if EAH["af"] == 4 else ipv6(dst_of(EAH), ah))[0] == ENOENT
    # the right SPI under a wrong destination: every byte counts
    for k in range(4):
        d = bytearray(d4)
        d[k] ^= 0x80
        assert both(ipv4(d, rec4()))[0] == ENOENT
    for k in range(2, 16):
        d = bytearray(d6)
        d[k] ^= 0x01
        assert both(ipv6(d, rec6()))[0] == ENOENT
    # ... and under the wrong family
    assert both(ipv4(d6[:4], rec6()))[0] == ENOENT
    assert both(ipv6(bytes(E4["dst"]), rec4()))[0] == ENOENT
    # every SA of the table is found
    for e in DB.entries:
        p = esp_payload(RNG, int(e["spi"]), 16)
        got = both(ipv4(dst_of(e), p) if e["af"] == 4 else ipv6(dst_of(e), p))
        assert got == (accepted(e, 20 if e["af"] == 4 else 40, 16) if e["proto"] == 50
                       else (ENOENT, (OFF4, 0, 0xffff, 0, 0)))


def test_random_packets_of_every_kind():
    rng = np.random.default_rng(51)
    seen = set()
    for flags in (0, L.CLS_IPCSUM):
        for kind, pkt in random_packets(rng, DB, 2500):
            off4 = int(rng.integers(0, 2**32 - 64))
            st, _ = both(pkt, flags, off4=off4)
            assert st == expected_status(kind, flags), (kind, pkt.hex())
            seen.add(kind)
    assert seen == set(KINDS)


def test_bad_arguments():
    import ctypes as C
    p = ipv4(dst_of(E4), rec4())
    d = L.Desc(1, 2, 3, 4, 5)
    lib = L.lib()
    assert lib.espgpu_esp_classify(TABLE.ctypes.data, len(TABLE), p, len(p), 7, 0, None) == EINVAL
    for tab, ns, fl in ((None, 128, 0), (TABLE.ctypes.data, 0, 0), (TABLE.ctypes.data, 96, 0),
                        (TABLE.ctypes.data, 128, 2)):
        assert lib.espgpu_esp_classify(tab, ns, p, len(p), 7, fl, C.byref(d)) == EINVAL
        assert (d.off4, d.len, d.sa, d.esn_hi, d.salt) == (7, 0, 0xffff, 0, 0)


# ---- espgpu_sad_build ------------------------------------------------------------

def _entry(spi, sa=1, proto=50, af=4, dst=None, salt=0, flags=0):
    e = np.zeros(1, dtype=SAD_DTYPE)
    e["spi"], e["sa"], e["proto"], e["af"], e["salt"], e["flags"] = spi, sa, proto, af, salt, flags
    if dst is None:
        dst = [10, 1, 2, 3] if af == 4 else list(range(0x20, 0x30))
    e["dst"][0, :len(dst)] = list(dst)
    return e


def test_sad_build_refusals():
    ok = _entry(0x1000)
    assert len(sad_build(ok, 2)) == 2
    for nslots in (0, 1, 3, 6, 96):                        # not a power of two, or too small
        with pytest.raises(ValueError):
            sad_build(ok, nslots)
    three = np.concatenate([_entry(0x1000), _entry(0x1001), _entry(0x1002)])
    with pytest.raises(ValueError):
        sad_build(three, 4)                                # nslots < 2 * nsas
    assert len(sad_build(three, 8)) == 8
    assert len(sad_build(three[:2], 4)) == 4
    assert not sad_build(three[:0], 1)["spi"].any()        # an empty SAD: one free slot
    bad = [_entry(0), _entry(0x1000, proto=0), _entry(0x1000, proto=108), _entry(0x1000, proto=6),
           _entry(0x1000, af=0), _entry(0x1000, af=2), _entry(0x1000, af=28), _entry(0x1000, flags=1)]
    for k in (4, 9, 15):
        e = _entry(0x1000)
        e["dst"][0, k] = 1
        bad.append(e)
    for e in bad:
        with pytest.raises(ValueError):
            sad_build(e, 4)
        with pytest.raises(ValueError):
            sad_build(np.concatenate([_entry(0x999), e]), 8)       # after a good one
    # a duplicate SPI, whatever else differs (one SPI namespace, key.c:1106-1109)
    with pytest.raises(ValueError):
        sad_build(np.concatenate([_entry(0x1000), _entry(0x2000), _entry(0x1000, sa=9, proto=51, af=6)]), 8)
    # 51 and af 6 with a full address are fine
    assert len(sad_build(np.concatenate([_entry(0x1000, proto=51), _entry(0x2000, af=6)]), 4)) == 4


@pytest.mark.parametrize("nslots", [2, 128, 4096])
def test_sad_build_home_slots(nslots):
    """Entries land in probe order from key_u32hash(spi) & mask, whole, and
    everything else is free."""
    rng = np.random.default_rng(nslots)
    db = Sadb(rng, nesp4=nslots // 4, nesp6=nslots // 8, nah=nslots // 8) if nslots > 2 else Sadb(rng, 1, 0, 0)
    table = sad_build(db.entries, nslots)
    model = [None] * nslots
    for e in db.entries:
        s = shard.key_u32hash(int(e["spi"])) & (nslots - 1)
        while model[s] is not None:
            s = (s + 1) & (nslots - 1)
        model[s] = e
    for s in range(nslots):
        if model[s] is None:
            assert table[s].tobytes() == bytes(32)
        else:
            assert table[s].tobytes() == model[s].tobytes()
    for e in db.entries:
        if e["proto"] == 50:
            p = esp_payload(rng, int(e["spi"]), 16)
            pkt = ipv4(dst_of(e), p) if e["af"] == 4 else ipv6(dst_of(e), p)
            assert both(pkt, table=table, db=db) == accepted(e, 20 if e["af"] == 4 else 40, 16)
    assert both(ipv4(b"\x0a\0\0\1", esp_payload(rng, db.unknown_spi(rng), 16)), table=table, db=db)[0] == ENOENT


def test_sad_build_chain_wraps_past_the_end():
    nslots, home, k = 16, 13, 7
    spis = chain_spis(home, nslots, k + 1)
    rng = np.random.default_rng(5)
    db = Sadb(rng, nesp4=4, nesp6=3, nah=0, spis=spis[:k])
    table = sad_build(db.entries, nslots)
    want = [(home + j) % nslots for j in range(k)]                      # 13, 14, 15, 0, 1, 2, 3
    assert [int(table[s]["spi"]) for s in want] == [int(e["spi"]) for e in db.entries]
    assert sorted(np.nonzero(table["spi"])[0]) == sorted(want)
    for e in db.entries:
        p = esp_payload(rng, int(e["spi"]), 16)
        pkt = ipv4(dst_of(e), p) if e["af"] == 4 else ipv6(dst_of(e), p)
        assert both(pkt, table=table, db=db) == accepted(e, 20 if e["af"] == 4 else 40, 16)
    # the same home slot, absent: probed through the whole chain to the free slot
    assert both(ipv4(dst_of(db.entries[0])[:4], esp_payload(rng, spis[k], 16)), table=table, db=db)[0] == ENOENT


def test_full_probe_is_bounded():
    """A table with no free slot (not one espgpu_sad_build makes): the probe
    stops after nslots steps."""
    spis = chain_spis(1, 4, 4)
    table = np.concatenate([_entry(s) for s in spis])
    assert E.esp_classify_host(table, ipv4(b"\x0a\1\2\3", esp_payload(RNG, chain_spis(1, 4, 5)[4], 16)))[0] == ENOENT
    assert E.esp_classify_host(table, ipv4(b"\x0a\1\2\3", esp_payload(RNG, spis[3], 16)))[0] == 0
