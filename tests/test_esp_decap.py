"""espgpu_esp_decap, the host rule of the inbound decapsulation step
(f-stack_amd/csrc/decap.h), against esp.esp_input_decap, a restatement of
esp_input_cb's tail and ipsec4/6_common_input_cb on bytes that shares nothing
with it: status, result offset and length, the resulting packet's bytes, every
byte of the buffer outside the result, and the SA's counters (check_one)."""
import ctypes as C
import struct

import numpy as np
import pytest

from decap_helpers import (ALENS, EINVAL, ENODATA, EPFNOSUPPORT, IVLENS, MODES, NXTS, check_one, in_flags, packet,
                           shape_of, trailer_of)
from espgpu import _lib as L
from espgpu import esp as E
from espgpu.batch import INSA_DTYPE

ANY, TRANSPORT, TUNNEL = MODES


def test_abi_additions():
    assert C.sizeof(L.InSA) == 24 and INSA_DTYPE.itemsize == 24
    for f in ("bytes", "packets", "flags", "pad_"):
        assert getattr(L.InSA, f).offset == INSA_DTYPE.fields[f][1]
    src = open(L.HEADER).read()
    for name, v in (("IN_TRANSPORT", "0x1"), ("IN_TUNNEL", "0x2"), ("IN_PAD_RAND", "0x4"), ("IN_AF6", "0x8"),
                    ("ENODATA", "61"), ("EPFNOSUPPORT", "96")):
        assert int(v, 0) == getattr(L, name)
        assert any(ln.split()[:3] == ["#define", "ESPGPU_" + name, v] for ln in src.splitlines()), name
    assert {"espgpu_esp_decap", "espgpu_esp_decap_batch"} <= set(L.header_symbols())
    assert L.lib().espgpu_abi_version() == 6


def _expected(mode, af6, nxt, q):
    """The rule's table (include/espgpu.h, checks 1-3), spelled out once more."""
    if nxt == 59:
        return ENODATA
    if nxt in (4, 41) and mode != TRANSPORT:
        return EINVAL if q < (20 if nxt == 4 else 40) else 0
    if not af6 and mode == TUNNEL:
        return EPFNOSUPPORT
    return 0


@pytest.mark.parametrize("af6", [False, True], ids=["af4", "af6"])
@pytest.mark.parametrize("mode", MODES, ids=["any", "transport", "tunnel"])
def test_every_shape_mode_and_next_header(mode, af6):
    rng = np.random.default_rng(70 + mode + 3 * af6)
    for ivlen in IVLENS:
        for alen in ALENS:
            for nxt in NXTS:
                for q in (0, 19, 20, 39, 40, 77):
                    pkt, skip, rlen = packet(rng, af6, ivlen, alen, q, nxt, ihl=int(rng.integers(5, 16)))
                    st = check_one(rng, in_flags(mode, af6), ivlen, alen, pkt, skip, rlen)
                    assert st == _expected(mode, af6, nxt, q), (ivlen, alen, nxt, q)


@pytest.mark.parametrize("ihl", range(5, 16))
def test_ipv4_header_move_overlaps_at_every_distance(ihl):
    """hlen 8, 16, 24 against skip 20 .. 60: the source and the destination of
    the move overlap by every amount, and not at all for hlen 24 > skip 20."""
    rng = np.random.default_rng(80 + ihl)
    for ivlen in IVLENS:
        for mode in (ANY, TRANSPORT):
            for nxt in (6, 17, 50):
                pkt, skip, rlen = packet(rng, False, ivlen, 16, int(rng.integers(0, 200)), nxt, ihl=ihl)
                assert check_one(rng, in_flags(mode), ivlen, 16, pkt, skip, rlen) == 0


def test_ipv6_transport():
    rng = np.random.default_rng(81)
    for ivlen in IVLENS:
        for mode, nxt in ((ANY, 6), (TRANSPORT, 41), (TRANSPORT, 4), (TUNNEL, 17), (TUNNEL, 50), (ANY, 58)):
            pkt, skip, rlen = packet(rng, True, ivlen, 12, int(rng.integers(0, 200)), nxt)
            assert check_one(rng, in_flags(mode, True), ivlen, 12, pkt, skip, rlen) == 0


def test_payload_of_two_three_and_four_bytes():
    """plen 2, 3, 4, with the pad length at plen - 2 (the whole payload is
    padding) and at plen - 1 (BADLEN); plen 1 and 0 are refused outright."""
    rng = np.random.default_rng(82)
    for af6 in (False, True):
        for ivlen in IVLENS:
            for plen in (2, 3, 4):
                for padlen, want in ((plen - 2, 0), (plen - 1, EINVAL)):
                    pkt, skip, rlen = packet(rng, af6, ivlen, 8, 0, 6, padlen=plen - 2, padbyte=padlen)
                    assert rlen == 8 + ivlen + plen + 8
                    assert check_one(rng, in_flags(TRANSPORT, af6), ivlen, 8, pkt, skip, rlen) == want
            for plen in (0, 1):
                pkt, skip, rlen = packet(rng, af6, ivlen, 8, 0, 6, padlen=0)
                pkt = pkt[:skip + 8 + ivlen + plen] + pkt[-8:]
                st = check_one(rng, in_flags(TRANSPORT, af6), ivlen, 8, pkt, skip, len(pkt) - skip,
                               trailer=L.TR_VALID | 6)
                assert st == EINVAL


def test_bad_pad_byte_with_and_without_pad_rand():
    rng = np.random.default_rng(83)
    for af6 in (False, True):
        for mode, nxt in ((TRANSPORT, 6), (TUNNEL, 4)):
            for prand, want in ((False, EINVAL), (True, 0)):
                pkt, skip, rlen = packet(rng, af6, 8, 16, 48, nxt, padlen=6, lastpad=0x77)
                assert trailer_of(pkt, skip, rlen, 8, 16) & L.TR_BADPAD
                assert check_one(rng, in_flags(mode, af6, prand), 8, 16, pkt, skip, rlen) == want
            # a zero pad length passes whatever lies before it (:614)
            pkt, skip, rlen = packet(rng, af6, 8, 16, 48, nxt, padlen=0)
            assert check_one(rng, in_flags(mode, af6), 8, 16, pkt, skip, rlen) == 0


def test_trailer_words_that_are_not_a_verdict():
    """Without VALID (the record failed before), and with BADLEN / NONE set on
    a record whose bytes are fine: the word decides, not the bytes."""
    rng = np.random.default_rng(84)
    for mode, nxt in ((TRANSPORT, 6), (TUNNEL, 4)):
        pkt, skip, rlen = packet(rng, False, 8, 16, 48, nxt, padlen=2)
        t = trailer_of(pkt, skip, rlen, 8, 16)
        f = in_flags(mode)
        assert check_one(rng, f, 8, 16, pkt, skip, rlen, trailer=t) == 0
        for word, want in ((t & ~L.TR_VALID, EINVAL), (0, EINVAL), (t | L.TR_BADLEN, EINVAL), (t | L.TR_NONE, ENODATA),
                           (t | L.TR_BADPAD, EINVAL), (t | L.TR_BADLEN | L.TR_NONE, EINVAL),
                           (t | L.TR_BADPAD | L.TR_NONE, EINVAL), ((t & ~0xff00) | 0xff00, EINVAL)):
            assert check_one(rng, f, 8, 16, pkt, skip, rlen, trailer=word, want=want) == want
        assert check_one(rng, f | L.IN_PAD_RAND, 8, 16, pkt, skip, rlen, trailer=t | L.TR_BADPAD | L.TR_NONE,
                         want=ENODATA) == ENODATA


def test_unusable_flags():
    rng = np.random.default_rng(85)
    pkt, skip, rlen = packet(rng, False, 8, 16, 48, 4, padlen=2)
    for f in (L.IN_TRANSPORT | L.IN_TUNNEL, 0x10, 0x80000000, L.IN_TUNNEL | 0x100, 0xf):
        assert check_one(rng, f, 8, 16, pkt, skip, rlen, want=EINVAL) == EINVAL


def test_unusable_skip():
    rng = np.random.default_rng(86)
    for mode, nxt in ((TRANSPORT, 6), (TUNNEL, 4)):
        for af6, skip in ((False, 16), (False, 64), (False, 0), (False, 22), (False, 41), (True, 44), (True, 36),
                          (True, 20), (True, 42)):
            pkt, _, rlen = packet(rng, af6, 8, 16, 48, nxt, padlen=2, ihl=15)
            hdr = (pkt[:60] * 2)[:skip]
            assert check_one(rng, in_flags(mode, af6), 8, 16, hdr + pkt[-rlen:], skip, rlen) == EINVAL


def test_header_that_is_not_the_skip_says():
    """Transport mode reads the header it moves: ip_hl * 4 != skip or a wrong
    version nibble refuse the packet.  Tunnel mode never looks."""
    rng = np.random.default_rng(87)
    for first in (0x46, 0x45 + 0x20, 0x35, 0x65, 0x05):
        pkt, skip, rlen = packet(rng, False, 8, 16, 48, 6, padlen=2, ihl=5)
        bad = bytes([first]) + pkt[1:]
        assert check_one(rng, in_flags(TRANSPORT), 8, 16, bad, skip, rlen) == EINVAL
    for first in (0x40, 0x50, 0x70, 0x00, 0xf0):
        pkt, skip, rlen = packet(rng, True, 8, 16, 48, 6, padlen=2)
        bad = bytes([first | (pkt[0] & 0xf)]) + pkt[1:]
        assert check_one(rng, in_flags(TRANSPORT, True), 8, 16, bad, skip, rlen) == EINVAL
    for af6 in (False, True):
        pkt, skip, rlen = packet(rng, af6, 8, 16, 48, 4, padlen=2)
        insa = L.InSA(0, 0, in_flags(TUNNEL, af6), 0)
        buf = bytearray(b"\xff" * skip + pkt[skip:])
        assert E.esp_decap_host(insa, shape_of(8, 16), buf, skip, rlen, trailer_of(pkt, skip, rlen, 8, 16)) == \
            (0, skip + 16, 48)


def test_checksum_is_recomputed_in_full():
    """A stored checksum that was wrong does not survive (an incremental
    update would carry the error over); a header whose words fold to 0xffff
    gets the checksum 0."""
    rng = np.random.default_rng(88)
    for ihl in (5, 6, 11, 15):
        for kw in (dict(bad_sum=True), dict(fold_ffff=True)):
            # q chosen so that ip_len does not change: the folded sum stays 0xffff
            pkt, skip, rlen = packet(rng, False, 8, 16, 50, 50, padlen=0, ihl=ihl, **kw)
            if "fold_ffff" in kw:
                # the new ip_len and ip_p differ from the old: rebuild the id so that the *result* folds to 0xffff
                h = bytearray(pkt[:skip])
                h[2:4], h[9], h[10:12], h[4:6] = struct.pack(">H", skip + 50), 50, b"\0\0", b"\0\0"
                h[4:6] = struct.pack(">H", E.in_cksum(bytes(h)))
                assert E.in_cksum(bytes(h)) == 0
                pkt = bytes(h) + pkt[skip:]
            buf = bytearray(pkt)
            insa = L.InSA(0, 0, in_flags(TRANSPORT), 0)
            st, off, ln = E.esp_decap_host(insa, shape_of(8, 16), buf, skip, rlen, trailer_of(pkt, skip, rlen, 8, 16))
            assert (st, off, ln) == (0, 16, skip + 50)
            hdr = bytes(buf[off:off + skip])
            assert E.in_cksum(hdr) == 0 and struct.unpack(">H", hdr[2:4])[0] == ln and hdr[9] == 50
            if "fold_ffff" in kw:
                assert hdr[10:12] == b"\0\0"
            assert check_one(rng, in_flags(TRANSPORT), 8, 16, pkt, skip, rlen) == 0


def test_counters_carry_and_stay_on_refusal():
    rng = np.random.default_rng(89)
    pkt, skip, rlen = packet(rng, False, 8, 16, 300, 4, padlen=2)
    assert check_one(rng, in_flags(TUNNEL), 8, 16, pkt, skip, rlen, bytes0=2**32 - 100, packets0=2**32 - 1) == 0
    assert check_one(rng, in_flags(TRANSPORT), 8, 16, pkt, skip, rlen, bytes0=2**32 - 100, packets0=2**32 - 1) == 0
    assert check_one(rng, in_flags(TUNNEL), 8, 16, pkt, skip, rlen, bytes0=2**64 - 100, packets0=7) == 0
    pkt, skip, rlen = packet(rng, False, 8, 16, 300, 17, padlen=2)
    assert check_one(rng, in_flags(TUNNEL), 8, 16, pkt, skip, rlen, bytes0=2**32 - 100, packets0=5) == EPFNOSUPPORT


def test_null_arguments_and_shapes():
    lib = L.lib()
    rng = np.random.default_rng(90)
    pkt, skip, rlen = packet(rng, False, 8, 16, 48, 4, padlen=2)
    buf = bytearray(pkt)
    raw = C.cast((C.c_uint8 * len(buf)).from_buffer(buf), C.c_void_p)
    insa, shape, off, ln = L.InSA(0, 0, 0, 0), shape_of(8, 16), C.c_uint32(7), C.c_uint32(7)
    t = trailer_of(pkt, skip, rlen, 8, 16)
    good = [C.byref(insa), C.byref(shape), raw, skip, rlen, t, C.byref(off), C.byref(ln)]
    for k in (0, 1, 2, 6, 7):
        a = list(good)
        a[k] = None
        assert lib.espgpu_esp_decap(*a) == EINVAL
    for ivlen in (4, 12, 24, 0xfffffff8):
        bad = L.EShape(ivlen, 4, 16)
        assert lib.espgpu_esp_decap(C.byref(insa), C.byref(bad), raw, skip, rlen, t, C.byref(off), C.byref(ln)) == EINVAL
    bad = L.EShape(8, 4, 0xffffffff)
    assert lib.espgpu_esp_decap(C.byref(insa), C.byref(bad), raw, skip, rlen, t, C.byref(off), C.byref(ln)) == EINVAL
    # tunnel mode does not touch the packet, so a length near 2^32 shows the arithmetic alone
    assert lib.espgpu_esp_decap(C.byref(insa), C.byref(shape), raw, skip, 0xfffffffc, t, C.byref(off), C.byref(ln)) == 0
    assert (off.value, ln.value) == (skip + 16, 0xfffffffc - 32 - 4) and bytes(buf) == pkt
    assert (insa.bytes, insa.packets) == (0xfffffffc - 32 - 4, 1)
    insa = L.InSA(0, 0, 0, 0)
    assert lib.espgpu_esp_decap(*[C.byref(insa)] + good[1:]) == 0 and (off.value, ln.value) == (skip + 16, 48)


def test_random_packets():
    """5000 packets of every family, mode, shape and next header, a fifth of
    them with a defect."""
    rng = np.random.default_rng(91)
    seen = {}
    for _ in range(5000):
        af6, mode, prand = bool(rng.integers(2)), MODES[int(rng.integers(3))], bool(rng.integers(4) == 0)
        ivlen, alen = IVLENS[int(rng.integers(3))], ALENS[int(rng.integers(6))]
        nxt = int(rng.choice([4, 41, 6, 17, 50, 1, 58, 59, 4, 41]))
        q = int(rng.choice([0, 8, 19, 20, 21, 39, 40, 41, 64, int(rng.integers(0, 1400))]))
        kw = {}
        defect = int(rng.integers(10))
        if defect == 0:
            kw["lastpad"] = int(rng.integers(256))
        elif defect == 1:
            kw["padbyte"] = int(rng.integers(256))
        pkt, skip, rlen = packet(rng, af6, ivlen, alen, q, nxt, ihl=int(rng.integers(5, 16)), **kw)
        st = check_one(rng, in_flags(mode, af6, prand), ivlen, alen, pkt, skip, rlen,
                       bytes0=int(rng.integers(0, 2**63)), packets0=int(rng.integers(0, 2**40)))
        seen[st] = seen.get(st, 0) + 1
    assert set(seen) == {0, EINVAL, ENODATA, EPFNOSUPPORT} and seen[0] > 2500, seen
