"""Shared by the decapsulation tests: decrypted ESP packets of every kind the
rule distinguishes, the trailer word of a decrypted record, one packet through
both the host rule and esp.py's restatement of the reference, and the host
rule applied to a batch."""
import struct

import numpy as np

from espgpu import _lib as L
from espgpu import esp as E
from espgpu.batch import INSA_DTYPE, PKT_DTYPE

EINVAL, ENODATA, EPFNOSUPPORT = L.EINVAL, L.ENODATA, L.EPFNOSUPPORT
IVLENS, ALENS = (0, 8, 16), (0, 8, 12, 16, 24, 32)
MODES = (E.IPSEC_MODE_ANY, E.IPSEC_MODE_TRANSPORT, E.IPSEC_MODE_TUNNEL)
NXTS = (4, 41, 6, 17, 59, 50)
GUARD = 32


def in_flags(mode, af6=False, prand=False):
    return ({E.IPSEC_MODE_ANY: 0, E.IPSEC_MODE_TRANSPORT: L.IN_TRANSPORT, E.IPSEC_MODE_TUNNEL: L.IN_TUNNEL}[mode] |
            (L.IN_AF6 if af6 else 0) | (L.IN_PAD_RAND if prand else 0))


def flags_mode(flags):
    """(mode, af6, prand) of usable ESPGPU_IN_* flags."""
    mode = {0: E.IPSEC_MODE_ANY, L.IN_TRANSPORT: E.IPSEC_MODE_TRANSPORT, L.IN_TUNNEL: E.IPSEC_MODE_TUNNEL}[flags & 3]
    return mode, bool(flags & L.IN_AF6), bool(flags & L.IN_PAD_RAND)


def outer4(rng, ihl, total, proto=50, bad_sum=False, fold_ffff=False):
    """An outer IPv4 header of ihl dwords with random options; fold_ffff: the
    16-bit words without the checksum sum to 0xffff, so the field holds 0."""
    h = bytearray(struct.pack(">BBHHHBBH4s4s", 0x40 | ihl, int(rng.integers(256)), total & 0xffff,
                              int(rng.integers(65536)), 0, int(rng.integers(1, 256)), proto, 0,
                              rng.integers(0, 256, 4, dtype=np.uint8).tobytes(),
                              rng.integers(0, 256, 4, dtype=np.uint8).tobytes()) +
                  rng.integers(0, 256, ihl * 4 - 20, dtype=np.uint8).tobytes())
    if fold_ffff:
        h[4:6] = b"\0\0"
        h[4:6] = struct.pack(">H", E.in_cksum(bytes(h)))     # the id field absorbs the rest
    h[10:12] = struct.pack(">H", E.in_cksum(bytes(h)))
    if bad_sum:
        h[11] ^= 0x5a
    return bytes(h)


def outer6(rng, plen, nxt=50):
    return struct.pack(">IHBB", 0x60000000 | int(rng.integers(1 << 28)), plen & 0xffff, nxt,
                       int(rng.integers(1, 256))) + rng.integers(0, 256, 32, dtype=np.uint8).tobytes()


def record(rng, ivlen, alen, q, padlen, nxt, lastpad=None, padbyte=None):
    """A decrypted ESP record: header and IV, q payload bytes, padlen pad bytes
    1, 2, 3, ... (the last one `lastpad` if given), the pad length byte
    (`padbyte` if it is to lie), next header, ICV: plen = q + padlen + 2."""
    pad = bytearray(range(1, padlen + 1))
    if lastpad is not None and pad:
        pad[-1] = lastpad
    return (rng.integers(0, 256, 8 + ivlen + q, dtype=np.uint8).tobytes() + bytes(pad) +
            bytes([padlen if padbyte is None else padbyte, nxt]) + rng.integers(0, 256, alen, dtype=np.uint8).tobytes())


def packet(rng, af6, ivlen, alen, q, nxt, padlen=None, ihl=5, lastpad=None, padbyte=None, **kw):
    """(outer header + decrypted record, skip, rlen) as the decrypt leaves them."""
    if padlen is None:
        padlen = int(rng.integers(0, 12))
    rec = record(rng, ivlen, alen, q, padlen, nxt, lastpad, padbyte)
    if af6:
        return outer6(rng, len(rec)) + rec, 40, len(rec)
    return outer4(rng, ihl, ihl * 4 + len(rec), **kw) + rec, ihl * 4, len(rec)


def trailer_of(pkt, skip, rlen, ivlen, alen):
    """The word espgpu_decrypt_batch_trailer gives for the record at pkt +
    skip: the kernels' esp_trailer_word on the dword that holds the last three
    payload bytes, as they lie in the unstripped packet."""
    end = skip + rlen - alen
    plen = rlen - 8 - ivlen - alen
    l0, padlen, nh = pkt[end - 3], pkt[end - 2], pkt[end - 1]
    t = nh | padlen << 8 | L.TR_VALID
    if padlen + 2 > plen:
        t |= L.TR_BADLEN
    if padlen != l0 and padlen != 0:
        t |= L.TR_BADPAD
    if nh == 59:
        t |= L.TR_NONE
    return t


def shape_of(ivlen, alen):
    return L.EShape(ivlen, 16 if ivlen == 16 else 4, alen)


def check_one(rng, flags, ivlen, alen, pkt, skip, rlen, trailer=None, bytes0=0, packets0=0, want=None):
    """One packet through espgpu_esp_decap, in a buffer with guard bytes around
    it, against esp.esp_input_decap: status, result, the resulting packet's
    bytes, every other byte of the buffer and the SA's counters.  `want`: the
    expected status where the restatement cannot express the input (unusable
    flags, a trailer word that is not the bytes' own).  Returns the status."""
    pkt = bytes(pkt)
    if trailer is None:
        trailer = trailer_of(pkt, skip, rlen, ivlen, alen)
    buf = bytearray(rng.integers(0, 256, GUARD, dtype=np.uint8).tobytes() + pkt +
                    rng.integers(0, 256, GUARD, dtype=np.uint8).tobytes())
    before = bytes(buf)
    insa = L.InSA(bytes0, packets0, flags, 0x5a5a5a5a)
    st, off, ln = E.esp_decap_host(insa, shape_of(ivlen, alen), buf, skip, rlen, trailer, at=GUARD)
    if want is None:
        mode, af6, prand = flags_mode(flags)
        want, res, booked = E.esp_input_decap(mode, af6, prand, ivlen, alen, pkt[:skip + rlen], skip)
    else:
        assert want != 0
        res, booked = None, 0
    ctx = (flags, ivlen, alen, skip, rlen, hex(trailer))
    assert st == want, (st, want) + ctx
    assert (insa.flags, insa.pad_) == (flags, 0x5a5a5a5a)
    if st:
        assert (off, ln) == (0, 0), ctx
        assert bytes(buf) == before, ("a refused packet was written",) + ctx
        assert (insa.bytes, insa.packets) == (bytes0, packets0), ctx
        return st
    assert ln == len(res) == booked, (ln, len(res), booked) + ctx
    a = GUARD + off
    assert bytes(buf[a:a + ln]) == res, ("resulting packet", off, ln) + ctx
    assert bytes(buf[:a]) == before[:a] and bytes(buf[a + ln:]) == before[a + ln:], ("outside the result",) + ctx
    assert insa.bytes == (bytes0 + booked) & (2**64 - 1) and insa.packets == packets0 + 1, ctx
    return 0


def layout(rng, pkts, max_gap4=6):
    """The packets at an irregular 4-byte-aligned stride in one arena of
    random bytes: (arena uint8 array, PKT_DTYPE array)."""
    offs, pos = [], 4 * int(rng.integers(0, max_gap4 + 1))
    for p in pkts:
        offs.append(pos)
        pos += ((len(p) + 3) & ~3) + 4 * int(rng.integers(0, max_gap4 + 1))
    arena = rng.integers(0, 256, pos + 64, dtype=np.uint8)
    rec = np.zeros(len(pkts), dtype=PKT_DTYPE)
    for i, p in enumerate(pkts):
        arena[offs[i]:offs[i] + len(p)] = np.frombuffer(p, dtype=np.uint8)
        rec[i] = (offs[i] // 4, len(p))
    return arena, rec


def host_decap_batch(arena, out, rec, desc, trailer, status, insa, shapes):
    """espgpu_esp_decap_batch's contract with the host rule, in index order.
    arena holds the outer headers, out the decrypted records (the same array
    for the in-place form); shapes[sa] is the (ivlen, alen) of the ESP session
    with that id, None where the ctx has no such session.  Returns (out,
    PKT_DTYPE ipkt, dstatus, INSA_DTYPE insa); the inputs are not modified."""
    n = len(rec)
    res = out.copy()
    ipkt = np.zeros(n, dtype=PKT_DTYPE)
    dst = np.zeros(n, dtype=np.uint8)
    ins = [L.InSA(int(e["bytes"]), int(e["packets"]), int(e["flags"]), int(e["pad_"])) for e in insa]
    for i in range(n):
        o4, sa = int(rec["off4"][i]), int(desc["sa"][i])
        ipkt[i] = (o4, 0)
        if status[i]:
            continue
        dst[i] = EINVAL
        if sa >= len(ins) or sa >= len(shapes) or shapes[sa] is None:
            continue
        ivlen, alen = shapes[sa]
        skip, rlen = (int(desc["off4"][i]) - o4) * 4, int(desc["len"][i])
        assert 0 <= skip < 64, "the helper takes descriptors that belong to their packets"
        o = o4 * 4
        # the header as the arena has it in front of the record as out has it
        tmp = bytearray(arena[o:o + skip].tobytes() + res[o + skip:o + skip + rlen].tobytes())
        st, off, ln = E.esp_decap_host(ins[sa], shape_of(ivlen, alen), tmp, skip, rlen, int(trailer[i]))
        dst[i] = st
        if st == 0:
            ipkt[i] = (o4 + off // 4, ln)
            if off == 8 + ivlen:                                     # transport: the header moved
                res[o + off:o + off + skip] = np.frombuffer(bytes(tmp[off:off + skip]), dtype=np.uint8)
    got = np.zeros(len(ins), dtype=INSA_DTYPE)
    for k, s in enumerate(ins):
        got[k] = (s.bytes, s.packets, s.flags, s.pad_)
    return res, ipkt, dst, got
