"""Shared by the encapsulation tests: cleartext packets, SAs' outbound policies,
one packet through both the host rule and esp.py's restatement of the
reference, and the host rule applied to a batch."""
import struct

import numpy as np

from espgpu import _lib as L
from espgpu import esp as E
from espgpu.batch import PKT_DTYPE
from helpers import DESC

EINVAL, ENOTSUP, EMSGSIZE, EAFNOSUPPORT, ENOBUFS = L.EINVAL, L.ENOTSUP, L.EMSGSIZE, L.EAFNOSUPPORT, L.ENOBUFS
IVLENS, ALENS = (0, 8, 16), (0, 8, 12, 16, 24, 32)
GUARD = 32
ROOM = 8 + 16 + 40, 17 + 32        # the most any shape asks for: hlen + oh, padding + alen


def enc_flags(tunnel=False, af6=False, dfbit=0, ecn=0, rfc6864=False):
    return ((L.ENC_TUNNEL if tunnel else 0) | (L.ENC_AF6 if af6 else 0) |
            {0: 0, 1: L.ENC_DF_SET, 2: L.ENC_DF_COPY}[dfbit] |
            {0: 0, 1: L.ENC_ECN_ALLOWED, -1: L.ENC_ECN_NOCARE}[ecn] | (L.ENC_RFC6864 if rfc6864 else 0))


def flags_policy(flags):
    """(tunnel, af6, dfbit, ecn, rfc6864) of usable ESPGPU_ENC_* flags."""
    return (bool(flags & L.ENC_TUNNEL), bool(flags & L.ENC_AF6),
            {0: 0, L.ENC_DF_SET: 1, L.ENC_DF_COPY: 2}[flags & (L.ENC_DF_SET | L.ENC_DF_COPY)],
            {0: 0, L.ENC_ECN_ALLOWED: 1, L.ENC_ECN_NOCARE: -1}[flags & (L.ENC_ECN_ALLOWED | L.ENC_ECN_NOCARE)],
            bool(flags & L.ENC_RFC6864))


def addr(rng, af6):
    """A global unicast address: never unspecified, never link-local."""
    a = rng.integers(1, 255, 16 if af6 else 4, dtype=np.uint8)
    a[0] = 0x20
    return a.tobytes()


def encsa(flags, ttl, src, dst, bytes0=0, packets0=0):
    e = L.EncSA(bytes0, packets0, flags, ttl)
    e.pad_[:] = [0x5a, 0x5b, 0x5c]
    e.src[:len(src)] = list(src)
    e.dst[:len(dst)] = list(dst)
    return e


def inner4(rng, ihl, plen, dst=None, df=None, tos=None, proto=None, fold_ffff=False, total=None):
    """A cleartext IPv4 packet of ihl dwords of header (random options) and
    plen payload bytes; ip_len and ip_sum as ip_output may leave them before
    the IPsec hook: stale.  fold_ffff: the header's 16-bit words will sum to
    0xffff once ip_len = `total` and ip_p = 50 are in and the checksum field
    is zero, so the field ends as 0."""
    off = (int(rng.integers(4)) << 14 if df is None else (0x4000 if df else 0))
    h = bytearray(struct.pack(">BBHHHBBH4s4s", 0x40 | ihl, int(rng.integers(256)) if tos is None else tos,
                              int(rng.integers(65536)), int(rng.integers(65536)), off & 0x4000,
                              int(rng.integers(1, 256)), int(rng.choice([6, 17, 1, 47])) if proto is None else proto,
                              int(rng.integers(65536)), addr(rng, False), dst or addr(rng, False)) +
                  rng.integers(0, 256, ihl * 4 - 20, dtype=np.uint8).tobytes())
    if fold_ffff:
        t = bytearray(h)
        t[2:4], t[9], t[10:12], t[4:6] = struct.pack(">H", total), 50, b"\0\0", b"\0\0"
        h[4:6] = struct.pack(">H", E.in_cksum(bytes(t)))      # the id field absorbs the rest
    return bytes(h) + rng.integers(0, 256, plen, dtype=np.uint8).tobytes()


def inner6(rng, plen, dst=None, tc=None, nxt=None):
    tc = int(rng.integers(256)) if tc is None else tc
    return (struct.pack(">IHBB", 0x60000000 | tc << 20 | int(rng.integers(1 << 20)), int(rng.integers(65536)),
                        int(rng.choice([6, 17, 58, 0, 43])) if nxt is None else nxt, int(rng.integers(1, 256))) +
            addr(rng, True) + (dst or addr(rng, True)) + rng.integers(0, 256, plen, dtype=np.uint8).tobytes())


def reference(e, ivlen, blks, alen, pkt, headroom, tailroom, ip_id):
    """esp.ipsec_output_encap for an L.EncSA with usable flags."""
    tunnel, af6, dfbit, ecn, rfc = flags_policy(e.flags)
    return E.ipsec_output_encap(tunnel, af6, bytes(e.src), bytes(e.dst), e.ttl, dfbit, ecn, rfc, ivlen, blks, alen,
                                pkt, headroom, tailroom, ip_id)


def check_one(rng, e, ivlen, blks, alen, pkt, headroom=None, tailroom=None, ip_id=0x1234, want=None):
    """One packet through espgpu_esp_encap against esp.ipsec_output_encap, in
    a buffer of guard bytes, headroom, the packet, tailroom, guard bytes: the
    status, the four results, and every byte of the buffer (the wire packet's
    defined bytes as the restatement has them, everything else as it was).
    Rooms left out are exactly what the packet needs.  `want`: the expected
    status where the restatement cannot express the input (unusable flags).
    Returns (status, front, wire bytes of the buffer or None)."""
    pkt = bytes(pkt)
    if want is None and (headroom is None or tailroom is None):
        st0, front0, wire0, _ = reference(e, ivlen, blks, alen, pkt, 1 << 20, 1 << 20, ip_id)
        need = (front0, len(wire0) - front0 - len(pkt)) if st0 == 0 else ROOM
        headroom = need[0] if headroom is None else headroom
        tailroom = need[1] if tailroom is None else tailroom
    elif headroom is None:
        headroom, tailroom = ROOM
    at = GUARD + headroom
    buf = bytearray(rng.integers(0, 256, at, dtype=np.uint8).tobytes() + pkt +
                    rng.integers(0, 256, tailroom + GUARD, dtype=np.uint8).tobytes())
    before = bytes(buf)
    sa0 = bytes(e)
    shape = L.EShape(ivlen, blks, alen)
    st, front, total, reclen, frame = E.esp_encap_host(e, shape, buf, at, len(pkt), headroom, tailroom, ip_id)
    ctx = (hex(e.flags), ivlen, blks, alen, len(pkt), headroom, tailroom)
    assert bytes(e) == sa0, ("the SA was written",) + ctx
    if want is None:
        want, wfront, wire, nxt = reference(e, ivlen, blks, alen, pkt, headroom, tailroom, ip_id)
    else:
        assert want != 0
    assert st == want, (st, want) + ctx
    if st:
        assert (front, total, reclen, frame) == (0, 0, 0, 0), ctx
        assert bytes(buf) == before, ("a refused packet was written",) + ctx
        return st, 0, None
    assert (front, total) == (wfront, len(wire)), (front, total, wfront, len(wire)) + ctx
    hlen = 8 + ivlen
    rlen = frame & 0xffff
    skip = 40 if pkt[0] >> 4 == 6 else (pkt[0] & 0xf) * 4
    assert frame >> 16 == nxt and reclen == total - (front - hlen or skip), ctx
    assert reclen == hlen + rlen + ((blks - ((rlen + 2) % blks)) % blks) + 2 + alen, ctx
    exp = bytearray(before)
    for k, b in enumerate(wire):
        if b is not None:
            exp[at - front + k] = b
    if bytes(buf) != bytes(exp):
        bad = [k - at for k in range(len(buf)) if buf[k] != exp[k]]
        raise AssertionError(("bytes differ at (relative to the packet)", bad[:16]) + ctx)
    return 0, front, bytes(buf[at - front:at - front + total])


def layout(rng, pkts, headroom, tailroom, max_gap4=5):
    """The packets in one arena of random bytes, each with its rooms and an
    irregular 4-byte-aligned gap to the next span: (arena, PKT_DTYPE array)."""
    offs, pos = [], 4 * int(rng.integers(0, max_gap4 + 1))
    for p in pkts:
        pos += headroom
        offs.append(pos)
        pos += ((len(p) + tailroom + 3) & ~3) + 4 * int(rng.integers(0, max_gap4 + 1))
    arena = rng.integers(0, 256, pos + 64, dtype=np.uint8)
    rec = np.zeros(len(pkts), dtype=PKT_DTYPE)
    for i, p in enumerate(pkts):
        arena[offs[i]:offs[i] + len(p)] = np.frombuffer(p, dtype=np.uint8)
        rec[i] = (offs[i] // 4, len(p))
    return arena, rec


def encsa_of(row):
    e = L.EncSA(int(row["bytes"]), int(row["packets"]), int(row["flags"]), int(row["ttl"]))
    e.pad_[:] = [int(x) for x in row["pad_"]]
    e.src[:] = [int(x) for x in row["src"]]
    e.dst[:] = [int(x) for x in row["dst"]]
    return e


def host_encap_batch(arena, rec, sa, enc, shapes, headroom, tailroom, id0, frame0):
    """espgpu_esp_encap_batch's contract with the host rule, in index order.
    shapes[sa] is the L.EShape of the ESP session with that id under its outsa
    flags, None where the ctx has no such session.  Returns (arena, DESC desc,
    frame, PKT_DTYPE opkt, estatus); the inputs are not modified, and frame
    keeps frame0's words for the packets that are not accepted."""
    n = len(rec)
    res = bytearray(arena.tobytes())
    desc = np.zeros(n, dtype=DESC)
    frame = np.array(frame0[:n], dtype=np.uint32)
    opkt = np.zeros(n, dtype=PKT_DTYPE)
    est = np.zeros(n, dtype=np.uint8)
    es = [encsa_of(r) for r in enc]
    for i in range(n):
        o4, ln, s = int(rec["off4"][i]), int(rec["len"][i]), int(sa[i])
        desc[i], opkt[i], est[i] = (o4, 0, 0xffff, 0, 0), (o4, 0), EINVAL
        if s >= len(es) or s >= len(shapes) or shapes[s] is None:
            continue
        st, front, total, reclen, f = E.esp_encap_host(es[s], shapes[s], res, o4 * 4, ln, headroom, tailroom,
                                                       (id0 + i) & 0xffff)
        est[i] = st
        if st == 0:
            desc[i] = (o4 - front // 4 + (total - reclen) // 4, reclen, s, 0, 0)
            frame[i] = f
            opkt[i] = (o4 - front // 4, total)
    return np.frombuffer(bytes(res), dtype=np.uint8), desc, frame, opkt, est


def host_sent_batch(opkt, desc, status, enc):
    """espgpu_esp_sent_batch with the host rule: the ENCSA_DTYPE table after."""
    out = enc.copy()
    es = [encsa_of(r) for r in enc]
    for i in range(len(opkt)):
        s = int(desc["sa"][i])
        if s < len(es):
            assert E.esp_sent_host(es[s], int(status[i]), int(opkt["len"][i])) == 0
    for k, e in enumerate(es):
        out["bytes"][k], out["packets"][k] = np.uint64(e.bytes), np.uint64(e.packets)
    return out
