"""Shared by the outbound AH tests: cleartext packets with well-formed or
refused IPv4 options, AH SAs' outbound policies, one packet through the host
rules and ah.py's restatements of the reference, and the host rules applied to
a batch in index order."""
import struct

import numpy as np

import ah_in_helpers as H
from encap_helpers import addr, enc_flags, encsa_of, flags_policy
from espgpu import _lib as L
from espgpu import ah as A
from espgpu import esp as E
from espgpu.batch import PKT_DTYPE
from helpers import DESC

EINVAL, EACCES, ENOTSUP, EMSGSIZE, EAFNOSUPPORT, ENOBUFS = (L.EINVAL, L.EACCES, L.ENOTSUP, L.EMSGSIZE,
                                                            L.EAFNOSUPPORT, L.ENOBUFS)
SLOT = L.AH_SAVE_SLOT
GUARD = 32
MLENS = (12, 16, 24, 32)
ROOM = 12 + 64 + 40                 # the most any SA asks for: ahsize + oh


def ah_enc_flags(keeptos=False, **kw):
    return enc_flags(**kw) | L.ENC_AH | (L.ENC_AH_KEEPTOS if keeptos else 0)


def clear4(rng, ihl, opts, plen, dst=None, src=None, tos=None, df=None, proto=None, consistent=True):
    """A cleartext IPv4 packet: ihl dwords of header with the option bytes
    `opts`, plen payload bytes.  consistent: ip_len and ip_sum are right."""
    skip = ihl * 4
    assert len(opts) == skip - 20
    off = int(rng.integers(2)) << 14 if df is None else (0x4000 if df else 0)
    h = bytearray(struct.pack(">BBHHHBBH4s4s", 0x40 | ihl, int(rng.integers(1, 256)) if tos is None else tos,
                              skip + plen if consistent else int(rng.integers(65536)), int(rng.integers(65536)), off,
                              int(rng.integers(1, 256)), int(rng.choice([6, 17, 1, 47])) if proto is None else proto,
                              0, src or addr(rng, False), dst or addr(rng, False)) + bytes(opts))
    h[10:12] = struct.pack(">H", E.in_cksum(bytes(h)) if consistent else int(rng.integers(65536)))
    return bytes(h) + rng.integers(0, 256, plen, dtype=np.uint8).tobytes()


def clear6(rng, plen, dst=None, src=None, tc=None, nxt=None, consistent=True):
    tc = int(rng.integers(256)) if tc is None else tc
    return (struct.pack(">IHBB", 0x60000000 | tc << 20 | int(rng.integers(1 << 20)),
                        plen if consistent else int(rng.integers(65536)),
                        int(rng.choice([6, 17, 58, 50])) if nxt is None else nxt, int(rng.integers(1, 256))) +
            (src or addr(rng, True)) + (dst or addr(rng, True)) + rng.integers(0, 256, plen, dtype=np.uint8).tobytes())


def sr_lengths(opts):
    """The lengths of the LSRR / SSRR options that the walk over the
    well-formed option bytes meets."""
    off, out = 0, []
    while off < len(opts) and opts[off] != 0:
        if opts[off] == 1:
            off += 1
            continue
        if opts[off] in (0x83, 0x89):
            out.append(opts[off + 1])
        off += opts[off + 1]
    return out


def short_sr(opts):
    return any(ln < 4 for ln in sr_lengths(opts))


def good_options(rng, room, sr_ok=True):
    """ah_in_helpers.good_options without the source-route options that only
    the outbound rule refuses; sr_ok False: without any."""
    while True:
        o = H.good_options(rng, room)
        if not (short_sr(o) if sr_ok else sr_lengths(o)):
            return o


def sr_option(rng, typ, ln):
    """An LSRR / SSRR option of `ln` bytes."""
    return bytes([typ, ln]) + rng.integers(1, 255, ln - 2, dtype=np.uint8).tobytes()


def reference(e, mlen, pkt, headroom, ip_id):
    """The restatement for an L.EncSA with usable flags: (status, front, the
    hashed packet as a list with None for the SPI, the sequence number and the
    ICV field, the saved wire header, hs, nxt)."""
    tunnel, af6, dfbit, ecn, rfc = flags_policy(e.flags & ~(L.ENC_AH | L.ENC_AH_KEEPTOS))
    st, front, wire, hs, nxt = A.ipsec_output_encap_ah(tunnel, af6, bytes(e.src), bytes(e.dst), e.ttl, dfbit, ecn, rfc,
                                                       mlen, pkt, headroom, ip_id)
    if st:
        return st, 0, None, None, 0, 0
    st, hashed, saved = A.ah_output(af6, wire, hs, not e.flags & L.ENC_AH_KEEPTOS)
    if st:
        return st, 0, None, None, 0, 0
    return 0, front, hashed, saved, hs, nxt


def check_encap(rng, e, mlen, pkt, headroom=None, ip_id=0x1234, want=None):
    """One packet through espgpu_ah_encap against the restatement, in a buffer
    of guard bytes, headroom, the packet, guard bytes: the status, the three
    results, every byte of the buffer (the wire packet's defined bytes as the
    restatement has them, everything else as it was) and the save slot byte
    for byte.  headroom left out is exactly what the packet needs.  `want`: the
    expected status where the restatement cannot express the input.  Returns
    (status, front, hashed packet bytes of the buffer or None, slot, hs)."""
    pkt = bytes(pkt)
    if headroom is None:
        headroom = ROOM
        if want is None:
            st0, front0 = reference(e, mlen, pkt, 1 << 20, ip_id)[:2]
            headroom = front0 if st0 == 0 else ROOM
    at = GUARD + headroom
    buf = bytearray(rng.integers(0, 256, at, dtype=np.uint8).tobytes() + pkt +
                    rng.integers(0, 256, GUARD, dtype=np.uint8).tobytes())
    before = bytes(buf)
    slot0 = rng.integers(0, 256, SLOT, dtype=np.uint8).tobytes()
    slot = bytearray(slot0)
    sa0 = bytes(e)
    st, front, total, salt = A.ah_encap_host(e, mlen, buf, at, len(pkt), headroom, ip_id, slot)
    ctx = (hex(e.flags), mlen, len(pkt), headroom, pkt[:60].hex())
    assert bytes(e) == sa0, ("the SA was written",) + ctx
    if want is None:
        want, wfront, hashed, saved, hs, nxt = reference(e, mlen, pkt, headroom, ip_id)
    else:
        assert want != 0
    assert st == want, (st, want) + ctx
    if st:
        assert (front, total, salt) == (0, 0, 0), ctx
        assert bytes(buf) == before, ("a refused packet was written",) + ctx
        assert bytes(slot) == slot0, ("a refused packet's save slot was written",) + ctx
        return st, 0, None, bytes(slot), 0
    assert (front, total, salt) == (wfront, len(hashed), hs + 12), (front, total, salt, wfront, len(hashed), hs) + ctx
    exp = bytearray(before)
    for k, b in enumerate(hashed):
        if b is not None:
            exp[at - front + k] = b
    if bytes(buf) != bytes(exp):
        bad = [k - at for k in range(len(buf)) if buf[k] != exp[k]]
        raise AssertionError(("bytes differ at (relative to the packet)", bad[:16]) + ctx)
    assert bytes(slot[:hs]) == saved and bytes(slot[hs:]) == slot0[hs:], ("save slot",) + ctx
    assert buf[at - front + hs] == nxt
    return 0, front, bytes(buf[at - front:at - front + total]), bytes(slot), hs


def layout(rng, pkts, headroom, max_gap4=5):
    """The packets in one arena of random bytes, each with its headroom and an
    irregular 4-byte-aligned gap to the next span: (arena, PKT_DTYPE array)."""
    offs, pos = [], 4 * int(rng.integers(0, max_gap4 + 1))
    for p in pkts:
        pos += headroom
        offs.append(pos)
        pos += ((len(p) + 3) & ~3) + 4 * int(rng.integers(0, max_gap4 + 1))
    arena = rng.integers(0, 256, pos + 64, dtype=np.uint8)
    rec = np.zeros(len(pkts), dtype=PKT_DTYPE)
    for i, p in enumerate(pkts):
        arena[offs[i]:offs[i] + len(p)] = np.frombuffer(p, dtype=np.uint8)
        rec[i] = (offs[i] // 4, len(p))
    return arena, rec


def host_encap_batch(arena, rec, sa, enc, mlens, headroom, id0, hsave):
    """espgpu_ah_encap_batch's contract with the host rule, in index order.
    mlens[sa] is the ICV length of the DIGEST session with that id, None where
    the ctx holds no such session.  Returns (arena, DESC desc, PKT_DTYPE opkt,
    estatus, hsave); the inputs are not modified."""
    n = len(rec)
    res = bytearray(arena.tobytes())
    hs = bytearray(hsave.tobytes())
    desc = np.zeros(n, dtype=DESC)
    opkt = np.zeros(n, dtype=PKT_DTYPE)
    est = np.zeros(n, dtype=np.uint8)
    es = [encsa_of(r) for r in enc]
    for i in range(n):
        o4, ln, s = int(rec["off4"][i]), int(rec["len"][i]), int(sa[i])
        desc[i], opkt[i], est[i] = (o4, 0, 0xffff, 0, 0), (o4, 0), EINVAL
        if s >= len(es) or s >= len(mlens) or mlens[s] is None:
            continue
        slot = bytearray(hs[i * SLOT:(i + 1) * SLOT])
        st, front, total, salt = A.ah_encap_host(es[s], mlens[s], res, o4 * 4, ln, headroom, (id0 + i) & 0xffff, slot)
        hs[i * SLOT:(i + 1) * SLOT] = slot
        est[i] = st
        if st == 0:
            desc[i] = (o4 - front // 4, total, s, 0, salt)
            opkt[i] = (o4 - front // 4, total)
    return (np.frombuffer(bytes(res), dtype=np.uint8), desc, opkt, est, np.frombuffer(bytes(hs), dtype=np.uint8))


def outsa_of(row):
    return L.OutSA(int(row["count"]), int(row["cntr"]), int(row["spi"]), int(row["salt"]), int(row["flags"]),
                   int(row["pad_"]))


def host_frame_batch(arena, desc, outsa, digest):
    """espgpu_ah_frame_batch's contract with the host rule, in index order.
    digest[sa]: the ctx holds a DIGEST session with that id.  Returns (arena,
    desc, fstatus, outsa)."""
    n = len(desc)
    res = bytearray(arena.tobytes())
    d = desc.copy()
    fst = np.zeros(n, dtype=np.uint8)
    os_ = [outsa_of(r) for r in outsa]
    for i in range(n):
        s, ln, salt = int(d["sa"][i]), int(d["len"][i]), int(d["salt"][i])
        st = EINVAL
        if ln and s < len(os_) and s < len(digest) and digest[s] and 12 <= salt <= ln and salt % 4 == 0:
            st, hi = A.ah_frame_host(os_[s], res, int(d["off4"][i]) * 4, ln, salt, int(d["esn_hi"][i]))
            d["esn_hi"][i] = hi
        fst[i] = st
        if st:
            d["len"][i] = 0
    out = outsa.copy()
    for k, o in enumerate(os_):
        out[k] = (o.count, o.cntr, o.spi, o.salt, o.flags, o.pad_)
    return np.frombuffer(bytes(res), dtype=np.uint8), d, fst, out


def host_sent_batch(arena, opkt, desc, status, enc, digest, hsave):
    """espgpu_ah_sent_batch's contract with the host rule.  Returns (arena,
    ENCSA_DTYPE table, sstatus)."""
    n = len(desc)
    res = bytearray(arena.tobytes())
    sst = np.zeros(n, dtype=np.uint8)
    es = [encsa_of(r) for r in enc]
    for i in range(n):
        s = int(desc["sa"][i])
        if status[i] or s >= len(es) or s >= len(digest) or not digest[s]:
            continue
        slot = bytearray(hsave[i * SLOT:(i + 1) * SLOT].tobytes())
        sst[i] = A.ah_sent_host(es[s], 0, res, int(opkt["off4"][i]) * 4, int(opkt["len"][i]), int(desc["salt"][i]),
                                slot)
    out = enc.copy()
    for k, e in enumerate(es):
        out["bytes"][k], out["packets"][k] = np.uint64(e.bytes), np.uint64(e.packets)
    return np.frombuffer(bytes(res), dtype=np.uint8), out, sst
