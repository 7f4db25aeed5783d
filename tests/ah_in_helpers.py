"""Shared by the inbound AH tests: IPv4 option areas of every kind the massage
distinguishes, AH packets of both families, one packet through both host rules
and ah.py's restatements of the reference, and the host rules applied to a
batch in index order."""
import hashlib
import hmac as pyhmac
import struct

import numpy as np

from decap_helpers import flags_mode
from espgpu import _lib as L
from espgpu import ah as A
from espgpu import esp as E
from espgpu.batch import INSA_DTYPE, PKT_DTYPE

EINVAL, EACCES, EMSGSIZE, EPFNOSUPPORT = L.EINVAL, L.EACCES, L.EMSGSIZE, L.EPFNOSUPPORT
SLOT = L.AH_SAVE_SLOT
GUARD = 32
MLENS = (12, 16, 24, 32)
KEEP = (0x82, 0x85, 0x86, 0x94, 0x95)
ZEROED = (0x83, 0x89, 0x44, 0x07, 0x88, 0x52)          # LSRR, SSRR, timestamp, RR, stream id, traceroute
HASH = {1: hashlib.sha1, 256: hashlib.sha256, 384: hashlib.sha384, 512: hashlib.sha512}


def ah_flags(mode=E.IPSEC_MODE_ANY, af6=False, keeptos=False):
    return ({E.IPSEC_MODE_ANY: 0, E.IPSEC_MODE_TRANSPORT: L.IN_TRANSPORT, E.IPSEC_MODE_TUNNEL: L.IN_TUNNEL}[mode] |
            (L.IN_AF6 if af6 else 0) | L.IN_AH | (L.IN_AH_KEEPTOS if keeptos else 0))


def good_options(rng, room, only=None):
    """`room` bytes of well-formed options: NOPs, kept and zeroed options with
    random bodies, and now and then an EOL with arbitrary bytes behind it.
    only: draw the option types from this tuple."""
    out = bytearray()
    while len(out) < room:
        left = room - len(out)
        r = rng.random()
        if left == 1 or r < 0.15:
            out.append(1)                                  # NOP
        elif r < 0.22:
            out.append(0)                                  # EOL: the rest is never looked at
            out += rng.integers(0, 256, left - 1, dtype=np.uint8).tobytes()
        else:
            kinds = only if only is not None else (KEEP if rng.random() < 0.5 else ZEROED)
            t = int(kinds[int(rng.integers(len(kinds)))])
            ln = int(rng.integers(2, min(left, 40) + 1))
            out += bytes([t, ln]) + rng.integers(0, 256, ln - 2, dtype=np.uint8).tobytes()
    return bytes(out)


def bad_options(rng, room, kind):
    """`room` (>= 4) bytes of options the loop refuses: `lone` an option type
    in the header's last byte, `len0` / `len1` an option length below 2,
    `past` an option that runs one byte past the header; each behind a
    well-formed front, with a kept or a zeroed type."""
    t = int((KEEP + ZEROED)[int(rng.integers(len(KEEP) + len(ZEROED)))])
    # past: two bytes left, the option says three
    tail = {"lone": bytes([t]), "len0": bytes([t, 0]), "len1": bytes([t, 1]), "past": bytes([t, 3])}[kind]
    f = bytearray()                                        # no EOL in front: the bad option must be reached
    while len(f) < room - len(tail):
        left = room - len(tail) - len(f)
        if left == 1 or rng.random() < 0.3:
            f.append(1)
        else:
            ln = int(rng.integers(2, left + 1))
            f += bytes([int(rng.choice(KEEP + ZEROED)), ln]) + rng.integers(0, 256, ln - 2, dtype=np.uint8).tobytes()
    return bytes(f) + tail


def ah_header(rng, nxt, mlen, af6, spi, seq, ah_len=None):
    """struct newah, a random ICV and the alignment padding: ah_hdrsiz bytes."""
    ahsize = A.ah_hdrsiz(mlen, af6)
    ln = (ahsize - 8) // 4 if ah_len is None else ah_len
    return (bytes([nxt, ln & 0xff]) + rng.integers(0, 256, 2, dtype=np.uint8).tobytes() + struct.pack(">II", spi, seq) +
            rng.integers(0, 256, ahsize - 12, dtype=np.uint8).tobytes())


def ah_packet4(rng, ihl, opts, nxt, mlen, q, spi=0x1234, seq=1, dst=None, src=None, ah_len=None, cut=0):
    """An IPv4 AH packet: header of ihl dwords with `opts`, the AH header, q
    payload bytes; `cut` bytes short of that.  Returns (bytes, skip)."""
    skip = ihl * 4
    body = ah_header(rng, nxt, mlen, False, spi, seq, ah_len) + rng.integers(0, 256, q, dtype=np.uint8).tobytes()
    body = body[:len(body) - cut]
    h = bytearray(struct.pack(">BBHHHBBH4s4s", 0x40 | ihl, int(rng.integers(1, 256)), (skip + len(body)) & 0xffff,
                              int(rng.integers(65536)), int(rng.choice([0, 0x4000])), int(rng.integers(1, 256)), 51, 0,
                              src if src is not None else rng.integers(1, 255, 4, dtype=np.uint8).tobytes(),
                              dst if dst is not None else rng.integers(1, 255, 4, dtype=np.uint8).tobytes()) +
                  bytes(opts))
    assert len(h) == skip
    h[10:12] = struct.pack(">H", E.in_cksum(bytes(h)))
    return bytes(h) + body, skip


def ah_packet6(rng, nxt, mlen, q, spi=0x1234, seq=1, dst=None, src=None, ah_len=None, cut=0, plen=None):
    body = ah_header(rng, nxt, mlen, True, spi, seq, ah_len) + rng.integers(0, 256, q, dtype=np.uint8).tobytes()
    body = body[:len(body) - cut]
    if src is None:
        src = bytes([0x20, 0x01]) + rng.integers(0, 256, 14, dtype=np.uint8).tobytes()
    if dst is None:
        dst = bytes([0x20, 0x02]) + rng.integers(0, 256, 14, dtype=np.uint8).tobytes()
    return struct.pack(">IHBB", 0x60000000 | int(rng.integers(1, 1 << 28)), len(body) if plen is None else plen, 51,
                       int(rng.integers(1, 256))) + bytes(src) + bytes(dst) + body, 40


def sign(pkt, skip, mlen, key, sha, af6, esn_hi=None, cleartos=True):
    """The packet with the ICV a sender computes: HMAC (hashlib) over the
    packet as ah_input massages it, the ICV field zeroed, and for an ESN SA
    the high sequence word behind it."""
    st, massaged, _ = A.ah_input(af6, mlen, pkt, skip, cleartos)
    assert st == 0
    m = bytearray(massaged)
    m[skip + 12:skip + 12 + mlen] = bytes(mlen)
    msg = bytes(m) + (struct.pack(">I", esn_hi) if esn_hi is not None else b"")
    icv = pyhmac.new(key, msg, HASH[sha]).digest()[:mlen]
    return pkt[:skip + 12] + icv + pkt[skip + 12 + mlen:]


def check_input(rng, flags, mlen, pkt, skip, want=None, length=None):
    """One packet through espgpu_ah_input, in a buffer with guard bytes around
    it, against ah.ah_input: status, the packet's bytes, every other byte of
    the buffer, and the save slot.  `want`: the expected status where the
    restatement cannot express the input (unusable flags).  Returns (status,
    packet after, slot)."""
    pkt = bytes(pkt)
    length = len(pkt) if length is None else length
    buf = bytearray(rng.integers(0, 256, GUARD, dtype=np.uint8).tobytes() + pkt +
                    rng.integers(0, 256, GUARD, dtype=np.uint8).tobytes())
    before = bytes(buf)
    slot0 = rng.integers(0, 256, SLOT, dtype=np.uint8).tobytes()
    slot = bytearray(slot0)
    insa = L.InSA(7, 9, flags, 0x5a5a5a5a)
    st = A.ah_input_host(insa, mlen, buf, length, skip + 12, slot, at=GUARD)
    if want is None:
        _, af6, _ = flags_mode(flags & 0xf)
        want, massaged, saved = A.ah_input(af6, mlen, pkt[:length], skip, not flags & L.IN_AH_KEEPTOS)
    else:
        assert want != 0
    ctx = (hex(flags), mlen, skip, length, pkt[:skip + 12].hex())
    assert st == want, (st, want) + ctx
    assert (insa.bytes, insa.packets, insa.flags, insa.pad_) == (7, 9, flags, 0x5a5a5a5a)
    if st:
        assert bytes(buf) == before, ("a refused packet was written",) + ctx
        assert bytes(slot) == slot0, ("a refused packet's save slot was written",) + ctx
        return st, pkt, bytes(slot)
    assert bytes(buf[GUARD:GUARD + length]) == massaged, ("massaged packet",) + ctx
    assert massaged[skip:] == pkt[skip:length], "the AH header or the payload changed"
    assert bytes(buf[:GUARD]) == before[:GUARD] and bytes(buf[GUARD + length:]) == before[GUARD + length:], ctx
    assert bytes(slot[:skip]) == saved == pkt[:skip] and bytes(slot[skip:]) == slot0[skip:], ("save slot",) + ctx
    return 0, bytes(buf[GUARD:GUARD + length]), bytes(slot)


def check_decap(rng, flags, mlen, pkt, slot, skip, bytes0=0, packets0=0, want=None):
    """One packet as espgpu_ah_input left it through espgpu_ah_decap against
    ah.ah_input_cb_decap: status, result, the resulting packet's bytes, every
    other byte of the buffer, the slot unchanged and the SA's counters."""
    pkt = bytes(pkt)
    buf = bytearray(rng.integers(0, 256, GUARD, dtype=np.uint8).tobytes() + pkt +
                    rng.integers(0, 256, GUARD, dtype=np.uint8).tobytes())
    before = bytes(buf)
    hs = bytearray(slot)
    insa = L.InSA(bytes0, packets0, flags, 0x5a5a5a5a)
    st, off, ln = A.ah_decap_host(insa, mlen, buf, len(pkt), skip + 12, hs, at=GUARD)
    if want is None:
        mode, af6, _ = flags_mode(flags & 0xf)
        want, res, booked = A.ah_input_cb_decap(mode, af6, mlen, pkt, bytes(slot[:skip]), skip)
    else:
        assert want != 0
        res, booked = None, 0
    ctx = (hex(flags), mlen, skip, len(pkt))
    assert st == want, (st, want) + ctx
    assert bytes(hs) == bytes(slot) and (insa.flags, insa.pad_) == (flags, 0x5a5a5a5a)
    if st:
        assert (off, ln) == (0, 0), ctx
        assert bytes(buf) == before, ("a refused packet was written",) + ctx
        assert (insa.bytes, insa.packets) == (bytes0, packets0), ctx
        return st, None
    assert ln == len(res) == booked, (ln, len(res), booked) + ctx
    a = GUARD + off
    assert bytes(buf[a:a + ln]) == res, ("resulting packet", off, ln) + ctx
    assert bytes(buf[:a]) == before[:a] and bytes(buf[a + ln:]) == before[a + ln:], ("outside the result",) + ctx
    assert insa.bytes == (bytes0 + booked) & (2**64 - 1) and insa.packets == packets0 + 1, ctx
    return 0, (off, res)


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


def _insa_list(insa):
    return [L.InSA(int(e["bytes"]), int(e["packets"]), int(e["flags"]), int(e["pad_"])) for e in insa]


def host_ah_input_batch(arena, desc, insa, mlens, hsave):
    """espgpu_ah_input_batch's contract with the host rule, in index order.
    mlens[sa] is the ICV length of the DIGEST session with that id, None
    where the ctx holds no such session.  Returns (arena, desc, hsave,
    astatus); the inputs are not modified."""
    n = len(desc)
    res, d, hs = arena.copy(), desc.copy(), hsave.copy()
    ast = np.zeros(n, dtype=np.uint8)
    ins = _insa_list(insa)
    for i in range(n):
        sa, ln = int(d["sa"][i]), int(d["len"][i])
        if ln == 0 or sa >= len(ins) or sa >= len(mlens) or mlens[sa] is None:
            continue
        o = int(d["off4"][i]) * 4
        buf = bytearray(res[o:o + ln].tobytes())
        slot = bytearray(hs[i * SLOT:(i + 1) * SLOT].tobytes())
        st = A.ah_input_host(ins[sa], mlens[sa], buf, ln, int(d["salt"][i]), slot)
        ast[i] = st
        if st:
            d["len"][i] = 0
        res[o:o + ln] = np.frombuffer(bytes(buf), dtype=np.uint8)
        hs[i * SLOT:(i + 1) * SLOT] = np.frombuffer(bytes(slot), dtype=np.uint8)
    return res, d, hs, ast


def host_ah_decap_batch(arena, desc, status, insa, mlens, esp, hsave, ipkt0):
    """espgpu_ah_decap_batch's contract with the host rule, in index order.
    esp[sa]: the ctx holds an ESP session with that id.  ipkt0 is d_ipkt as the
    call finds it (an ESP record's entry stays).  Returns (arena, ipkt,
    dstatus, insa)."""
    n = len(desc)
    res, ipkt = arena.copy(), ipkt0.copy()
    dst = np.zeros(n, dtype=np.uint8)
    ins = _insa_list(insa)
    for i in range(n):
        o4, sa, ln = int(desc["off4"][i]), int(desc["sa"][i]), int(desc["len"][i])
        if status[i]:
            ipkt[i] = (o4, 0)
            continue
        if sa < len(esp) and esp[sa]:
            continue
        ipkt[i] = (o4, 0)
        dst[i] = EINVAL
        if sa >= len(ins) or sa >= len(mlens) or mlens[sa] is None or ln == 0:
            continue
        o = o4 * 4
        buf = bytearray(res[o:o + ln].tobytes())
        slot = bytearray(hsave[i * SLOT:(i + 1) * SLOT].tobytes())
        st, off, out_len = A.ah_decap_host(ins[sa], mlens[sa], buf, ln, int(desc["salt"][i]), slot)
        dst[i] = st
        if st == 0:
            ipkt[i] = (o4 + off // 4, out_len)
            res[o:o + ln] = np.frombuffer(bytes(buf), dtype=np.uint8)
    got = np.zeros(len(ins), dtype=INSA_DTYPE)
    for k, s in enumerate(ins):
        got[k] = (s.bytes, s.packets, s.flags, s.pad_)
    return res, ipkt, dst, got
