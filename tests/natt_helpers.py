"""Shared by the NAT-T tests: UDP-encapsulated ESP packets of every kind the
classification rule distinguishes, an SADB whose IPv4 ESP SAs are partly NAT-T
ones, decapsulated transport packets for the checksum fix, and the host rules
applied to a batch."""
import struct

import numpy as np

from espgpu import _lib as L
from espgpu import esp as E
from espgpu.batch import INSA_DTYPE, PKT_DTYPE
import classify_helpers as CH
import decap_helpers as DH

EINVAL, ENOTSUP, ENOENT = L.EINVAL, L.ENOTSUP, L.ENOENT
PORT = 4500


class NattSadb(CH.Sadb):
    """CH.Sadb with every second IPv4 ESP SA a NAT-T one (distinct port pairs);
    ref carries the sixth member esp.ipsec_input_classify_natt reads."""

    def __init__(self, rng, **kw):
        super().__init__(rng, **kw)
        k = 0
        for e in self.entries:
            if e["proto"] == 50 and e["af"] == 4:
                k += 1
                if k & 1:
                    sport, dport = 1024 + 7 * k, PORT if k & 2 else 4501 + k
                    e["flags"] = L.SAD_NATT
                    e["dst"][4:8] = np.frombuffer(struct.pack(">HH", sport, dport), dtype=np.uint8)
        self.ref = {int(e["spi"]): (int(e["sa"]), int(e["proto"]), int(e["af"]), bytes(e["dst"]), int(e["salt"]),
                                    ports_of(e)) for e in self.entries}

    def pick_natt(self, rng, natt=True):
        c = [e for e in self.entries if e["proto"] == 50 and e["af"] == 4 and bool(e["flags"] & L.SAD_NATT) == natt]
        return c[int(rng.integers(len(c)))]


def ports_of(e):
    """(sport, dport) of a NAT-T SAD entry, None for a plain one."""
    return struct.unpack(">HH", bytes(e["dst"][4:8])) if e["flags"] & L.SAD_NATT else None


def udp4(dst, sport, dport, payload, ihl=5, ulen=None, uh_sum=0, ip_len=None, off=0, tail=b"", opts=None):
    """An IPv4 datagram: UDP header (uh_ulen = 8 + len(payload) unless given), payload."""
    ulen = 8 + len(payload) if ulen is None else ulen
    return CH.ipv4(dst, struct.pack(">HHHH", sport, dport, ulen & 0xffff, uh_sum) + bytes(payload), ihl=ihl, proto=17,
                   ip_len=ip_len, off=off, tail=tail, opts=opts)


def _esp(rng, e, n=None):
    return CH.esp_payload(rng, int(e["spi"]), 8 + 4 * int(rng.integers(0, 40)) if n is None else n)


def _port_entry(rng, db, port):
    """A NAT-T entry whose dport is the configured port."""
    c = [e for e in db.entries if e["flags"] & L.SAD_NATT and ports_of(e)[1] == port]
    return c[int(rng.integers(len(c)))]


def natt_packet(rng, db, port, kind):
    """One packet of `kind` addressed to `port`; every kind starts from a good
    packet of an SA whose dport is `port` and breaks one thing."""
    e = _port_entry(rng, db, port)
    sport, dport = ports_of(e)
    dst = CH.dst_of(e)
    ihl = int(rng.integers(5, 16))
    good = _esp(rng, e)
    if kind == "good":
        return udp4(dst, sport, dport, good, ihl=ihl)
    if kind == "trim":                                 # uh_ulen shorter than ip_len - hlen: the surplus is ignored
        return udp4(dst, sport, dport, good + bytes(int(rng.integers(1, 9))), ihl=ihl, ulen=8 + len(good))
    if kind == "tail":                                 # bytes past ip_len
        return udp4(dst, sport, dport, good, ihl=ihl, tail=bytes(int(rng.integers(1, 20))))
    if kind == "noudp":                                # ip_len - hlen < 8
        return CH.ipv4(dst, bytes(int(rng.integers(0, 8))), ihl=ihl, proto=17)
    if kind == "otherport":
        return udp4(dst, sport, port ^ (1 << int(rng.integers(16))), good, ihl=ihl)
    if kind == "ulen_small":
        return udp4(dst, sport, dport, good, ihl=ihl, ulen=int(rng.integers(0, 8)))
    if kind == "ulen_big":
        return udp4(dst, sport, dport, good, ihl=ihl, ulen=8 + len(good) + int(rng.integers(1, 9)))
    if kind == "sum":
        return udp4(dst, sport, dport, good, ihl=ihl, uh_sum=int(rng.integers(1, 65536)))
    if kind == "keepalive":
        return udp4(dst, sport, dport, b"\xff", ihl=ihl)
    if kind == "short_esp":                            # ulen - 8 in 0..7
        return udp4(dst, sport, dport, good[:int(rng.integers(0, 8))], ihl=ihl)
    if kind == "ike":                                  # the non-ESP marker
        return udp4(dst, sport, dport, bytes(4) + good[4:], ihl=ihl)
    if kind == "unaligned":
        return udp4(dst, sport, dport, good + bytes(int(rng.integers(1, 4))), ihl=ihl)
    if kind == "unknown":
        return udp4(dst, sport, dport, CH.esp_payload(rng, db.unknown_spi(rng), 24), ihl=ihl)
    if kind == "wrongdst":
        d = bytearray(dst)
        d[int(rng.integers(4))] ^= 1 << int(rng.integers(8))
        return udp4(d, sport, dport, good, ihl=ihl)
    if kind == "plain_sa":                             # UDP-encapsulated, but the SA has no natt
        p = db.pick_natt(rng, natt=False)
        return udp4(CH.dst_of(p), sport, dport, _esp(rng, p), ihl=ihl)
    if kind == "sport":
        return udp4(dst, sport ^ (1 << int(rng.integers(16))), dport, good, ihl=ihl)
    if kind == "dport":                                # an SA whose natt->dport is not the socket's port
        c = [x for x in db.entries if x["flags"] & L.SAD_NATT and ports_of(x)[1] != port]
        x = c[int(rng.integers(len(c)))]
        return udp4(CH.dst_of(x), ports_of(x)[0], port, _esp(rng, x), ihl=ihl)
    if kind == "frag":
        return udp4(dst, sport, dport, good, ihl=ihl, off=int(rng.choice([0x2000, 0x0001, 0x1fff])))
    if kind == "esp_natt_sa":                          # plain ip_p 50 for a NAT-T SA: the host's
        return CH.ipv4(dst, good, ihl=ihl)
    raise KeyError(kind)


# kind -> status with the port set, in the header's check order; the first three are accepted
NATT_KINDS = {
    "good": 0, "trim": 0, "tail": 0,
    "noudp": ENOTSUP, "otherport": ENOTSUP, "ulen_small": EINVAL, "ulen_big": EINVAL, "sum": ENOTSUP,
    "keepalive": ENOTSUP, "short_esp": ENOTSUP, "ike": ENOTSUP, "unaligned": EINVAL, "unknown": ENOENT,
    "wrongdst": ENOENT, "plain_sa": ENOENT, "sport": ENOENT, "dport": ENOENT, "frag": ENOTSUP,
    "esp_natt_sa": ENOTSUP,
}


def in_flags(mode, prand=False):
    return DH.in_flags(mode, False, prand) | L.IN_NATT


def natt_in_packet(rng, ivlen, alen, q, nxt, ihl=5, padlen=None, sport=4500, dport=4500, **kw):
    """(IP header + UDP header + decrypted record, skip, rlen) as the decrypt
    leaves a UDP-encapsulated packet: skip covers the UDP header."""
    if padlen is None:
        padlen = int(rng.integers(0, 12))
    rec = DH.record(rng, ivlen, alen, q, padlen, nxt)
    hdr = DH.outer4(rng, ihl, ihl * 4 + 8 + len(rec), proto=17, **kw)
    return hdr + struct.pack(">HHHH", sport, dport, 8 + len(rec), 0) + rec, ihl * 4 + 8, len(rec)


def host_decap_batch(arena, out, rec, desc, trailer, status, insa, shapes):
    """DH.host_decap_batch for batches with NAT-T SAs: skip up to 68, and the
    header of a transport result copied wherever the rule put it."""
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
        assert 0 <= skip < 72
        o = o4 * 4
        tmp = bytearray(arena[o:o + skip].tobytes() + res[o + skip:o + skip + rlen].tobytes())
        st, off, ln = E.esp_decap_host(ins[sa], DH.shape_of(ivlen, alen), tmp, skip, rlen, int(trailer[i]))
        dst[i] = st
        if st == 0:
            ipkt[i] = (o4 + off // 4, ln)
            if off != skip + 8 + ivlen:                              # transport: the header moved
                u = 8 if ins[sa].flags & L.IN_NATT else 0
                res[o + off:o + off + skip - u] = np.frombuffer(bytes(tmp[off:off + skip - u]), dtype=np.uint8)
    got = np.zeros(len(ins), dtype=INSA_DTYPE)
    for k, s in enumerate(ins):
        got[k] = (s.bytes, s.packets, s.flags, s.pad_)
    return res, ipkt, dst, got


# ---- the checksum fix ---------------------------------------------------------
def tpacket(rng, proto, seglen, ihl=5, ulen=None, field=None, ip_len=None):
    """A decapsulated IPv4 packet: ihl dwords of header with a right checksum,
    then seglen random bytes as the TCP / UDP segment.  UDP: uh_ulen = seglen
    unless given; field: the checksum field's value as a little-endian load."""
    total = ihl * 4 + seglen
    h = bytearray(DH.outer4(rng, ihl, total if ip_len is None else ip_len, proto=proto))
    seg = bytearray(rng.integers(0, 256, seglen, dtype=np.uint8).tobytes())
    if proto == 17 and seglen >= 6:
        seg[4:6] = struct.pack(">H", (seglen if ulen is None else ulen) & 0xffff)
    off = 6 if proto == 17 else 16
    if field is not None and seglen >= off + 2:
        seg[off:off + 2] = struct.pack("<H", field)
    return bytes(h) + bytes(seg)


def force_result_zero(pkt, proto, at):
    """pkt with the two bytes at `at` (even, inside the summed segment, not the
    field) set so that the recomputed sum folds to 0xffff: the checksum comes
    out as 0x0000 (stored as 0xffff for UDP)."""
    m = bytearray(pkt)
    skip = (m[0] & 0xf) * 4
    m[at:at + 2] = b"\0\0"
    r, _ = E.udp_ipsec_adjust_cksum(bytes(m), 0, proto, skip, 1)
    off = skip + (6 if proto == 17 else 16)
    c = r[off:off + 2]
    if proto == 17 and c == b"\xff\xff":
        return None                                    # already there with the word as zero: cannot tell
    m[at:at + 2] = c                                   # S + ~S = 0xffff
    return bytes(m)


def host_natt_batch(out, ipkt, desc, trailer, status, dstatus, insa, policy):
    """espgpu_esp_natt_cksum_batch's contract with the host rule: (out, cflags)."""
    res = bytearray(out.tobytes())
    cf = np.zeros(len(ipkt), dtype=np.uint8)
    for i in range(len(ipkt)):
        sa = int(desc["sa"][i])
        if status[i] or dstatus[i] or sa >= len(insa):
            continue
        e = insa[sa]
        s = L.InSA(int(e["bytes"]), int(e["packets"]), int(e["flags"]), int(e["pad_"]))
        rc, c = E.esp_natt_cksum_host(s, res, int(ipkt["off4"][i]) * 4, int(ipkt["len"][i]), int(trailer[i]), policy)
        assert rc == 0
        cf[i] = c
    return np.frombuffer(bytes(res), dtype=np.uint8), cf
