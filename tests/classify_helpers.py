"""Shared by the classification tests: received packets of every kind the rule
distinguishes, a small SADB in the three forms the tests need (SAD_DTYPE
entries for espgpu_sad_build, the dict esp.ipsec_input_classify reads), and
the host rule applied to a batch."""
import struct

import numpy as np

from espgpu import _lib as L
from espgpu import esp as E
from espgpu import shard
from espgpu.batch import PKT_DTYPE, SAD_DTYPE
from helpers import DESC

EINVAL, ENOTSUP, ENOENT = L.EINVAL, L.ENOTSUP, L.ENOENT


def ipv4(dst, payload, ihl=5, proto=50, off=0, ip_len=None, opts=None, bad_sum=False, tail=b""):
    """An IPv4 packet: header of ihl dwords (options `opts` or zeros), the
    checksum right unless bad_sum, then payload and `tail` (bytes past ip_len)."""
    hlen = ihl * 4
    if ip_len is None:
        ip_len = hlen + len(payload)
    opts = bytes(max(hlen - 20, 0)) if opts is None else bytes(opts)
    h = bytearray(struct.pack(">BBHHHBBH4s4s", 0x40 | ihl, 0, ip_len & 0xffff, 0x1234, off, 64, proto, 0,
                              bytes([10, 0, 0, 1]), bytes(dst)) + opts)
    h[10:12] = struct.pack(">H", E.in_cksum(bytes(h)))
    if bad_sum:
        h[10] ^= 0x40
    return bytes(h) + bytes(payload) + bytes(tail)


def ipv6(dst, payload, nxt=50, plen=None, tail=b""):
    if plen is None:
        plen = len(payload)
    src = bytes([0x20, 0x01, 0x0d, 0xb8]) + bytes(11) + b"\x01"
    return struct.pack(">IHBB", 0x60000000, plen & 0xffff, nxt, 64) + src + bytes(dst) + bytes(payload) + bytes(tail)


def esp_payload(rng, spi, n):
    """n bytes of an ESP record: the SPI, then random bytes."""
    body = rng.integers(0, 256, max(n, 4), dtype=np.uint8).tobytes()
    return (struct.pack(">I", spi) + body)[:n]


class Sadb:
    """nesp4 / nesp6 ESP SAs and nah AH SAs (both families) with distinct SPIs
    and destinations; sa ids in insertion order from sa0."""

    def __init__(self, rng, nesp4=20, nesp6=16, nah=4, sa0=0, spis=None):
        n = nesp4 + nesp6 + nah
        spis = shard.random_spis(n, int(rng.integers(1, 2**31))) if spis is None else list(spis)
        order = rng.permutation(n)
        self.entries = np.zeros(n, dtype=SAD_DTYPE)
        for k, j in enumerate(order):
            af = 4 if j < nesp4 else 6 if j < nesp4 + nesp6 else (4, 6)[int(j) & 1]
            e = self.entries[k]
            e["spi"], e["sa"], e["af"] = spis[k], sa0 + k, af
            e["proto"] = 50 if j < nesp4 + nesp6 else 51
            e["salt"] = int(rng.integers(0, 2**32))
            dst = rng.integers(0, 256, 16, dtype=np.uint8)
            dst[0] = 0x20 if af == 6 else 10                     # not fe80::/10
            if af == 4:
                dst[4:] = 0
            e["dst"] = dst
        self.ref = {int(e["spi"]): (int(e["sa"]), int(e["proto"]), int(e["af"]), bytes(e["dst"]), int(e["salt"]))
                    for e in self.entries}

    def pick(self, rng, proto=50, af=None):
        c = [e for e in self.entries if e["proto"] == proto and (af is None or e["af"] == af)]
        return c[int(rng.integers(len(c)))]

    def unknown_spi(self, rng):
        while True:
            s = int(rng.integers(256, 2**32))
            if s not in self.ref:
                return s


def chain_spis(home, nslots, count, start=0x100):
    """The first `count` SPIs >= start whose home slot is `home` (as shard.spis_for_rank searches)."""
    out, s = [], start
    while len(out) < count:
        if shard.key_u32hash(s) & (nslots - 1) == home:
            out.append(s)
        s += 1
    return out


def dst_of(e):
    return bytes(e["dst"])[:4 if e["af"] == 4 else 16]


# kind -> (packet builder, the status the rule gives); the random draws mix them
def _good4(rng, db):
    e = db.pick(rng, af=4)
    ihl = int(rng.integers(5, 16))
    n = 8 + 4 * int(rng.integers(0, 40))
    opts = rng.integers(0, 256, ihl * 4 - 20, dtype=np.uint8).tobytes()
    return ipv4(dst_of(e), esp_payload(rng, int(e["spi"]), n), ihl=ihl, opts=opts)


def _good6(rng, db):
    e = db.pick(rng, af=6)
    return ipv6(dst_of(e), esp_payload(rng, int(e["spi"]), 8 + 4 * int(rng.integers(0, 40))))


def _tail4(rng, db):
    e = db.pick(rng, af=4)
    return ipv4(dst_of(e), esp_payload(rng, int(e["spi"]), 24), tail=rng.integers(0, 256, int(rng.integers(1, 30)),
                                                                                  dtype=np.uint8).tobytes())


def _tail6(rng, db):
    e = db.pick(rng, af=6)
    return ipv6(dst_of(e), esp_payload(rng, int(e["spi"]), 24), tail=bytes(int(rng.integers(1, 30))))


def _short(rng, db):
    return _good4(rng, db)[:int(rng.integers(0, 20))]


def _badver(rng, db):
    p = bytearray(_good4(rng, db))
    p[0] = (int(rng.choice([0, 1, 2, 3, 5, 7, 8, 15])) << 4) | (p[0] & 0xf)
    return bytes(p)


def _badihl(rng, db):
    e = db.pick(rng, af=4)
    p = bytearray(ipv4(dst_of(e), esp_payload(rng, int(e["spi"]), 24)))
    p[0] = 0x40 | int(rng.integers(0, 5))
    return bytes(p)


def _hlen_gt_len(rng, db):
    e = db.pick(rng, af=4)
    return ipv4(dst_of(e), b"", ihl=15, ip_len=60)[:int(rng.integers(20, 60))]


def _badsum(rng, db):
    e = db.pick(rng, af=4)
    return ipv4(dst_of(e), esp_payload(rng, int(e["spi"]), 24), ihl=int(rng.integers(5, 9)), bad_sum=True)


def _iplen_lt_hlen(rng, db):
    e = db.pick(rng, af=4)
    return ipv4(dst_of(e), esp_payload(rng, int(e["spi"]), 24), ihl=6, ip_len=int(rng.integers(0, 24)))


def _iplen_gt_len(rng, db):
    e = db.pick(rng, af=4)
    return ipv4(dst_of(e), esp_payload(rng, int(e["spi"]), 24), ip_len=44 + int(rng.integers(1, 2000)))


def _frag(rng, db):
    e = db.pick(rng, af=4)
    off = int(rng.choice([0x2000, 0x2001, 0x0001, 0x1fff, 0x00b9]))
    return ipv4(dst_of(e), esp_payload(rng, int(e["spi"]), 24), off=off | int(rng.choice([0, 0x4000])))


def _proto4(rng, db):
    e = db.pick(rng, af=4)
    return ipv4(dst_of(e), esp_payload(rng, int(e["spi"]), 24), proto=int(rng.choice([51, 108, 17, 6, 1, 4, 49])))


def _small4(rng, db):
    e = db.pick(rng, af=4)
    return ipv4(dst_of(e), esp_payload(rng, int(e["spi"]), int(rng.integers(0, 8))))


def _unaligned4(rng, db):
    e = db.pick(rng, af=4)
    return ipv4(dst_of(e), esp_payload(rng, int(e["spi"]), 24 + int(rng.integers(1, 4))))


def _unknown4(rng, db):
    return ipv4(dst_of(db.pick(rng, af=4)), esp_payload(rng, db.unknown_spi(rng), 24))


def _spi0(rng, db):
    return ipv4(dst_of(db.pick(rng, af=4)), esp_payload(rng, 0, 24))


def _ahspi(rng, db):
    e = db.pick(rng, proto=51)
    p = esp_payload(rng, int(e["spi"]), 24)
    return ipv4(dst_of(e), p) if e["af"] == 4 else ipv6(dst_of(e), p)


def _wrongdst4(rng, db):
    e = db.pick(rng, af=4)
    d = bytearray(dst_of(e))
    d[int(rng.integers(4))] ^= 1 << int(rng.integers(8))
    return ipv4(d, esp_payload(rng, int(e["spi"]), 24))


def _wrongdst6(rng, db):
    e = db.pick(rng, af=6)
    d = bytearray(dst_of(e))
    d[int(rng.integers(2, 16))] ^= 1 << int(rng.integers(8))
    return ipv6(d, esp_payload(rng, int(e["spi"]), 24))


def _wrongaf(rng, db):
    if rng.integers(2):
        e = db.pick(rng, af=6)                   # an IPv6 SA's SPI in an IPv4 packet to its first 4 bytes
        return ipv4(dst_of(e)[:4], esp_payload(rng, int(e["spi"]), 24))
    e = db.pick(rng, af=4)
    return ipv6(bytes(e["dst"]), esp_payload(rng, int(e["spi"]), 24))


def _short6(rng, db):
    return _good6(rng, db)[:int(rng.integers(20, 40))]


def _jumbo6(rng, db):
    e = db.pick(rng, af=6)
    return ipv6(dst_of(e), esp_payload(rng, int(e["spi"]), 24), plen=0)


def _plen_gt_len6(rng, db):
    e = db.pick(rng, af=6)
    return ipv6(dst_of(e), esp_payload(rng, int(e["spi"]), 24), plen=24 + int(rng.integers(1, 2000)))


def _nxt6(rng, db):
    e = db.pick(rng, af=6)
    return ipv6(dst_of(e), esp_payload(rng, int(e["spi"]), 24), nxt=int(rng.choice([0, 43, 44, 51, 60, 6, 17])))


def _linklocal6(rng, db):
    e = db.pick(rng, af=6)
    d = bytearray(dst_of(e))
    d[0], d[1] = 0xfe, 0x80 | int(rng.integers(0, 0x40))
    return ipv6(d, esp_payload(rng, int(e["spi"]), 24))


def _small6(rng, db):
    e = db.pick(rng, af=6)
    return ipv6(dst_of(e), esp_payload(rng, int(e["spi"]), int(rng.integers(1, 8))))


def _unaligned6(rng, db):
    e = db.pick(rng, af=6)
    return ipv6(dst_of(e), esp_payload(rng, int(e["spi"]), 24 + int(rng.integers(1, 4))))


def _unknown6(rng, db):
    return ipv6(dst_of(db.pick(rng, af=6)), esp_payload(rng, db.unknown_spi(rng), 24))


KINDS = {
    "good4": (_good4, 0), "good6": (_good6, 0), "tail4": (_tail4, 0), "tail6": (_tail6, 0),
    "short": (_short, EINVAL), "badver": (_badver, EINVAL), "badihl": (_badihl, EINVAL),
    "hlen_gt_len": (_hlen_gt_len, EINVAL), "badsum": (_badsum, None), "iplen_lt_hlen": (_iplen_lt_hlen, EINVAL),
    "iplen_gt_len": (_iplen_gt_len, EINVAL), "frag": (_frag, ENOTSUP), "proto4": (_proto4, ENOTSUP),
    "small4": (_small4, EINVAL), "unaligned4": (_unaligned4, EINVAL), "unknown4": (_unknown4, ENOENT),
    "spi0": (_spi0, ENOENT), "ahspi": (_ahspi, ENOENT), "wrongdst4": (_wrongdst4, ENOENT),
    "wrongdst6": (_wrongdst6, ENOENT), "wrongaf": (_wrongaf, ENOENT), "short6": (_short6, EINVAL),
    "jumbo6": (_jumbo6, ENOTSUP), "plen_gt_len6": (_plen_gt_len6, EINVAL), "nxt6": (_nxt6, ENOTSUP),
    "linklocal6": (_linklocal6, ENOTSUP), "small6": (_small6, EINVAL), "unaligned6": (_unaligned6, EINVAL),
    "unknown6": (_unknown6, ENOENT),
}


def expected_status(kind, flags):
    """badsum is EINVAL under CLS_IPCSUM and a good packet without it."""
    st = KINDS[kind][1]
    return (EINVAL if flags & L.CLS_IPCSUM else 0) if st is None else st


def random_packets(rng, db, n, good=0.5):
    """n packets: `good` of them accepted kinds, the rest spread over every
    other kind.  Returns [(kind, bytes)]."""
    names = list(KINDS)
    ok = [k for k in names if KINDS[k][1] == 0]
    bad = [k for k in names if KINDS[k][1] != 0]
    out = []
    for _ in range(n):
        pool = ok if rng.random() < good else bad
        k = pool[int(rng.integers(len(pool)))]
        out.append((k, KINDS[k][0](rng, db)))
    return out


def layout(rng, pkts, max_gap4=6):
    """The packets at an irregular 4-byte-aligned stride in one arena of
    random bytes: (arena uint8 array, PKT_DTYPE array).  The arena ends 64
    bytes past the last packet."""
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


def host_classify_batch(table, arena, rec, flags=0):
    """espgpu_esp_classify on every packet of a layout, in index order:
    (DESC array, status uint8 array)."""
    desc = np.zeros(len(rec), dtype=DESC)
    st = np.zeros(len(rec), dtype=np.uint8)
    for i, r in enumerate(rec):
        o = int(r["off4"]) * 4
        rc, d = E.esp_classify_host(table, arena[o:o + int(r["len"])].tobytes(), int(r["off4"]), flags)
        desc[i], st[i] = d, rc
    return desc, st
