"""Shared by the outbound framing tests: the session kinds, and the sequential
definition of espgpu_esp_frame_batch -- the host rule espgpu_esp_frame applied
to the records in index order."""
import ctypes as C

import numpy as np

from helpers import DESC, EtaSA, GcmSA

EINVAL = 22


def sa_kinds(rng):
    """(name, SA, outsa flags that change its shape): every session kind the
    framing serves."""
    from espgpu import _lib as L
    return [("gcm128", GcmSA(rng, 16), 0), ("gcm256", GcmSA(rng, 32), 0),
            ("cbc-sha1", EtaSA(rng), 0),
            ("ctr-sha256", EtaSA(rng, ctr=True, sha=256), 0),
            ("ctr-sha256-compat", EtaSA(rng, ctr=True, sha=256), L.OUT_CTRCOMPAT),
            ("null-sha1", EtaSA(rng, null=True), 0),
            ("cbc", EtaSA(rng, noauth=True), 0), ("ctr", EtaSA(rng, ctr=True, noauth=True), 0)]


def record_len(shape, rlen):
    padding = ((shape.blks - ((rlen + 2) % shape.blks)) % shape.blks) + 2
    return 8 + shape.ivlen + rlen + padding + shape.alen


def host_frame_batch(arena, desc, frame, outsa, shapes):
    """shapes[sa]: the L.EShape of session sa under outsa[sa].flags, or None
    where the engine holds no ESP session.  Returns (arena, desc, fstatus,
    outsa) after the batch; the inputs are not modified."""
    from espgpu import _lib as L
    lib = L.lib()
    arena, desc, outsa = arena.copy(), desc.copy(), outsa.copy()
    n, nout = len(desc), len(outsa)
    outs = [L.OutSA(int(o["count"]), int(o["cntr"]), int(o["spi"]), int(o["salt"]), int(o["flags"]),
                    int(o["pad_"])) for o in outsa]
    fst = np.zeros(n, dtype=np.uint8)
    base = arena.ctypes.data
    hi = C.c_uint32(0)
    for i in range(n):
        sa = int(desc["sa"][i])
        rc = EINVAL
        if sa < nout and sa < len(shapes) and shapes[sa] is not None:
            f = int(frame[i])
            rc = lib.espgpu_esp_frame(C.byref(outs[sa]), C.byref(shapes[sa]), base + int(desc["off4"][i]) * 4,
                                      int(desc["len"][i]), f & 0xffff, (f >> 16) & 0xff, C.byref(hi))
        if rc == 0:
            desc["esn_hi"][i] = hi.value
            if shapes[sa].ivlen == 8:
                desc["salt"][i] = outs[sa].salt
        else:
            assert rc == EINVAL
            desc["len"][i] = 0
            fst[i] = EINVAL
    for k, o in enumerate(outs):
        outsa[k] = (np.uint64(o.count), np.uint64(o.cntr), o.spi, o.salt, o.flags, o.pad_)
    return arena, desc, fst, outsa


def layout(rng, shapes, sa, rlen, guard=8, fill=True):
    """An arena with the records of (sa[i], rlen[i]) at 4-byte aligned offsets,
    `guard` .. guard + 3 bytes apart, random bytes everywhere (payloads, the
    fields the framing leaves alone, the guards), and their descriptors with
    len = the length the SA's shape asks for (0 where it has none)."""
    n = len(sa)
    desc = np.zeros(n, dtype=DESC)
    lens = np.array([record_len(shapes[s], int(r)) if s < len(shapes) and shapes[s] is not None else 24
                     for s, r in zip(sa, rlen)], dtype=np.int64)
    stride = (lens + guard + 3) & ~3
    offs = np.concatenate([[0], np.cumsum(stride)[:-1]]) + 4 * ((guard + 3) // 4)
    total = int(offs[-1] + stride[-1]) + 64 if n else 64
    arena = rng.integers(0, 256, total, dtype=np.uint8) if fill else np.zeros(total, dtype=np.uint8)
    desc["off4"] = offs // 4
    desc["len"] = lens
    desc["sa"] = sa
    desc["esn_hi"] = 0x5a5a5a5a
    desc["salt"] = 0xa5a5a5a5
    return arena, desc
