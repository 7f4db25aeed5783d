"""Outbound framing, host side: espgpu_esp_frame (the rule that defines
espgpu_esp_frame_batch) against esp.py's restatement of esp_output
(xform_esp.c:700-716, 782-843, 867-887), the counter edges, the shape helper,
the kernels' closed form against the sequential rule, and the framed packet
through the oracle's encrypt and decrypt.  No GPU."""
import numpy as np
import pytest

import oracle as O
from espgpu import _lib as L
from espgpu import esp as E
from frame_helpers import EINVAL, host_frame_batch, layout, record_len, sa_kinds

FILL = 0xA5
KINDS = sa_kinds(np.random.default_rng(2024))
PAD_MODES = [0, L.OUT_PAD_SEQ, L.OUT_PAD_ZERO, L.OUT_PAD_RAND]
M64 = 2**64 - 1


def _raw(sa, shape, payload):
    """The record as the caller hands it over: payload in place, FILL elsewhere."""
    rec = bytearray([FILL]) * record_len(shape, len(payload))
    rec[8 + shape.ivlen:8 + shape.ivlen + len(payload)] = payload
    return rec


def _outsa(st, spi, salt=0):
    return L.OutSA(st.count, st.cntr, spi, salt, st.flags, 0)


@pytest.mark.parametrize("name,sa,kflags", KINDS, ids=[k[0] for k in KINDS])
@pytest.mark.parametrize("esn", [False, True])
@pytest.mark.parametrize("pad", PAD_MODES)
def test_host_rule_matches_esp_output_frame(name, sa, kflags, esn, pad):
    """Byte for byte, rlen 0 .. 35: every pad length and every alignment of
    the trailer for blks 4 and 16."""
    rng = np.random.default_rng(7)
    esa = sa.esp_sa()
    flags = kflags | pad | (L.OUT_ESN if esn else 0)
    shape = E.esp_frame_shape(esa, flags)
    st = E.OutState(count=0x1_0000_0000 * 3 + 41, cntr=0x0102030405060708, flags=flags)
    o = _outsa(st, esa.spi)
    for rlen in range(36):
        payload = rng.integers(0, 256, rlen, dtype=np.uint8).tobytes()
        nh = int(rng.integers(0, 256))
        want, want_hi, st = E.esp_output_frame(st, esa, payload, nh, fill=FILL)
        rec = _raw(esa, shape, payload)
        assert len(rec) == len(want)
        rc, hi = E.esp_frame_host(o, shape, rec, rlen, nh, esn_hi=0x77)
        assert rc == 0 and bytes(rec) == want, (rlen, bytes(rec).hex(), want.hex())
        assert hi == want_hi and (o.count, o.cntr) == (st.count, st.cntr)
        assert hi == (st.count >> 32 if esn else 0)
    assert o.count == 0x1_0000_0000 * 3 + 41 + 36
    assert o.cntr == 0x0102030405060708 + (36 if shape.ivlen == 8 else 0)


def _run(esa, flags, count0, k, cntr0=5):
    """k records of SA esa from count0: [(status, seq, esn_hi)], final outsa,
    checked against esp_output_frame on the way."""
    shape = E.esp_frame_shape(esa, flags)
    st = E.OutState(count0, cntr0, flags)
    o = _outsa(st, esa.spi)
    res = []
    for j in range(k):
        rec = _raw(esa, shape, bytes([j]) * 3)
        before = bytes(rec)
        want, want_hi, st2 = E.esp_output_frame(st, esa, bytes([j]) * 3, 4, fill=FILL)
        c0, n0 = o.count, o.cntr
        rc, hi = E.esp_frame_host(o, shape, rec, 3, 4, esn_hi=0x77)
        if want is None:
            # refused: rec, outsa and esn_hi untouched
            assert rc == EINVAL and bytes(rec) == before and hi == 0x77 and (o.count, o.cntr) == (c0, n0)
            assert st2 is st
            res.append((rc, None, None))
        else:
            assert rc == 0 and bytes(rec) == want and hi == want_hi
            res.append((0, int.from_bytes(rec[4:8], "big"), hi))
        st = st2
        assert (o.count, o.cntr) == (st.count, st.cntr)
    return res, o


GCM_SA, CBC_SA = KINDS[0][1].esp_sa(), KINDS[2][1].esp_sa()


def test_counter_edge_esn_high_word_changes_inside_the_run():
    res, o = _run(GCM_SA, L.OUT_ESN | L.OUT_PAD_SEQ, 2**32 - 3, 6)
    assert res == [(0, 2**32 - 2, 0), (0, 2**32 - 1, 0), (0, 0, 1), (0, 1, 1), (0, 2, 1), (0, 3, 1)]
    assert o.count == 2**32 + 3 and o.cntr == 11


def test_counter_edge_non_esn_low_word_wraps_as_in_the_reference():
    res, o = _run(GCM_SA, L.OUT_PAD_SEQ, 2**32 - 3, 6)
    assert res == [(0, 2**32 - 2, 0), (0, 2**32 - 1, 0), (0, 0, 0), (0, 1, 0), (0, 2, 0), (0, 3, 0)]
    assert o.count == 2**32 + 3 and o.cntr == 11


@pytest.mark.parametrize("esa", [GCM_SA, CBC_SA], ids=["gcm", "cbc"])
def test_counter_edge_wrapcheck_refuses_and_freezes(esa):
    res, o = _run(esa, L.OUT_WRAPCHECK | L.OUT_PAD_SEQ, 2**32 - 3, 6)
    assert res == [(0, 2**32 - 2, 0), (0, 2**32 - 1, 0)] + [(EINVAL, None, None)] * 4
    assert o.count == 2**32 - 1 and o.cntr == (7 if esa is GCM_SA else 5)
    # a non-ESN counter that has wrapped before (no WRAPCHECK then) stops at the next low-word limit
    res, o = _run(esa, L.OUT_WRAPCHECK, 5 * 2**32 - 2, 3)
    assert [r[0] for r in res] == [0, EINVAL, EINVAL] and o.count == 5 * 2**32 - 1


def test_counter_edge_cycseq_is_never_refused():
    for esn in (0, L.OUT_ESN):
        res, o = _run(GCM_SA, L.OUT_WRAPCHECK | L.OUT_CYCSEQ | esn, 2**32 - 3, 6)
        assert [r[0] for r in res] == [0] * 6 and o.count == 2**32 + 3
    res, o = _run(GCM_SA, L.OUT_WRAPCHECK | L.OUT_CYCSEQ | L.OUT_ESN, M64 - 1, 4)
    assert [(r[0], r[1], r[2]) for r in res] == [(0, 2**32 - 1, 2**32 - 1), (0, 0, 0), (0, 1, 0), (0, 2, 0)]
    assert o.count == 2


def test_counter_edge_top_of_the_esn_space():
    res, o = _run(GCM_SA, L.OUT_WRAPCHECK | L.OUT_ESN, M64 - 2, 4)
    assert res == [(0, 2**32 - 2, 2**32 - 1), (0, 2**32 - 1, 2**32 - 1), (EINVAL, None, None), (EINVAL, None, None)]
    assert o.count == M64 and o.cntr == 7
    # ESN with WRAPCHECK passes the 32-bit limit
    res, o = _run(GCM_SA, L.OUT_WRAPCHECK | L.OUT_ESN, 2**32 - 3, 6)
    assert [r[0] for r in res] == [0] * 6 and o.count == 2**32 + 3
    # without WRAPCHECK the 64-bit counter wraps to 0, as count++ does
    res, o = _run(GCM_SA, L.OUT_ESN, M64 - 1, 3)
    assert res == [(0, 2**32 - 1, 2**32 - 1), (0, 0, 0), (0, 1, 0)] and o.count == 1


def test_wrong_length_is_refused_untouched():
    esa = CBC_SA
    shape = E.esp_frame_shape(esa, 0)
    for delta in (-4, -1, 1, 16):
        o = L.OutSA(9, 9, esa.spi, 0, L.OUT_PAD_SEQ, 0)
        rec = bytearray([FILL]) * (record_len(shape, 10) + delta)
        before = bytes(rec)
        rc, hi = E.esp_frame_host(o, shape, rec, 10, 4, esn_hi=0x77)
        assert rc == EINVAL and bytes(rec) == before and hi == 0x77 and (o.count, o.cntr) == (9, 9)


@pytest.mark.parametrize("name,sa,kflags", KINDS, ids=[k[0] for k in KINDS])
def test_shape_helper_follows_secassoc(name, sa, kflags):
    esa = sa.esp_sa()
    shape = E.esp_frame_shape(esa, kflags)
    assert 8 + shape.ivlen == esa.hlen and shape.alen == esa.alen
    assert shape.blks == (16 if esa.ctr and kflags & L.OUT_CTRCOMPAT else max(4, esa.blocksize))
    assert shape.blks == E.esp_out_blks(esa, kflags)
    # CTRCOMPAT changes AES-CTR SAs only
    other = E.esp_frame_shape(esa, kflags ^ L.OUT_CTRCOMPAT)
    assert (other.blks != shape.blks) == esa.ctr


def test_shape_helper_refuses_ah_and_unserved_sessions():
    import ctypes as C
    from espgpu.opencrypto import crypto_session_params
    lib = L.lib()
    shape = L.EShape()
    for kw in (dict(csp_mode=L.CSP_MODE_DIGEST, csp_auth_alg=L.CRYPTO_SHA1_HMAC, csp_auth_klen=20,
                    csp_auth_key=b"a" * 20, csp_auth_mlen=12),
               dict(csp_mode=L.CSP_MODE_AEAD, csp_ivlen=16, csp_cipher_alg=25, csp_cipher_klen=16)):
        p, _keep = crypto_session_params(**kw)._c()
        assert lib.espgpu_esp_frame_shape(C.byref(p), 0, C.byref(shape)) == EINVAL
    # mlen 0 = the whole hash, as espgpu_newsession keeps it
    p, _keep = crypto_session_params(csp_mode=L.CSP_MODE_ETA, csp_ivlen=16, csp_cipher_alg=L.CRYPTO_AES_CBC,
                                     csp_cipher_klen=16, csp_cipher_key=b"k" * 16,
                                     csp_auth_alg=L.CRYPTO_SHA2_256_HMAC, csp_auth_klen=32,
                                     csp_auth_key=b"a" * 32)._c()
    assert lib.espgpu_esp_frame_shape(C.byref(p), 0, C.byref(shape)) == 0
    assert (shape.ivlen, shape.blks, shape.alen) == (16, 16, 32)


def _closed_form(desc, part, outsa, ctr_iv):
    """The kernels' arithmetic (frame.hip): a stable sort by
    SA, rank = grouped position - segment start, the first m = min(k, room)
    ranks accepted with count0 + rank + 1 and cntr0 + rank.  Returns (accepted,
    count, cntr per record; final count, cntr per SA)."""
    n, nout = len(desc), len(outsa)
    key = np.where(part, desc["sa"].astype(np.int64), nout)
    order = np.argsort(key, kind="stable")
    skey = key[order]
    head = np.r_[True, skey[1:] != skey[:-1]]
    start = np.maximum.accumulate(np.where(head, np.arange(n), 0))
    rank = np.arange(n) - start
    acc, cnt, ctr = np.zeros(n, bool), [0] * n, [0] * n
    fin = [(int(o["count"]), int(o["cntr"])) for o in outsa]
    for p in range(n):
        sa = int(skey[p])
        if sa >= nout:
            continue
        c0, n0, f = int(outsa["count"][sa]), int(outsa["cntr"][sa]), int(outsa["flags"][sa])
        if not f & L.OUT_WRAPCHECK or f & L.OUT_CYCSEQ:
            room = M64
        else:
            room = M64 - c0 if f & L.OUT_ESN else 0xffffffff - (c0 & 0xffffffff)
        r, i = int(rank[p]), int(order[p])
        if r < room:
            acc[i], cnt[i], ctr[i] = True, (c0 + r + 1) & M64, (n0 + r) & M64
        if p + 1 == n or skey[p + 1] != sa:
            m = min(r + 1, room)
            fin[sa] = ((c0 + m) & M64, (n0 + m) & M64 if ctr_iv[sa] else n0)
    return acc, cnt, ctr, fin


@pytest.mark.parametrize("seed", range(6))
def test_closed_form_equals_the_sequential_rule(seed):
    from espgpu.batch import OUTSA_DTYPE
    rng = np.random.default_rng(100 + seed)
    sas = [k[1].esp_sa() for k in KINDS]
    nout = len(sas) + 2                       # two entries without a session
    outsa = np.zeros(nout, dtype=OUTSA_DTYPE)
    edge = [2**32 - 3, 2**32 - 40, M64 - 5, 5 * 2**32 - 9, 17, 0]
    for k in range(nout):
        f = int(rng.choice([0, L.OUT_ESN])) | int(rng.choice([0, L.OUT_WRAPCHECK])) | \
            int(rng.choice([0, 0, L.OUT_CYCSEQ])) | int(rng.choice(PAD_MODES))
        c0 = edge[int(rng.integers(len(edge)))]
        if k == 0:                             # these two run out of numbers inside the batch
            f, c0 = L.OUT_WRAPCHECK | L.OUT_PAD_SEQ, 2**32 - 3
        elif k == 1:
            f, c0 = L.OUT_WRAPCHECK | L.OUT_ESN, M64 - 5
        if k < len(sas):
            f |= KINDS[k][2]
        outsa[k] = (np.uint64(c0), int(rng.integers(0, 2**40)), 0x1000 + k, 0x01020304 * (k + 1), f, 0)
    shapes = [E.esp_frame_shape(s, int(outsa["flags"][k])) for k, s in enumerate(sas)] + [None, None]
    n = 400
    sa = rng.integers(0, nout + 2, n)          # some sa >= nout
    rlen = rng.integers(0, 80, n)
    arena, desc = layout(rng, shapes, sa, rlen)
    bad = rng.random(n) < 0.1                  # a wrong len
    desc["len"][bad] += rng.choice([-4, 4, 1], int(bad.sum())).astype(np.uint16)
    frame = (rlen | (rng.integers(0, 256, n) << 16)).astype(np.uint32)
    part = np.array([s < nout and shapes[s] is not None and int(desc["len"][i]) == record_len(shapes[s], int(rlen[i]))
                     for i, s in enumerate(sa)])
    assert 0 < part.sum() < n
    h_arena, h_desc, h_fst, h_out = host_frame_batch(arena, desc, frame, outsa, shapes)
    acc, cnt, ctr, fin = _closed_form(desc, part, outsa, [s is not None and s.ivlen == 8 for s in shapes])
    assert np.array_equal(h_fst == 0, acc)
    assert (h_fst[~part] == EINVAL).all() and acc.sum() < part.sum()    # (some SA ran out of numbers)
    for i in np.flatnonzero(acc):
        s, o = int(sa[i]), int(desc["off4"][i]) * 4
        esn = int(outsa["flags"][s]) & L.OUT_ESN
        assert int.from_bytes(h_arena[o + 4:o + 8].tobytes(), "big") == cnt[i] & 0xffffffff
        assert int(h_desc["esn_hi"][i]) == (cnt[i] >> 32 if esn else 0)
        if shapes[s].ivlen == 8:
            assert int.from_bytes(h_arena[o + 8:o + 16].tobytes(), "big") == ctr[i]
    assert [(int(o["count"]), int(o["cntr"])) for o in h_out] == fin


@pytest.mark.parametrize("name", ["gcm128", "cbc-sha1", "ctr-sha256-compat", "null-sha1", "cbc"])
@pytest.mark.parametrize("esn", [False, True])
def test_framed_packet_is_what_the_peer_accepts(name, esn):
    """Host rule -> oracle encrypt -> oracle decrypt: status 0, the payload
    back, and the trailer word carries the pad length and next header."""
    from espgpu.batch import OUTSA_DTYPE
    from helpers import EtaSA, GcmSA
    rng = np.random.default_rng(5)
    # a fresh SA of this kind with the ESN flag wanted (a CIPHER session has none)
    sa = {"gcm128": lambda: GcmSA(rng, 16, esn=esn), "cbc-sha1": lambda: EtaSA(rng, esn=esn),
          "ctr-sha256-compat": lambda: EtaSA(rng, ctr=True, sha=256, esn=esn),
          "null-sha1": lambda: EtaSA(rng, null=True, esn=esn), "cbc": lambda: EtaSA(rng, noauth=True)}[name]()
    esa = sa.esp_sa()
    kflags = L.OUT_CTRCOMPAT if name == "ctr-sha256-compat" else 0
    flags = kflags | L.OUT_PAD_SEQ | (L.OUT_ESN if sa.esn else 0)
    shapes = [E.esp_frame_shape(esa, flags)]
    outsa = np.zeros(1, dtype=OUTSA_DTYPE)
    outsa[0] = (2**32 - 5 if sa.esn else 100, 9, esa.spi, int.from_bytes(esa.salt, "little"), flags, 0)
    n = 24
    rlen = np.r_[np.arange(0, 20), rng.integers(20, 1400, 4)]
    nh = rng.integers(0, 59, n)
    arena, desc = layout(rng, shapes, np.zeros(n, dtype=np.int64), rlen)
    frame = (rlen | (nh << 16)).astype(np.uint32)
    framed, fdesc, fst, fout = host_frame_batch(arena, desc, frame, outsa, shapes)
    assert (fst == 0).all() and int(fout["count"][0]) == int(outsa["count"][0]) + n
    ct = framed.copy()
    O.batch([sa.oracle], ct, fdesc["off4"], fdesc["len"], fdesc["sa"], esn_hi=fdesc["esn_hi"].copy(),
            nthreads=2, encrypt=True)
    assert (fdesc["salt"] == int.from_bytes(esa.salt, "little")).all() or shapes[0].ivlen != 8
    pt = ct.copy()
    _, st = O.batch([sa.oracle], pt, fdesc["off4"], fdesc["len"], fdesc["sa"], esn_hi=fdesc["esn_hi"].copy(),
                    nthreads=2)
    assert (np.asarray(st) == 0).all()
    for i in range(n):
        o, ln = int(fdesc["off4"][i]) * 4, int(fdesc["len"][i])
        body = pt[o + 8 + shapes[0].ivlen:o + ln - shapes[0].alen].tobytes()
        raw = arena[o + 8 + shapes[0].ivlen:o + 8 + shapes[0].ivlen + int(rlen[i])].tobytes()
        assert body[:int(rlen[i])] == raw
        w, padlen = E.trailer_word(body), len(body) - int(rlen[i]) - 2
        assert w == (int(nh[i]) | (padlen << 8) | L.TR_VALID), (i, hex(w))
        assert E.trailer_accepts(w)
