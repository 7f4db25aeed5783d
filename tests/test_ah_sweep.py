"""CPU side of the AH digest sweeps (ah_sweep_helpers.py): the layouts cover
what they were chosen for, asserted from the layouts themselves; the
reference (AhSA.icv_hole / AhSA.icv, oracle.hmac) is pinned to Python's hmac
and hashlib at every length and key length the GPU tests use; and every
layout's expected statuses hold the classes it promises."""
import hashlib
import hmac

import numpy as np
import pytest

import ah_sweep_helpers as H
from ah_helpers import BLOCK

_HASH = {1: hashlib.sha1, 256: hashlib.sha256, 384: hashlib.sha384, 512: hashlib.sha512}
HASH_ESN = pytest.mark.parametrize("sha,esn", H.HASH_ESN, ids=H.HASH_ESN_IDS)


def test_length_sets():
    for sha in H.SHAS:
        blk = BLOCK[sha]
        assert H.dense_lens(sha) == list(range(H.MLEN[sha], 4 * blk + 9))
        assert H.key_lens(sha) == [1, H.HASHSIZE[sha], blk - 1, blk, blk + 1, 2 * blk + 7]
    assert len(H.dense_lens(1)) == 253 and len(H.dense_lens(512)) == 489
    assert set(H.LONG_LENS) == set(range(1480, 1521)) | set(range(8990, 9011)) | set(range(65400, 65536))
    # the padding of total_blocks is SHA's own: hashlib's block count of the same message
    for sha, esn in H.HASH_ESN:
        for L in (0, 1, 55, 56, 111, 112, 119, 120, 65535):
            n = L + (4 if esn else 0)
            padded = n + 1 + (-(n + 1 + BLOCK[sha] // 8)) % BLOCK[sha] + BLOCK[sha] // 8
            assert H.total_blocks(sha, esn, L) * BLOCK[sha] == padded


@HASH_ESN
def test_dense_lengths_reach_every_residue_at_every_block_count(sha, esn):
    """Every L mod blk at 1, 2, 3 and 4 or more total blocks: at 1 to 3 every
    residue that any record of at least the ICV field has at that count, at 4
    or more every residue there is."""
    blk = BLOCK[sha]
    lens = H.dense_lens(sha)
    for t in (1, 2, 3):
        possible = {L % blk for L in range(H.MLEN[sha], 8 * blk) if H.total_blocks(sha, esn, L) == t}
        assert {L % blk for L in lens if H.total_blocks(sha, esn, L) == t} == possible
        assert len(possible) == (blk if t > 1 else blk - H.MLEN[sha] - (4 if esn else 0) - blk // 8)
    assert {L % blk for L in lens if H.total_blocks(sha, esn, L) >= 4} == set(range(blk))
    assert max(H.total_blocks(sha, esn, L) for L in lens) == 5
    # all four positions of the ESN word and the 0x80 byte in their dword, at every block count
    assert {(L & 3, H.total_blocks(sha, esn, L)) for L in lens} == {(r, t) for r in range(4) for t in range(1, 6)}


@HASH_ESN
def test_uniform_units_cover_every_field_class_at_every_salt(sha, esn):
    """Every class of field_class at every salt mod blk (multiples of 4)
    where it can exist at all among the dense lengths, and a field that ends
    exactly at L in every class and at every salt residue it can have."""
    lay = H.uniform(sha, esn)
    blk, m = BLOCK[sha], H.MLEN[sha]
    lens = H.unit_lens(sha)
    assert sorted(lens) == H.dense_lens(sha)
    assert lay.n == len(lens) * 64 and (lay.L.reshape(-1, 64) == np.array(lens)[:, None]).all()
    assert (lay.salt % 4 == 0).all() and (lay.salt + m <= lay.L).all() and not lay.malformed.any()
    possible, ends = set(), set()
    for L in lens:
        for s in range(0, L - m + 1, 4):
            c, end = H.field_class(sha, L, s, m)
            possible.add((c, s % blk))
            if end:
                ends.add((c, s % blk))
    have = {H.field_class(sha, int(L), int(s), m) + (int(s) % blk,) for L, s in zip(lay.L, lay.salt)}
    assert {(c, r) for c, _, r in have} == possible
    assert {(c, r) for c, end, r in have if end} == ends
    # (a field that ends with the record cannot end inside a whole block that has another after it)
    assert {c for c, _ in possible} == set(H.FIELD_CLASSES)
    assert {c for c, _ in ends} == set(H.FIELD_CLASSES) - {"two-whole"}
    # a field across two whole blocks, or across the last whole block and the tail, at each dword of the cut
    for c in ("two-whole", "whole-tail"):
        assert {r for cc, r in possible if cc == c} == {blk - m + 4 * k for k in range(1, m // 4)}
    # every salt of a length where 64 lanes can hold them all, 64 different ones elsewhere
    for u, L in enumerate(lens):
        ns = ((L - m) & ~3) // 4 + 1
        got = set(lay.salt[u * 64:(u + 1) * 64])
        assert got <= {4 * k for k in range(ns)} and len(got) == min(ns, 64), L


@HASH_ESN
def test_uniform_units_tampering(sha, esn):
    """Even units intact; in odd units byte 0, byte L - 1 and a field byte
    of three records at rotating lanes; the accepted lanes are no prefix."""
    lay = H.uniform(sha, esn)
    t = lay.tampered.reshape(-1, 64)
    assert not t[::2].any() and (t[1::2].sum(axis=1) == 3).all() and t.any(axis=0).all()
    assert all(not r[:61].all() for r in ~t[1::2])
    at = {}
    for i, pos, _ in lay.tamper:
        at.setdefault(i // 64, []).append((pos, int(lay.L[i]), int(lay.salt[i])))
    for u, flips in at.items():
        (p0, L, _), (p1, _, _), (p2, _, s2) = flips
        assert p0 == 0 and p1 == L - 1 and s2 <= p2 < s2 + H.MLEN[sha]
    # the last byte in a partial dword at each of its three positions; waves of equal lengths, all
    # accepted, with the message ending at each byte of a dword, at every block count
    assert {f[1][1] & 3 for f in at.values()} == {0, 1, 2, 3}
    for units in (lay.L[::64][::2], lay.L[::64][1::2]):
        assert {(int(L) & 3, H.total_blocks(sha, esn, int(L))) for L in units} == {
            (r, n) for r in range(4) for n in range(1, 6)}


@HASH_ESN
def test_mixed_families_are_what_they_prescribe(sha, esn):
    blk = BLOCK[sha]
    j = H.quads(sha, esn)
    assert j.n == H.MIXED_UNITS * 64 and (j.salt + j.mlen <= j.L).all()
    tb = np.array([H.total_blocks(sha, esn, int(L)) for L in j.L]).reshape(-1, 4)
    lo = (j.L & 3).reshape(-1, 4)
    assert all(len(set(q)) == 4 for q in tb) and all(sorted(q) == [0, 1, 2, 3] for q in lo)
    assert {tuple(q) for q in lo} == {tuple((k + r) % 4 for k in range(4)) for r in range(4)}
    assert set(tb.reshape(-1)) == set(range(1, 9))
    # the longest record of a quad at each of its four positions
    assert set(np.argmax(tb, axis=1)) == {0, 1, 2, 3}
    k = H.one_long(sha, esn)
    Ls = k.L.reshape(-1, 64)
    long = Ls >= 1480
    assert (long.sum(axis=1) == 1).all() and (np.argmax(long, axis=1) == np.arange(H.MIXED_UNITS)).all()
    assert {int(u) % 4 for u in np.argmax(long, axis=1)} == {0, 1, 2, 3}
    assert set(Ls[long]) <= set(H.LONG_LENS) and 65535 in Ls[long] and len(set(Ls[long])) == H.MIXED_UNITS
    assert {int(L) & 3 for L in Ls[long]} == {0, 1, 2, 3}
    assert all(H.total_blocks(sha, esn, int(L)) == 1 for L in Ls[~long]) and Ls[~long].max() < blk
    assert k.tampered[[u * 64 + u for u in range(0, H.MIXED_UNITS, 5)]].all() and k.tampered.sum() >= 10


def test_interleaved_and_random_layouts_are_what_they_prescribe():
    ly = H.hashes()
    wide = np.array([s.sha >= 384 for s in ly.sas])[ly.descs["sa"]]
    assert ly.n == H.MIXED_UNITS * 64 and len(ly.sas) == 11
    assert {(s.sha, s.esn) for s in ly.sas} == set(H.HASH_ESN)
    assert {(s.sha, s.mlen, s.sa.mlen) for s in ly.sas} >= {(1, 20, 20), (512, 64, 64), (384, 48, 0)}
    assert all(0 < wide[q:q + 4].sum() < 4 for q in range(0, ly.n, 4))        # lanes of both launches in every quad
    for u in range(H.MIXED_UNITS):
        sl = slice(u * 64, u * 64 + 64)
        assert len(set(ly.descs["sa"][sl])) == 11
        narrow = {ly.sas[s].sha for s in ly.descs["sa"][sl]}
        assert narrow == set(H.SHAS)                                           # both passes, both wide hashes
    assert len({tuple(ly.descs["sa"][u * 64:u * 64 + 4]) for u in range(H.MIXED_UNITS)}) == 11
    assert 0.02 < ly.tampered.mean() < 0.08
    m = H.random_mix()
    assert m.n == H.MIXED_UNITS * 64 - 27 and m.n % 64
    for kind in H.BAD_KINDS:
        assert (m.kind == kind).sum() >= 20, kind
    assert m.malformed[-1] and 0.02 < m.tampered.mean() < 0.08 and not (m.tampered & m.malformed).any()
    d = m.descs
    mlen = np.array([s.mlen for s in m.sas])[d["sa"]]
    assert (d["len"][m.kind == "len0"] == 0).all()
    short = m.kind == "short"
    assert ((d["len"][short] > 0) & (d["len"][short] < mlen[short])).all()
    assert (d["salt"][m.kind == "salt-odd"] & 3 != 0).all()
    past = m.kind == "salt-past"
    assert ((d["salt"][past] % 4 == 0) & (d["salt"][past] + mlen[past] > d["len"][past])).all()
    assert (d["salt"][m.kind == "salt-big"] > 0xffff).all()
    assert set(d["sa"][m.kind == "freed"]) == set(m.freed_sas) and not set(d["sa"][m.kind != "freed"]) & set(m.freed_sas)
    ok = ~m.malformed
    assert ((d["len"][ok] >= mlen[ok]) & (d["salt"][ok] % 4 == 0) & (d["salt"][ok] + mlen[ok] <= d["len"][ok])).all()
    assert {(m.sas[s].sha, m.sas[s].esn) for s in d["sa"][ok]} == set(H.HASH_ESN)
    kl = H.key_lengths()
    assert [len(s.key) for s in kl.sas] == [k for sha in H.SHAS for k in H.key_lens(sha)] and kl.n == 96
    assert len({s.key for s in kl.sas}) == 24
    for i in range(kl.n):
        s = kl.sa_of(i)
        assert kl.L[i] == [s.mlen, BLOCK[s.sha] - 9, BLOCK[s.sha], 2 * BLOCK[s.sha] + 3][i % 4]


def _py_hmac(sa, msg, esn_hi):
    m = bytes(msg) + (int(esn_hi).to_bytes(4, "big") if sa.esn else b"")
    return hmac.new(sa.key, m, _HASH[sa.sha]).digest()[:sa.mlen]


@HASH_ESN
def test_reference_is_hashlib_hmac_at_every_dense_length(sha, esn):
    """AhSA.icv and AhSA.icv_hole against Python's hmac at every dense
    length: the uniform layout's own records (its key, its salts), the field
    zeroed by hand here."""
    lay = H.uniform(sha, esn)
    signed, bad, st = H.reference(lay)
    sa = lay.sas[0]
    seen = set()
    for i in range(0, lay.n, 13):                    # 4 or 5 records of every length
        o, L, s, eh = int(lay.off[i]), int(lay.L[i]), int(lay.salt[i]), int(lay.descs["esn_hi"][i])
        rec = lay.arena[o:o + L].tobytes()
        assert sa.icv(rec, eh) == _py_hmac(sa, rec, eh), lay.where(i)
        holed = rec[:s] + bytes(sa.mlen) + rec[s + sa.mlen:]
        want = _py_hmac(sa, holed, eh)
        assert sa.icv_hole(rec, s, eh) == want and signed[o + s:o + s + sa.mlen].tobytes() == want, lay.where(i)
        seen.add(L)
    assert seen == set(H.dense_lens(sha))
    # the ESN word is hashed exactly when the session has ESN
    rec = lay.arena[:100].tobytes()
    assert (sa.icv(rec, 1) != sa.icv(rec, 2)) == esn


def test_reference_is_hashlib_hmac_at_every_key_length_and_long_length():
    """hashlib takes the long-key branch by itself."""
    kl = H.key_lengths()
    signed, _, _ = H.reference(kl)
    for i in range(kl.n):
        sa = kl.sa_of(i)
        o, L, s, eh = int(kl.off[i]), int(kl.L[i]), int(kl.salt[i]), int(kl.descs["esn_hi"][i])
        rec = kl.arena[o:o + L].tobytes()
        assert sa.icv(rec, eh) == _py_hmac(sa, rec, eh), kl.where(i)
        holed = rec[:s] + bytes(sa.mlen) + rec[s + sa.mlen:]
        assert signed[o + s:o + s + sa.mlen].tobytes() == _py_hmac(sa, holed, eh), kl.where(i)
    # a key of one byte more than the block is not the key cut to the block
    rng = np.random.default_rng(5)
    for sha in H.SHAS:
        sa = H.make_sa(rng, sha, aklen=BLOCK[sha] + 1)
        assert sa.icv(b"abc") != hmac.new(sa.key[:BLOCK[sha]], b"abc", _HASH[sha]).digest()[:sa.mlen]
    for lay in (H.one_long(1, True), H.one_long(512, False), H.hashes()):
        signed, _, _ = H.reference(lay)
        for i in list(range(0, lay.n, 65))[:32] + list(range(7, lay.n, 41)):
            sa = lay.sa_of(i)
            o, L, s, eh = int(lay.off[i]), int(lay.L[i]), int(lay.salt[i]), int(lay.descs["esn_hi"][i])
            rec = lay.arena[o:o + L].tobytes()
            holed = rec[:s] + bytes(sa.mlen) + rec[s + sa.mlen:]
            assert signed[o + s:o + s + sa.mlen].tobytes() == _py_hmac(sa, holed, eh), lay.where(i)


def _layouts():
    for sha, esn in H.HASH_ESN:
        yield "uniform", H.uniform(sha, esn)
        yield "quads", H.quads(sha, esn)
        yield "one_long", H.one_long(sha, esn)
    yield "hashes", H.hashes()
    yield "random", H.random_mix()
    yield "keys", H.key_lengths()


def test_every_layout_holds_the_classes_it_promises():
    """The reference's self-check passes (a tampered record's stored ICV
    differs from icv_hole of its tampered bytes), the signed arena differs
    from the arena in ICV fields only, and the expected statuses contain 0
    and EBADMSG everywhere, EINVAL where the layout has malformed records."""
    for name, lay in _layouts():
        signed, bad, st = H.reference(lay)
        assert set(st) == ({0, H.EBADMSG, H.EINVAL} if name == "random" else {0, H.EBADMSG}), name
        assert (st == H.EINVAL).sum() == lay.malformed.sum() and (st == H.EBADMSG).sum() == lay.tampered.sum()
        field = np.zeros(len(signed), dtype=bool)
        for i in np.nonzero(~lay.malformed)[0]:
            field[lay.off[i] + lay.salt[i]:lay.off[i] + lay.salt[i] + lay.mlen[i]] = True
        assert (signed[~field] == lay.arena[~field]).all(), name
        assert (bad != signed).sum() == len(lay.tamper), name
        # records do not overlap: each field is its record's own
        ends = lay.off + ((np.maximum(lay.L, 1) + 3) & ~3)
        assert (lay.off[1:] >= ends[:-1] + 4).all(), name
