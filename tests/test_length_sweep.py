"""CPU side of the payload-length sweeps (sweep_helpers.py): the length sets
cover what they were chosen for, the mixed layouts are what their families
prescribe, and the oracle's record composition at the sweep lengths is pinned
to hashlib's HMAC and, where tools/libossl_esp.so is built, to OpenSSL (the
oracle's primitives are pinned in test_oracle.py)."""
import hashlib
import hmac
import os
import sys

import numpy as np
import pytest

import oracle as O
import sweep_helpers as H
from helpers import oracle_decrypt

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import ossl_esp  # noqa: E402

needs_openssl = pytest.mark.skipif(not ossl_esp.available(), reason="tools/libossl_esp.so not built")


def test_length_sets():
    assert len(H.GCM_LENS) == 579 and H.GCM_LENS[0] == 0 and all(L % 4 == 0 for L in H.GCM_LENS)
    assert set(range(0, 2113, 4)) | set(range(4032, 4129, 4)) | set(range(8128, 8225, 4)) == set(H.GCM_LENS)
    assert H.CBC_LENS == [16 * nb for nb in range(69)]
    assert H.CTR_LENS == list(range(0, 1089, 4))


@pytest.mark.parametrize("S", [4, 8])
def test_gcm_lengths_cover_every_schedule_shape(S):
    """Every front padding S*M - N, every size of the last block and both
    parities of the step count M, at 4 and at 8 lanes per record; the GHASH
    preload boundary (96 blocks) and up to 5 CTR steps of the burst pass."""
    shapes = [H.gcm_shape(L, S) for L in H.GCM_LENS if L > 0]
    assert {p for _, p, _ in shapes} == set(range(S))
    assert {r for _, _, r in shapes} == {4, 8, 12, 16}
    assert {M & 1 for M, _, _ in shapes} == {0, 1}
    # every pad with every parity of M (a pair step's second half present or not)
    assert {(p, M & 1) for M, p, _ in shapes} == {(p, q) for p in range(S) for q in (0, 1)}
    assert H.gcm_shape(2112, S)[0] == {4: 34, 8: 17}[S]
    assert {M for M, _, _ in shapes} >= set(range(1, H.gcm_shape(2112, S)[0] + 1))
    ncts = {H.gcm_nct(L) for L in H.GCM_LENS}
    assert set(range(0, 133)) <= ncts                       # N = nct + 2 = 96 among them
    assert {(n + 32) // 32 for n in range(1, 133)} == {1, 2, 3, 4, 5}


def test_gcm_lengths_aligned_and_counter_windows():
    aligned = [L for L in H.GCM_LENS if H.gcm_aligned(L)]
    assert len(aligned) >= 100
    assert len([L for L in aligned if L <= 2112]) == 132
    # the counter of CT block i is i + 2: it reaches 256 at byte 4064 and 512
    # at byte 8160, and the windows hold lengths on both sides of each
    for edge in (4064, 8160):
        assert (edge // 16 + 2) & 255 == 0
        assert {edge - 32, edge - 4, edge, edge + 4, edge + 16, edge + 64} <= set(H.GCM_LENS)


@pytest.mark.parametrize("kind", list(H.ETA_KINDS))
def test_eta_lengths_cover_every_padding_shape(kind):
    """The hashed length hl + payload (+ 4 with ESN) reaches every residue
    modulo the hash block that the kind can reach at all, so every residue at
    which the padding needs a block more; CBC block counts cover nb mod 8."""
    sa = H.eta_sa(np.random.default_rng(0), kind)
    lens = [L for L in H.eta_lens(kind) if L > 0]
    if sa.noauth:
        assert {(L // 16) % 8 for L in lens} == set(range(8))
        return
    B = H.HASH_BLOCK[sa.sha]
    step = 16 if kind.startswith("cbc") else 4
    base = sa.hlen + (4 if sa.esn else 0)
    reachable = {(base + step * k) % B for k in range(B // step)}
    assert len(reachable) == B // step
    assert {(base + L) % B for L in lens} == reachable
    # 0x80 and the length field (8 bytes, 16 for the wide hashes) no longer fit
    over = {r for r in reachable if r + 1 + B // 8 > B}
    assert over and over <= {(base + L) % B for L in lens}
    if kind == "cbc128-sha384":
        assert 120 in over and (sa.hlen + 96) % 128 == 120
    if kind.startswith("cbc"):
        assert {(L // 16) % 8 for L in lens} == set(range(8))


def test_gcm_mixed_families_are_what_they_prescribe():
    rng = np.random.default_rng(1)
    a = H.gcm_family_lens("a-aligned", rng)
    assert a.shape == (H.GCM_WAVES, 16) and all(H.gcm_aligned(L) for L in a.reshape(-1))
    nct = (a + 15) // 16
    assert nct.min() >= 3 and nct.max() <= 131
    at_max = (nct == nct.max(axis=1, keepdims=True)).sum(axis=1)
    distinct = np.array([len(set(r)) for r in nct])
    assert (distinct[at_max != 15] >= 4).all() and (distinct >= 2).all()
    assert (at_max == 1).sum() >= 16 and (at_max == 15).sum() >= 16
    assert {int(i) for i in np.argmax(nct, axis=1)[at_max == 1]} >= set(range(1, 16, 3))   # rotating lanes
    # both parities of the wave's aligned step count Maw = (nct + 1) / 4
    assert {int(x) & 1 for x in (nct.max(axis=1) + 1) // 4} == {0, 1}
    b = H.gcm_family_lens("b-one-unaligned", rng)
    un = np.array([[not H.gcm_aligned(L) for L in r] for r in b])
    assert (un.sum(axis=1) == 1).all() and len(set(np.argmax(un, axis=1))) == 16
    c = H.gcm_family_lens("c-one-long", rng)
    assert ((c > 64).sum(axis=1) == 1).all() and len(set(np.argmax(c, axis=1))) == 16
    assert set(c.max(axis=1)) <= set(H._LONG_LENS) and 2112 in c and (c >= 4032).any() and (c >= 8128).any()
    d = (H.gcm_family_lens("d-ascending", rng) + 15) // 16
    assert (np.diff(d, axis=1) == 1).all() and list(d[:, 0]) == list(range(1, 65))
    e = H.gcm_mixed("e-random")
    assert e.n % 16 and e.foreign.sum() >= 10 and (e.descs["len"] % 4 == 2).sum() >= 10
    assert not e.foreign[::4].any() and (e.descs["len"][~e.foreign] == 16 + e.sas[0].mlen).any()


def test_eta_mixed_families_are_what_they_prescribe():
    for kind in ("cbc128-sha1", "ctr256-sha256"):
        f = H.eta_mixed("f-quads", kind)
        nb = (np.array([f.payload(i) for i in range(f.n)]) + 15) // 16
        quads = nb.reshape(-1, 4)
        assert f.n == H.ETA_UNITS * 64 and nb.min() >= 1 and nb.max() <= 68
        assert all(sorted(q % 4) == [0, 1, 2, 3] for q in quads)
        assert {tuple(q % 4) for q in quads} == {tuple((k + r) % 4 for k in range(4)) for r in range(4)}
        g = H.eta_mixed("g-one-long", kind)
        pl = np.array([g.payload(i) for i in range(g.n)]).reshape(-1, 64)
        assert ((pl == 1088).sum(axis=1) == 1).all() and (np.argmax(pl, axis=1) == np.arange(H.ETA_UNITS)).all()
        assert set(pl[pl != 1088]) == {16 if kind.startswith("cbc") else 4}
        h = H.eta_mixed("h-random", kind)
        assert h.n % 64 and h.orphan.sum() == 30 and 0.02 < h.tampered.mean() < 0.08
        pl = np.array([h.payload(i) for i in range(h.n)])
        assert (pl == 0).sum() >= 30
        if kind.startswith("cbc"):
            assert (pl % 16 == 12).sum() == 30 and (h.malformed == ((pl % 16 != 0) | (pl == 0) | h.orphan)).all()
    i = H.eta_interleaved()
    assert all(sorted(i.descs["sa"][q:q + 4]) == [0, 1, 2, 3] for q in range(0, i.n, 4))
    assert len({tuple(i.descs["sa"][u * 64:u * 64 + 4]) for u in range(H.ETA_UNITS)}) == 4


def test_uniform_layouts_keep_enough_intact_records():
    """At most 1/8 of a uniform layout is tampered and every length keeps at
    least 14 (GCM) or 61 (ETA) intact records; the tampered lanes rotate."""
    b = H.gcm_uniform(0)
    t = b.tampered.reshape(-1, H.GCM_RUN)
    assert b.n == 9264 and not t[::2].any() and (t[1::2].sum(axis=1) == 2).all() and t.any(axis=0).all()
    b = H.eta_uniform("ctr256-sha256")
    t = b.tampered.reshape(-1, H.ETA_UNIT)
    assert b.n == 273 * 64 and not t[::2].any() and (t[1::2].sum(axis=1) == 3).all() and t.any(axis=0).all()
    # the verified lanes of a tampered unit are no prefix of it
    assert all(not r[:61].all() for r in ~t[1::2])


def test_oracle_tells_the_mixed_layouts_record_classes_apart():
    """What the GPU cases assert before they touch the GPU, here for the mixed
    layouts: the oracle alone answers 0 for every intact well-formed record,
    EBADMSG for every tampered one and EINVAL for every malformed one
    (sweep_helpers.expected asserts it), decrypting and encrypting."""
    batches = [H.gcm_mixed(f) for f in H.GCM_FAMILIES] + [H.eta_interleaved()] + \
              [H.eta_mixed(f, k) for f in H.ETA_FAMILIES for k in H.MIXED_KINDS]
    for b in batches:
        for encrypt in (False, True):
            ref, st, trl = H.expected(b, encrypt)
            assert (st[b.malformed] == O.EINVAL).all() and (st[~b.malformed & ~b.tampered] == 0).all()
            assert ((trl != 0) == ((st == 0) & (not encrypt))).all()


_HASH = {1: hashlib.sha1, 256: hashlib.sha256, 384: hashlib.sha384, 512: hashlib.sha512}


@pytest.mark.parametrize("kind", list(H.ETA_KINDS))
def test_oracle_icv_is_hashlib_hmac_at_every_length(kind):
    """The ICV of an oracle-encrypted record is HMAC(akey, rec[:hl + ct] ||
    be32(esn_hi) with ESN)[:mlen], recomputed with Python's hmac, for every
    length of the kind's set; the oracle decrypts what it encrypted, answers
    EBADMSG for the tampered records and EINVAL for the empty payload."""
    b = H.eta_uniform(kind)
    sa = b.sas[0]
    ref, st = oracle_decrypt(b.sas, b.bad, b.descs, b.eh)
    ok = ~b.malformed & ~(b.tampered & (sa.mlen > 0))
    assert (st[ok] == 0).all() and (st[b.malformed] == O.EINVAL).all()
    assert sa.noauth or (st[b.tampered] == O.EBADMSG).all()
    for i in range(0, b.n, 7):                       # 9 or 10 records of every length
        o, L = int(b.descs["off4"][i]) * 4, int(b.descs["len"][i])
        if b.malformed[i] or b.tampered[i]:
            continue
        rec = b.bad[o:o + L].tobytes()
        if not sa.noauth:
            msg = rec[:L - sa.mlen] + (int(b.eh[i]).to_bytes(4, "big") if sa.esn else b"")
            assert rec[L - sa.mlen:] == hmac.new(sa.akey, msg, _HASH[sa.sha]).digest()[:sa.mlen], b.where(i)
        assert ref[o + sa.hlen:o + L - sa.mlen].tobytes() == b.plain[o + sa.hlen:o + L - sa.mlen].tobytes()


@needs_openssl
def test_openssl_gcm_matches_oracle_at_every_length():
    b = H.gcm_uniform(0)
    sa = b.sas[0]
    ref, st_ref = oracle_decrypt(b.sas, b.bad, b.descs, b.eh)
    work = b.bad.copy()
    _, st = ossl_esp.batch_decrypt("gcm", [sa.key], work, b.descs["off4"], b.descs["len"], b.descs["sa"],
                                   salts=[sa.salt], mlen=16, nthreads=4)
    assert (st == st_ref).all(), b.where(np.argmax(st != st_ref))
    assert (st[b.tampered] == O.EBADMSG).all() and (st[b.malformed] == O.EINVAL).all()
    assert int((st == 0).sum()) == b.n - 16 - int(b.tampered.sum())
    okm = H._payload_mask(b.descs, st == 0, len(work), b.sas)
    assert (work[okm] == ref[okm]).all() and (ref[okm] == b.plain[okm]).all()


@needs_openssl
def test_openssl_cbc_sha1_matches_oracle_at_every_length():
    b = H.eta_uniform("cbc128-sha1")
    sa = b.sas[0]
    ref, st_ref = oracle_decrypt(b.sas, b.bad, b.descs, b.eh)
    work = b.bad.copy()
    _, st = ossl_esp.batch_decrypt("cbc_sha1", [sa.key], work, b.descs["off4"], b.descs["len"], b.descs["sa"],
                                   akeys=[sa.akey], mlen=12, nthreads=4)
    assert (st == st_ref).all(), b.where(np.argmax(st != st_ref))
    assert (st[b.tampered] == O.EBADMSG).all() and (st[b.malformed] == O.EINVAL).all()
    assert (work == ref).all()       # verified records decrypted in place, failed ones untouched
