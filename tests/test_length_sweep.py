"""CPU side of the payload-length sweeps (sweep_helpers.py): the length sets,
short and long, cover what they were chosen for, the mixed layouts are what
their families prescribe, the long layouts stay under their arena cap, and the
oracle's record composition at the sweep lengths is pinned
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


# ---------------------------------------------------------------------------
# long records (test_long_records_gpu.py)

def test_long_length_sets():
    for _, _, mlen in H.GCM_SESSIONS:
        top = 65532 - 16 - mlen
        lens = H.GCM_LONG_LENS(mlen)
        want = set(range(8936, 8961, 4)) | set(range(top - 48, top + 1, 4))
        for k in (3, 4, 7, 8, 15):
            want |= set(range(4096 * k - 48, 4096 * k + 1, 4))
        assert len(lens) == 85 and lens == sorted(want) and all(L % 4 == 0 for L in lens)
        assert H.gcm_top(mlen) == top and lens[-1] == top and lens[0] > max(H.GCM_LENS)
    assert {(k >> b) & 1 for k in H.GCM_LONG_KEYS for b in range(4)} == {0, 1}
    assert all({(k >> b) & 1 for k in H.GCM_LONG_KEYS} == {0, 1} for b in range(4))
    for kind in H.ETA_KINDS:
        sa = H.eta_sa(np.random.default_rng(0), kind)
        assert H.eta_hlen_mlen(kind) == (sa.hlen, sa.mlen)
        room = 65532 - sa.hlen - sa.mlen
        lens = H.eta_long_lens(kind)
        assert len(lens) == 18 and lens == sorted(set(lens)) and lens[0] > max(H.eta_lens(kind))
        if kind.startswith("cbc"):
            assert lens[:10] == [16 * nb for nb in list(range(556, 564)) + [1024, 2048]]
            # the eight largest whole-block payloads that fit: one block more does not
            assert lens[10:] == [16 * (room // 16 - k) for k in range(7, -1, -1)]
            assert lens[-1] <= room < lens[-1] + 16
        else:
            assert lens[:10] == list(range(8936, 8965, 4)) + [16388, 32764]
            assert room % 4 == 0 and lens[10:] == list(range(room - 28, room + 1, 4))
        assert H.eta_top(kind) == lens[-1]
        assert sa.hlen + lens[-1] + sa.mlen <= 65532 < sa.hlen + lens[-1] + sa.mlen + (16 if sa.hlen == 24 else 4)
    # a record of the largest length a descriptor carries exists for GCM, CTR and NULL
    assert all(16 + H.gcm_top(m) + m == 65532 for _, _, m in H.GCM_SESSIONS)


def test_gcm_long_lengths_and_the_counter_cache_key():
    """CT block i takes counter i + 2 and the cache is keyed on ctr >> 8: for
    every window, which keys its lengths run through and on which side of the
    change the last block lies, at every last-block size on either side."""
    for k in range(1, 16):
        c = H.gcm_ctr_edge(k)
        assert c % 16 == 0 and (c // 16 + 2) == 256 * k          # the block that starts at c_k is the first of key k
    assert [H.gcm_ctr_edge(k) for k in (1, 2)] == [4064, 8160]   # the two the short sweep crosses
    for _, _, mlen in H.GCM_SESSIONS:
        lens = H.GCM_LONG_LENS(mlen)
        for k in H.GCM_LONG_KEYS:
            c = H.gcm_ctr_edge(k)
            win = [L for L in lens if c - 16 <= L <= c + 32]
            assert len(win) == 13
            before = [L for L in win if H.gcm_ctr_keys(L)[1] == k - 1]
            after = [L for L in win if H.gcm_ctr_keys(L)[1] == k]
            assert before == [L for L in win if L <= c] and after == [L for L in win if L > c]
            assert len(before) == 5 and len(after) == 8
            for side, top_key in ((before, k - 1), (after, k)):
                assert {H.gcm_shape(L, 4)[2] for L in side} == {4, 8, 12, 16}
                assert all(H.gcm_ctr_keys(L)[0] == list(range(top_key + 1)) for L in side)
            # a record that ends exactly at the change, and one whose last block is the first of key k
            assert c in before and H.gcm_nct(c) + 1 == 256 * k - 1 and H.gcm_nct(c + 4) + 1 == 256 * k
        jumbo = [L for L in lens if 8936 <= L <= 8960]
        assert len(jumbo) == 7 and all(H.gcm_ctr_keys(L) == ([0, 1, 2], 2) for L in jumbo)
        assert {H.gcm_shape(L, 4)[2] for L in jumbo} == {4, 8, 12, 16}
        top = [L for L in lens if L >= H.gcm_top(mlen) - 48]
        # c_16 = 65504: only the 8-byte ICV leaves room for a payload past it, one block of 4 bytes
        # under key 16; every other record ends under key 15
        assert len(top) == 13 and all(H.gcm_ctr_keys(L)[1] == (16 if L > H.gcm_ctr_edge(16) else 15) for L in top)
        assert [L for L in top if L > H.gcm_ctr_edge(16)] == ([65508] if mlen == 8 else [])
        assert {H.gcm_shape(L, 4)[2] for L in top} == {4, 8, 12, 16}
        # the last blocks' keys over the whole set
        assert {H.gcm_ctr_keys(L)[1] for L in lens} == {2, 3, 4, 6, 7, 8, 14, 15} | ({16} if mlen == 8 else set())
        # every front padding of the 4-lane schedule (the step parities belong to the short set)
        assert {H.gcm_shape(L, 4)[1] for L in lens} == set(range(4))


def test_gcm_long_aligned_lengths_step_back_from_every_key():
    """The aligned schedule's J0 slot is the one backward step of a lane's
    counter.  The short sweep takes it from keys 0 and 1 and GCM_LONG_LENS from
    2, 3, 6, 7, 14 and 15: never from 4 or 8, the keys that differ from key 0
    in one bit.  GCM_LONG_ALIGNED takes it from every key of GCM_LONG_KEYS."""
    assert {H.gcm_j0_back_key(L) for L in H.GCM_LENS} - {None} == {0, 1}
    for _, _, mlen in H.GCM_SESSIONS:
        back = {H.gcm_j0_back_key(L) for L in H.GCM_LONG_LENS(mlen)} - {None}
        assert back == {2, 3, 6, 7, 14, 15}
    lens = H.GCM_LONG_ALIGNED()
    assert lens == [12324, 12336, 16420, 16432, 28708, 28720, 32804, 32816, 61476, 61488]
    assert all(H.gcm_aligned(L) and H.gcm_nct(L) % 4 == 3 for L in lens)
    assert [H.gcm_j0_back_key(L) for L in lens] == [3, 3, 4, 4, 7, 7, 8, 8, 15, 15]
    assert [H.gcm_shape(L, 4)[2] for L in lens] == [4, 16] * 5 and max(lens) <= min(H.gcm_top(m) for m in (8, 12, 16))
    # slot nct - 4 (counter nct - 2) is the J0 lane's: the lane of slot nct
    assert all((H.gcm_nct(L) - 4) % 4 == H.gcm_nct(L) % 4 == 3 for L in lens)
    for si in range(len(H.GCM_SESSIONS)):
        b = H.gcm_long_aligned(si)
        assert b.n == 160 and len(b.plain) <= 5 << 20 and not b.malformed.any()
        t = b.tampered.reshape(-1, 16)
        assert not t[::2].any() and (t[1::2].sum(axis=1) == 1).all()
        _classes(b)


@pytest.mark.parametrize("kind", [k for k in H.ETA_KINDS if k.startswith("cbc") and "noauth" not in k])
def test_cbc_long_lengths_cover_every_residue_of_the_hashed_length(kind):
    """556..563 blocks: the hashed length hlen + payload (+ 4 with ESN) takes
    all eight residues mod 128 and all four mod 64 that whole blocks reach."""
    sa = H.eta_sa(np.random.default_rng(0), kind)
    base = sa.hlen + (4 if sa.esn else 0)
    hashed = [base + L for L in H.CBC_LONG_LENS(kind)[:8]]
    assert len({h % 128 for h in hashed}) == 8 and len({h % 64 for h in hashed}) == 4
    assert {h % 128 for h in hashed} == {(base + 16 * j) % 128 for j in range(8)}
    # with and without the ESN word the residues differ by 4: both sets are run
    assert {h % 16 for h in hashed} == {base % 16}
    B = H.HASH_BLOCK[sa.sha]
    assert any(h % B + 1 + B // 8 > B for h in hashed)           # a length whose padding needs a block more


def test_long_cbc_kinds_run_with_and_without_esn():
    esn = {bool(H.ETA_KINDS[k].get("esn")) for k in H.MIXED_KINDS if k.startswith("cbc") and "noauth" not in k}
    assert esn == {False, True}


def test_long_layouts_stay_under_the_arena_cap():
    """Every long layout's arena, from the lengths alone (the uniform ones are
    built below): at most 48 MiB."""
    for si, (_, _, mlen) in enumerate(H.GCM_SESSIONS):
        size = H.arena_bytes(np.repeat(H.GCM_LONG_LENS(mlen), H.GCM_RUN) + 16 + mlen)
        assert 44.0 <= round(size / 2**20, 1) <= 44.1 and size <= H.LONG_ARENA_CAP
    for kind in H.ETA_KINDS:
        hlen, mlen = H.eta_hlen_mlen(kind)
        size = H.arena_bytes(np.repeat(H.eta_long_lens(kind), H.ETA_UNIT) + hlen + mlen)
        assert 39.3 <= round(size / 2**20, 1) <= 39.5 and size <= H.LONG_ARENA_CAP
    # 517 GCM records, or 485 ETA ones, cannot reach it even if all had the largest length
    assert (H.GCM_LONG_WAVES * 16 + 5) * (65532 + 8) + 64 <= H.LONG_ARENA_CAP
    assert (H.ETA_LONG_UNITS * 64 - 27) * (65532 + 4) + 64 <= H.LONG_ARENA_CAP


def _classes(b):
    for encrypt in (False, True):
        ref, st, trl = H.expected(b, encrypt)
        auth = np.array([s.mlen > 0 for s in b.sas])[b.descs["sa"]]
        assert (st[b.malformed] == O.EINVAL).all() and (st[~b.malformed & ~b.tampered] == 0).all()
        if not encrypt:
            assert (st[b.tampered & auth] == O.EBADMSG).all() and (st[b.tampered & ~auth] == 0).all()
        assert ((trl != 0) == ((st == 0) & (not encrypt))).all()


@pytest.mark.parametrize("si", range(len(H.GCM_SESSIONS)), ids=H.GCM_SESSION_IDS)
def test_gcm_long_uniform_layout_and_oracle(si):
    """1360 records, 44.0 MiB; two tampered records in every second run; the
    oracle answers EBADMSG exactly for them, decrypting, and 0 for all
    encrypting."""
    b = H.gcm_long_uniform(si)
    mlen = H.GCM_SESSIONS[si][2]
    assert b.n == 85 * 16 == 1360 and len(b.plain) <= H.LONG_ARENA_CAP
    assert round(len(b.plain) / 2**20, 1) == 44.0
    assert len(b.plain) == H.arena_bytes(b.descs["len"])
    pl = np.array([b.payload(i) for i in range(b.n)]).reshape(-1, 16)
    assert (pl == np.array(H.GCM_LONG_LENS(mlen))[:, None]).all() and int(b.descs["len"].max()) == 65532
    t = b.tampered.reshape(-1, 16)
    assert not t[::2].any() and (t[1::2].sum(axis=1) == 2).all() and not b.malformed.any()
    assert len(set(np.nonzero(t)[1])) >= 8                       # the tampered lanes rotate
    _classes(b)
    assert H.gcm_long_uniform(si) is b                           # kept while no other long layout is asked for


@pytest.mark.parametrize("kind", H.MIXED_KINDS)
def test_eta_long_uniform_layout_and_oracle(kind):
    """1152 records, 39.4 MiB; even units intact, three tampered records in
    every odd one, no prefix of the unit verified."""
    b = H.eta_long_uniform(kind)
    assert b.n == 18 * 64 == 1152 and len(b.plain) <= H.LONG_ARENA_CAP
    assert round(len(b.plain) / 2**20, 1) == 39.4
    pl = np.array([b.payload(i) for i in range(b.n)]).reshape(-1, 64)
    assert (pl == np.array(H.eta_long_lens(kind))[:, None]).all()
    t = b.tampered.reshape(-1, 64)
    assert not t[::2].any() and (t[1::2].sum(axis=1) == 3).all() and not b.malformed.any()
    assert all(not r[:61].all() for r in ~t[1::2]) and len(set(np.nonzero(t)[1])) >= 20
    # the equal-length path's block counts: intact units at 1024 blocks or beyond, the longest one block
    # short of the kind's largest record (the largest itself is a tampered unit)
    nbu = (pl[::2, 0] + 15) // 16
    assert (nbu >= 1024).sum() >= 5 and nbu.max() >= (H.eta_top(kind) + 15) // 16 - 1 >= 4090
    _classes(b)


def test_one_long_layout_is_kept_at_a_time():
    a = H.gcm_long_mixed()
    assert H.gcm_long_mixed() is a
    H.eta_long_mixed("null-sha1")
    assert len(H._long_slot) == 1 and H.gcm_long_mixed() is not a


def test_gcm_long_mixed_is_what_it_prescribes():
    for foreign in (True, False):
        b = H.gcm_long_mixed(foreign)
        assert b.n == 32 * 16 + 5 and len(b.plain) <= H.LONG_ARENA_CAP
        pl = np.array([b.payload(i) for i in range(b.n)])
        tops = np.array([H.gcm_top(b.sas[s].mlen) for s in (np.arange(b.n) // 256 % 2)])
        good = ~b.malformed
        assert (pl[good] % 4 == 0).all() and pl[good].min() >= 4 and (pl[good] <= tops[good]).all()
        waves = pl[:512].reshape(32, 16)
        ok = good[:512].reshape(32, 16)
        assert ((waves > 32768) & ok).any(axis=1).all() and ((waves < 64) & ok).any(axis=1).all()
        assert len(set(np.argmax(waves, axis=1))) >= 8           # the long record's lane rotates
        # log-uniform: every octave from 4 bytes to 64 KiB is drawn, none holds half the records
        octave = np.bincount(np.log2(pl[good]).astype(int), minlength=16)[2:16]
        assert (octave >= 10).all() and octave.max() < b.n // 4
        # every lane of a wave changes its cache key at steps of its own: many distinct last keys per wave
        keys = np.array([[H.gcm_ctr_keys(L)[1] for L in w] for w in waves])
        assert np.median([len(set(w)) for w in keys]) >= 4 and set(keys.reshape(-1)) == set(range(16))
        # two sessions, one per aligned run of 256 records; guard bytes between records
        own = np.where(b.foreign, 1 - b.descs["sa"], b.descs["sa"])
        assert (own == np.arange(b.n) // 256 % 2).all() and b.sas[0].mlen != b.sas[1].mlen
        gaps = np.diff(b.descs["off4"].astype(np.int64)) * 4 - ((b.descs["len"][:-1].astype(np.int64) + 3) & ~3)
        assert (gaps >= 4).all()                                 # 8, or 4 where the descriptor's len grew by 2
        assert 0.02 < b.tampered.mean() < 0.08
        assert (b.descs["len"] % 4 == 2).sum() == 13 and b.descs["len"][b.n - 2] % 4 == 2
        assert int(b.foreign.sum()) == (12 if foreign else 0) and not b.foreign[::4].any()
        assert (b.malformed == (b.foreign | (b.descs["len"] % 4 == 2))).all()
        _classes(b)


@pytest.mark.parametrize("kind", H.MIXED_KINDS)
def test_eta_long_mixed_is_what_it_prescribes(kind):
    b = H.eta_long_mixed(kind)
    cbc = kind.startswith("cbc")
    assert b.n == 8 * 64 - 27 and len(b.plain) <= H.LONG_ARENA_CAP
    pl = np.array([b.payload(i) for i in range(b.n)])
    top = H.eta_top(kind)
    lanes = []
    for u in range(8):
        unit = pl[u * 64:(u + 1) * 64]
        ok = ~b.malformed[u * 64:(u + 1) * 64]
        assert ((unit == top) & ok).sum() >= 1 and unit.max() == top
        lanes.append(int(np.argmax(unit)))
    assert len(set(lanes)) == 8 and b.sas[0].hlen + top + b.sas[0].mlen > 65532 - 16
    good = ~b.malformed
    assert (pl[good] % (16 if cbc else 4) == 0).all() and pl[good].min() >= (16 if cbc else 4)
    octave = np.bincount(np.log2(pl[good]).astype(int), minlength=16)[4:16]
    assert (octave >= 10).all() and octave.max() < b.n // 4
    assert (pl == 0).sum() == 8 and b.orphan.sum() == 8 and 0.02 < b.tampered.mean() < 0.09
    short = (pl % 16 == 12) & (b.descs["len"] > 0) if cbc else np.zeros(b.n, dtype=bool)
    assert int(short.sum()) == (8 if cbc else 0)
    assert (b.malformed == ((pl == 0) | b.orphan | short)).all()
    _classes(b)


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
