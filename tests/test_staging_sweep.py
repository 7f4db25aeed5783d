"""CPU side of the staging sweeps (staging_helpers.py): the layouts cover what
they were chosen for, asserted from the layouts themselves and from the
engine's rules as restated in the helper (the small-batch bound, launch_gcm's
chunk size, stage_in's threads per record); and the helper's expected bytes
are pinned to the oracle record by record, for one layout per family."""
import hashlib
import hmac

import numpy as np
import pytest

import oracle as O
import staging_helpers as S

_HASH = {1: hashlib.sha1, 512: hashlib.sha512}


def _guards(lay, lead):
    """Every registered record keeps GUARD bytes before its lead bytes and
    after its end that belong to no other record."""
    regd = np.nonzero(lay.reg_off >= 0)[0]
    s, e = lay.reg_off[regd] - lead, lay.reg_off[regd] + lay.L[regd]
    assert (s[0] >= 64) and (s[1:] - e[:-1] >= S.GUARD).all() and lay.reg_size - e[-1] >= S.GUARD
    return regd


def test_rules_restated():
    assert S.slot_stat_off([44, 1480]) == 48 + 1488 + 16 + 32
    # launch_gcm: 8 (fused) or 4 (burst) records, doubled while below ceil(n / grid), at most 256
    assert [S.gcm_chunk(n, 1, False) for n in (1, 8, 9, 100, 256, 300)] == [8, 8, 16, 128, 256, 256]
    assert [S.gcm_chunk(n, 1, True) for n in (1, 4, 5, 100, 129, 300)] == [4, 4, 8, 128, 256, 256]
    assert S.gcm_chunk(100, 256, False) == 8 and S.gcm_chunk(4096, 256, True) == 16
    # stage_in: the largest power of two <= 64 with tpr * count <= WG
    assert [S.stage_tpr(c, 1024) for c in (1, 16, 17, 32, 64, 65, 128, 129, 256)] == [64, 64, 32, 32, 16, 8, 8, 4, 4]
    assert [S.stage_tpr(c, 512) for c in (8, 9, 16, 32, 33, 64, 65, 128, 129, 256)] == [64, 32, 32, 16, 8, 8, 4, 4, 2, 2]


def test_a_every_length_class_at_every_residue_for_every_kind():
    lay = S.esp_residues()
    _guards(lay, S.SKIP)
    assert lay.kinds == list(S.ESP_KINDS) and len(lay.kinds) == 7
    assert sorted({s.hlen for s in lay.sas}) == [8, 16, 24]
    have = {(int(k), int(L) % 16, int(r)) for k, L, r, g in zip(lay.sa, lay.L, lay.res, lay.registered) if g}
    for k, kind in enumerate(lay.kinds):
        sa = lay.sas[k]
        # the lengths a record of this kind can have: payload a multiple of 4, of 16 for AES-CBC
        step = 16 if S.is_cbc(kind) else 4
        classes = {(sa.hlen + p + sa.mlen) % 16 for p in range(step, 17 * step, step)}
        assert classes == ({0, 4, 8, 12} if step == 4 else {(sa.hlen + sa.mlen) % 16})
        assert {(m, r) for kk, m, r in have if kk == k} == {(m, r) for m in classes for r in range(16)}, kind
    assert (lay.reg_off[lay.registered] % 16 == lay.res[lay.registered]).all()
    # staged records of every kind beside them, a tenth tampered, of both classes; long and short records
    assert {int(k) for k in lay.sa[~lay.registered]} == set(range(7))
    assert lay.tampered.sum() == lay.n // 10 and lay.tampered[lay.registered].any() and lay.tampered[~lay.registered].any()
    assert lay.L.min() < 48 and lay.L.max() > 1448
    assert all(S.slot_stat_off(lay.L[g]) <= S.SMALL_BATCH for g in lay.groups)
    assert sorted(i for g in lay.groups for i in g) == list(range(lay.n))
    et, _ = S.expect(lay, False)
    auth = np.array([lay.sa_of(i).mlen > 0 for i in range(lay.n)])
    assert (et == np.where(lay.tampered & auth, O.EBADMSG, 0)).all()


def test_b_piece_boundaries():
    small, large = S.esp_pieces(False), S.esp_pieces(True)
    for lay in (small, large):
        _guards(lay, S.SKIP)
        assert lay.registered.all() and lay.n == 2 * len(S.PIECE_LENS) * len(S.PIECE_RES)
        gcm = lay.sa == 0
        for r in S.PIECE_RES:
            assert sorted(lay.L[gcm & (lay.res == r)]) == list(S.PIECE_LENS)
            assert sorted(lay.L[~gcm & (lay.res == r)]) == [4084, 4100, 4100, 8180, 8196, 8196, 65524]
        assert (lay.reg_off % 16 == lay.res).all() and lay.tampered.sum() == lay.n // 10
    # AES-CBC + HMAC-SHA1 records are 36 + 16 k bytes: the nearest to each of PIECE_LENS
    assert all((L - 36) % 16 == 0 for L in (4084, 4100, 8180, 8196, 65524))
    # the record on its way in ends 4 before, on and 4 after the first and the second piece boundary; the
    # result on its way out starts hlen into the record, so its pieces split elsewhere in the packet
    ends = {int(L) - k * S.PIECE for L in S.PIECE_LENS for k in (1, 2)}
    assert {-4, 0, 4} <= ends
    for lay in (small,):
        for i in range(lay.n):
            sa = lay.sa_of(i)
            cuts_in = set(range(S.PIECE, int(lay.L[i]), S.PIECE))
            cuts_out = {sa.hlen + c for c in range(S.PIECE, int(lay.L[i]) - sa.hlen - sa.mlen, S.PIECE)}
            assert not cuts_in & cuts_out
    assert 65532 // S.PIECE == 15 and 65532 % S.PIECE == S.PIECE - 4
    assert len(small.groups) > 6 and all(S.slot_stat_off(small.L[g]) <= S.SMALL_BATCH for g in small.groups)
    assert len(large.groups) == 1 and S.slot_stat_off(large.L) > S.SMALL_BATCH


@pytest.mark.parametrize("sha,esn", S.AH_SESSIONS, ids=S.AH_IDS)
def test_c_every_byte_length_and_every_pair_of_length_class_and_residue(sha, esn):
    lay = S.ah_layout(sha, esn)
    m, blk = lay.sa.mlen, S.BLOCK[sha]
    assert m == {1: 12, 512: 32}[sha] and lay.sa.esn == esn
    assert sorted(set(lay.L)) == list(range(m, 2 * blk + 9))
    per_len = {}
    for L, r in zip(lay.L, lay.res):
        per_len.setdefault(int(L), set()).add(int(r))
    assert all(len(v) >= 2 for v in per_len.values())
    assert {(int(L) % 16, int(r)) for L, r in zip(lay.L, lay.res)} == {(a, b) for a in range(16) for b in range(16)}
    assert (lay.reg_off % 16 == lay.res).all()
    assert (lay.doff % 4 == 0).all() and (lay.doff + m <= lay.L).all() and len(set(lay.doff % 16)) == 4
    s, e = lay.reg_off, lay.reg_off + lay.L
    assert (s[1:] - e[:-1] >= S.AH_LEAD).all() and s[0] >= 64
    assert all(S.slot_stat_off(lay.L[g] + 2 * S.AH_LEAD) <= S.SMALL_BATCH for g in lay.groups)
    # the reference is Python's hmac: COMPUTE over the range as it stands, the field's bytes included
    signed, bad, et = S.ah_expect(lay)
    for i in range(0, lay.n, 7):
        o, L, d = int(lay.reg_off[i]), int(lay.L[i]), int(lay.doff[i])
        msg = lay.arena[o:o + L].tobytes() + (int(lay.eh[i]).to_bytes(4, "big") if esn else b"")
        assert signed[o + d:o + d + m].tobytes() == hmac.new(lay.sa.key, msg, _HASH[sha]).digest()[:m], i
    field = np.zeros(lay.reg_size, dtype=bool)
    for o, d in zip(lay.reg_off, lay.doff):
        field[o + d:o + d + m] = True
    assert (signed[~field] == lay.arena[~field]).all() and (bad != signed).sum() == lay.tampered.sum() == lay.n // 10
    # a VERIFY whose range holds its own digest cannot match: EBADMSG for every request, tampered or not
    assert (et == O.EBADMSG).all()


@pytest.mark.parametrize("kernel", ["fused", "burst"])
def test_d_batch_sizes_reach_every_threads_per_record(kernel):
    """On one workgroup (grid 1) the chosen n reach every tpr of the kernel,
    a short last chunk, and at every tpr staged and registered records of
    every length class."""
    want = {"fused": {64, 32, 16, 8, 4}, "burst": {64, 32, 16, 8, 4, 2}}[kernel]
    ns = S.STAGE_N[kernel]
    assert ns == {"fused": (8, 16, 24, 40, 100, 200, 256, 300), "burst": (4, 8, 12, 24, 40, 100, 200, 256, 300)}[kernel]
    chunks = [S.gcm_chunk(n, 1, kernel == "burst") for n in ns]
    assert chunks == {"fused": [8, 16, 32, 64, 128, 256, 256, 256], "burst": [4, 8, 16, 32, 64, 128, 256, 256, 256]}[kernel]
    assert {t for n in ns for t in S.record_tpr(n, 1, kernel)} == want
    assert len(set(S.record_tpr(300, 1, kernel))) == 2                     # the last chunk: 44 records
    # with the default 256 workgroups none of this is reached
    assert {t for n in ns for t in S.record_tpr(n, 256, kernel)} == {64}
    for kind in S.STAGE_SESSIONS:
        seen = {}
        for n in ns:
            lay = S.esp_stage(kind, n)
            assert lay.n == n and len(lay.groups) == 1 and S.slot_stat_off(lay.L) <= S.SMALL_BATCH, n
            assert {int(L) % 16 for L in lay.L} == {0, 4, 8, 12}, n
            assert abs(int(lay.registered.sum()) - n // 2) <= 1 and lay.tampered.sum() == max(1, n // 8)
            assert (lay.reg_off[lay.registered] % 16 == lay.res[lay.registered]).all()
            if n >= 40:
                assert set(lay.res[lay.registered]) == set(range(16)), n
            if n >= 8:
                assert lay.L.max() > 1448 and lay.L.min() <= 48
            for t, L, g in zip(S.record_tpr(n, 1, kernel), lay.L, lay.registered):
                seen.setdefault(t, set()).add((int(L) % 16, bool(g)))
        for t in want - {64}:
            assert seen[t] == {(m, g) for m in (0, 4, 8, 12) for g in (False, True)}, (kind, t)
        # the records the unstrided copy lost bytes of: both sides 16-aligned, more loose bytes than threads
        assert all((12, False) in seen[t] for t in (8, 4)) and (8, False) in seen[4]
    # e. the batch behind a live door: 100 records on 65 - 64 = 1 workgroup
    assert set(S.record_tpr(100, 1, "fused")) == {8} and set(S.record_tpr(100, 65, "fused")) == {64}
    assert S.slot_stat_off(S.esp_stage(S.STAGE_SESSIONS[0], 32).L) <= S.SMALL_BATCH


@pytest.mark.parametrize("family", ["a", "b", "d"])
def test_expected_bytes_are_the_oracles(family):
    """expect() against the oracle's single-record entry points, record by
    record: esp_encrypt of the plaintext record; esp_decrypt of what
    esp_input is given, its status, and for an accepted record its payload
    between the header and ICV as given."""
    lay = {"a": S.esp_residues, "b": lambda: S.esp_pieces(False),
           "d": lambda: S.esp_stage(S.STAGE_SESSIONS[1], 100)}[family]()
    et_e, enc = S.expect(lay, True)
    et_d, dec = S.expect(lay, False)
    assert (et_e == 0).all()
    given = lay.records(lay.bad)
    for i, plain in enumerate(lay.records(lay.plain)):
        sa, eh = lay.sa_of(i), int(lay.eh[i])
        e, ct = sa.oracle.esp_encrypt(plain, eh)
        assert e == 0 and ct == enc[i], lay.where(i, "cpu")
        assert (given[i] != enc[i]) == bool(lay.tampered[i])
        e, pt = sa.oracle.esp_decrypt(given[i], eh)
        assert e == et_d[i], lay.where(i, "cpu")
        h, a, L = sa.hlen, sa.mlen, len(plain)
        if e == 0:
            assert dec[i] == given[i][:h] + pt[h:L - a] + given[i][L - a:], lay.where(i, "cpu")
            if not lay.tampered[i]:
                assert dec[i][h:L - a] == plain[h:L - a]
        else:
            assert e == O.EBADMSG and lay.tampered[i] and dec[i] == given[i]
    # the images: packets where the layout says, zeros between them
    img = lay.image(enc)
    mask = np.zeros(lay.reg_size, dtype=bool)
    for i in np.nonzero(lay.registered)[0]:
        s, L = int(lay.reg_off[i]), int(lay.L[i])
        assert img[s - S.SKIP:s].tobytes() == lay.hdr[i].tobytes() and img[s:s + L].tobytes() == enc[i]
        assert not mask[s - S.SKIP - S.GUARD:s + L + S.GUARD].any() or not mask[s - S.SKIP:s + L].any()
        mask[s - S.SKIP:s + L] = True
    assert not img[~mask].any() and lay.hdr.all()
