"""espgpu_esp_classify_batch (classify.hip): header sanity and SPI lookup for a
device-resident batch.  Every test compares the device batch with the host
rule espgpu_esp_classify (pinned against esp.py's restatement of the
reference in test_esp_classify.py) applied in index order: all of d_desc and
d_cstatus with guard entries past n, and the arena and the table unchanged."""
import numpy as np
import pytest

import oracle as O
from classify_helpers import (KINDS, Sadb, chain_spis, dst_of, esp_payload, host_classify_batch, ipv4, ipv6, layout,
                              random_packets)
from helpers import DESC, EtaSA, GcmSA, build_records, oracle_decrypt

EACCES, EINVAL = 13, 22
GUARD = 5


def _torch():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.fail("GPU test run without a visible HIP device")
    return torch


@pytest.fixture(scope="module")
def drv():
    _torch()
    from espgpu.opencrypto import GpuCryptoDriver
    d = GpuCryptoDriver(max_sessions=64, batch_records=1024, batch_bytes=1 << 20, nbatches=1)
    yield d
    d.close()
    import gc
    gc.collect()


@pytest.fixture(scope="module")
def mixed():
    """The module's pool: 3000 packets of every kind over 40 SAs, laid out once."""
    from espgpu.batch import sad_build
    rng = np.random.default_rng(60)
    db = Sadb(rng, nesp4=20, nesp6=16, nah=4)
    kp = random_packets(rng, db, 3000, good=0.6)
    arena, rec = layout(rng, [p for _, p in kp])
    return db, sad_build(db.entries, 128), [k for k, _ in kp], arena, rec


def _up(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()


def _classify(drv, arena, rec, table, flags=0, calls=None, stream=None):
    """Upload, esp_classify (once, or per (start, count, table) of `calls` back
    to back without a sync), download and compare everything with the host
    rule.  Returns the device (desc, cstatus)."""
    torch = _torch()
    from espgpu.batch import esp_classify
    n = len(rec)
    calls = calls or [(0, n, table)]
    d_arena, d_rec = _up(torch, arena), _up(torch, rec)
    d_tabs = [_up(torch, t) for _, _, t in calls]
    d_desc = torch.full(((n + GUARD) * 16,), 0xC3, dtype=torch.uint8, device="cuda")
    d_cst = torch.full((n + GUARD,), 0x77, dtype=torch.uint8, device="cuda")
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
    for (a, cnt, _), d_tab in zip(calls, d_tabs):
        esp_classify(drv, d_arena, d_rec[a * 8:], cnt, d_tab, d_desc[a * 16:], d_cst[a:], flags=flags, stream=stream)
    if stream is not None:
        stream.synchronize()
    else:
        torch.cuda.synchronize()
    w_desc, w_cst = np.zeros(n, dtype=DESC), np.zeros(n, dtype=np.uint8)
    for a, cnt, t in calls:
        w_desc[a:a + cnt], w_cst[a:a + cnt] = host_classify_batch(t, arena, rec[a:a + cnt], flags)
    g_desc, g_cst = d_desc.cpu().numpy(), d_cst.cpu().numpy()
    bad = np.flatnonzero(g_cst[:n] != w_cst)
    assert bad.size == 0, ("cstatus", bad[:8], g_cst[bad[:8]], w_cst[bad[:8]])
    gd = g_desc[:n * 16].view(DESC)
    bad = np.flatnonzero(gd != w_desc)
    assert bad.size == 0, ("desc", bad[:8], gd[bad[:8]], w_desc[bad[:8]])
    assert (g_cst[n:] == 0x77).all() and (g_desc[n * 16:] == 0xC3).all(), "wrote past n"
    assert np.array_equal(d_arena.cpu().numpy(), arena), "arena modified"
    for (_, _, t), d_tab in zip(calls, d_tabs):
        assert np.array_equal(d_tab.cpu().numpy(), t.view(np.uint8)), "table modified"
    assert np.array_equal(d_rec.cpu().numpy(), rec.view(np.uint8)), "d_pkt modified"
    return gd, g_cst[:n]


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [0, 1], ids=["nocsum", "ipcsum"])
def test_mixed_batch(drv, mixed, flags):
    """Every kind interleaved at an irregular stride, some with len > ip_len."""
    db, table, kinds, arena, rec = mixed
    assert set(kinds) == set(KINDS)
    desc, cst = _classify(drv, arena, rec, table, flags)
    ok = np.flatnonzero(cst == 0)
    assert 1000 < ok.size < 2500
    assert (desc["len"][ok] >= 8).all() and (desc["sa"][ok] < len(db.entries)).all()
    bad = np.flatnonzero(cst)
    assert (desc["len"][bad] == 0).all() and (desc["sa"][bad] == 0xffff).all()
    assert np.array_equal(desc["off4"][bad], rec["off4"][bad])
    assert {int(x) for x in np.unique(cst)} == {0, 2, 22, 95}


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1025])
def test_launch_edges(drv, mixed, n):
    _, table, _, arena, rec = mixed
    _classify(drv, arena, rec[7:7 + n], table, 1)


@pytest.mark.gpu
def test_zero_packets_and_arguments(drv, mixed):
    torch = _torch()
    _, table, _, arena, rec = mixed
    lib, ctx = drv.lib, drv.ctx
    d_arena, d_rec, d_tab = _up(torch, arena[:4096]), _up(torch, rec[:4]), _up(torch, table)
    d_desc = torch.zeros(64, dtype=torch.uint8, device="cuda")
    d_cst = torch.zeros(4, dtype=torch.uint8, device="cuda")
    args = (d_arena.data_ptr(), d_rec.data_ptr(), 4, d_tab.data_ptr(), 128, 0, d_desc.data_ptr(), d_cst.data_ptr(),
            None)
    assert lib.espgpu_esp_classify_batch(ctx, None, None, 0, None, 0, 0, None, None, None) == 0
    assert lib.espgpu_esp_classify_batch(None, *args) == EINVAL
    for k, v in ((0, None), (1, None), (3, None), (4, 0), (4, 96), (5, 2), (6, None), (7, None),
                 (0, d_arena.data_ptr() + 2), (3, d_tab.data_ptr() + 8)):
        a = list(args)
        a[k] = v
        assert lib.espgpu_esp_classify_batch(ctx, *a) == EINVAL, (k, v)
    assert lib.espgpu_health(ctx) == 0
    assert lib.espgpu_esp_classify_batch(ctx, *args) == 0
    torch.cuda.synchronize()


def _one_per_entry(rng, db, extra=()):
    pk = []
    for e in db.entries:
        p = esp_payload(rng, int(e["spi"]), 16)
        pk.append(ipv4(dst_of(e), p) if e["af"] == 4 else ipv6(dst_of(e), p))
    return pk + list(extra)


@pytest.mark.gpu
def test_table_of_two_slots(drv):
    from espgpu.batch import sad_build
    rng = np.random.default_rng(61)
    db = Sadb(rng, 1, 0, 0)
    pk = _one_per_entry(rng, db, [ipv4(dst_of(db.entries[0]), esp_payload(rng, db.unknown_spi(rng), 16))
                                  for _ in range(40)])
    arena, rec = layout(rng, pk)
    _, cst = _classify(drv, arena, rec, sad_build(db.entries, 2))
    assert cst[0] == 0 and (cst[1:] == 2).all()


@pytest.mark.gpu
def test_chain_wrapping_past_the_end(drv):
    """32 SPIs with one home slot in 64 slots: the chain runs 50 .. 63, 0 .. 17."""
    from espgpu.batch import sad_build
    rng = np.random.default_rng(62)
    spis = chain_spis(50, 64, 33)
    db = Sadb(rng, nesp4=16, nesp6=16, nah=0, spis=spis[:32])
    table = sad_build(db.entries, 64)
    assert sorted(np.flatnonzero(table["spi"])) == sorted((50 + j) % 64 for j in range(32))
    miss = [ipv4(dst_of(db.entries[0])[:4], esp_payload(rng, spis[32], 16)) for _ in range(3)]
    arena, rec = layout(rng, _one_per_entry(rng, db, miss))
    _, cst = _classify(drv, arena, rec, table)
    assert not cst[:32].any() and (cst[32:] == 2).all()


@pytest.mark.gpu
def test_large_table(drv):
    """131072 slots, 65535 entries, sampled by 4000 packets, a quarter of them misses."""
    from espgpu import shard
    from espgpu.batch import SAD_DTYPE, sad_build
    rng = np.random.default_rng(63)
    ns = 65535
    ent = np.zeros(ns, dtype=SAD_DTYPE)
    spis = np.array(shard.random_spis(ns + 1000, 64), dtype=np.uint32)
    rng.shuffle(spis)
    ent["spi"], ent["sa"], ent["proto"] = spis[:ns], np.arange(ns), 50
    ent["af"] = np.where(rng.random(ns) < 0.5, 4, 6)
    ent["salt"] = rng.integers(0, 2**32, ns)
    ent["dst"] = rng.integers(0, 256, (ns, 16))
    ent["dst"][:, 0] = 0x20
    ent["dst"][ent["af"] == 4, 4:] = 0
    table = sad_build(ent, 131072)
    pk = []
    for j in rng.integers(0, ns, 3000):
        e = ent[j]
        p = esp_payload(rng, int(e["spi"]), 16)
        pk.append(ipv4(dst_of(e), p) if e["af"] == 4 else ipv6(dst_of(e), p))
    pk += [ipv4(b"\x20\1\2\3", esp_payload(rng, int(s), 16)) for s in spis[ns:]]
    order = rng.permutation(len(pk))
    arena, rec = layout(rng, [pk[i] for i in order])
    _, cst = _classify(drv, arena, rec, table)
    assert (cst == 0).sum() == 3000 and (cst == 2).sum() == 1000


@pytest.mark.gpu
def test_callers_stream_and_a_rebuilt_table(drv, mixed):
    """Two calls on a caller's stream without a sync; the second reads a table
    rebuilt in another buffer after half the SAs went and the rest moved to
    other sessions."""
    torch = _torch()
    from espgpu.batch import sad_build
    db, table, _, arena, rec = mixed
    ent2 = db.entries[::2].copy()
    ent2["sa"] = 50 - np.arange(len(ent2))
    table2 = sad_build(ent2, 64)
    cut = 1400
    s = torch.cuda.Stream()
    desc, cst = _classify(drv, arena, rec, None, 1, calls=[(0, cut, table), (cut, len(rec) - cut, table2)], stream=s)
    assert (cst[cut:] == 2).sum() > (cst[:cut] == 2).sum()


@pytest.mark.gpu
def test_inbound_sequence_end_to_end(drv):
    """classify -> replay check -> decrypt in place with trailer words ->
    window update -> the three merges, on GCM and CBC+HMAC records behind IPv4
    (some with options) and IPv6 headers among fragments, TCP packets and
    unknown SPIs: the same as that sequence on descriptors built by the host
    rule, the classified records' plaintext is the oracle's, and a second
    batch replaying the first is refused."""
    torch = _torch()
    from espgpu.batch import (REPLAY_DTYPE, SAD_DTYPE, decrypt_batch, esp_classify, replay_check, replay_merge,
                              replay_update, sad_build)
    from test_replay_update_gpu import _tables
    rng = np.random.default_rng(64)
    sas = [GcmSA(rng), GcmSA(rng, esn=True), EtaSA(rng), EtaSA(rng, sha256=True)]
    afs, ihls = [4, 6, 4, 6], [5, 0, 7, 0]
    sids = []
    for s in sas:
        rc, sid = drv.newsession(s.esp_sa().csp())
        assert rc == 0
        sids.append(sid)
    nrec = 240
    sa_idx = rng.integers(0, 4, nrec)
    ct_lens = [16 * int(rng.integers(1, 9)) for _ in range(nrec)]
    seqs = [1001 + i for i in range(nrec)]
    his = np.where(sa_idx == 1, 3, 0).astype(np.uint32)
    plain, ct, rdesc, _ = build_records(rng, sas, sa_idx, ct_lens, seqs=seqs, esn_hi=his)
    want, wst = oracle_decrypt(sas, ct, rdesc, his)
    assert not wst.any()
    # the SAD: each SA under one family and destination
    ent = np.zeros(4, dtype=SAD_DTYPE)
    for k, s in enumerate(sas):
        ent["spi"][k], ent["sa"][k], ent["proto"][k], ent["af"][k] = s.spi, sids[k], 50, afs[k]
        ent["salt"][k] = int.from_bytes(s.salt, "little")
        m = 4 if afs[k] == 4 else 16
        ent["dst"][k, :m] = rng.integers(1, 255, m)
        ent["dst"][k, 0] = 0x20
    table = sad_build(ent, 8)
    noise_db = Sadb(rng, 4, 4, 2)                       # SPIs the table does not hold
    pk, src = [], []
    for i in range(nrec):
        o, ln, k = int(rdesc["off4"][i]) * 4, int(rdesc["len"][i]), int(sa_idx[i])
        body = ct[o:o + ln].tobytes()
        tail = bytes(int(rng.integers(0, 3)) * 2)
        if afs[k] == 4:
            ihl = ihls[k] + int(rng.integers(0, 2)) * (ihls[k] > 5)
            pk.append(ipv4(dst_of(ent[k]), body, ihl=ihl, opts=rng.integers(0, 256, ihl * 4 - 20, dtype=np.uint8),
                           tail=tail))
        else:
            pk.append(ipv6(dst_of(ent[k]), body, tail=tail))
        src.append(i)
        if rng.random() < 0.3:
            kind = ("frag", "proto4", "unknown4", "unknown6", "nxt6")[int(rng.integers(5))]
            pk.append(KINDS[kind][0](rng, noise_db))
            src.append(-1)
    src = np.array(src)
    n = len(pk)
    arena, rec = layout(rng, pk)
    h_desc, h_cst = host_classify_batch(table, arena, rec, 1)
    real = np.flatnonzero(src >= 0)
    assert not h_cst[real].any() and h_cst[src < 0].all()
    assert np.array_equal(h_desc["len"][real], rdesc["len"]) and np.array_equal(h_desc["sa"][real],
                                                                                 np.array(sids)[sa_idx])
    wins = [(0, 0, 0, 0, None)] * (max(sids) + 1)
    for k in range(4):
        wins[sids[k]] = ((3 << 32 | 999, 64, 32, O.REPLAY_ESN, None) if k == 1 else (1000, 64, 32, 0, None))
    tab, words = _tables(wins)

    def inbound(d_tab, d_words, device_classify):
        d_arena, d_rec, d_sad = _up(torch, arena), _up(torch, rec), _up(torch, table)
        mk = lambda: torch.zeros(n, dtype=torch.uint8, device="cuda")
        cst, rst, ust, st = mk(), mk(), mk(), mk()
        tr = torch.zeros(n, dtype=torch.int32, device="cuda")
        if device_classify:
            d_desc = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
            esp_classify(drv, d_arena, d_rec, n, d_sad, d_desc, cst, flags=1)
        else:
            d_desc, cst = _up(torch, h_desc), _up(torch, h_cst)
        replay_check(drv, d_arena, d_desc, n, d_tab, d_words, rst)
        decrypt_batch(drv, d_arena, d_desc, n, st, trailer=tr)
        replay_update(drv, d_arena, d_desc, n, st, d_tab, d_words, ust)
        replay_merge(drv, st, rst, n)
        replay_merge(drv, st, ust, n)
        replay_merge(drv, st, cst, n)
        torch.cuda.synchronize()
        return (st.cpu().numpy(), tr.cpu().numpy(), d_arena.cpu().numpy(), d_tab.cpu().numpy(),
                d_words.cpu().numpy(), d_desc.cpu().numpy().view(DESC))

    runs = []
    for dev in (True, False):
        d_tab, d_words = _up(torch, tab), torch.from_numpy(words.view(np.int32).copy()).cuda()
        runs.append((inbound(d_tab, d_words, dev), d_tab, d_words))
    (g, g_tab, g_words), (w, _, _) = runs
    for name, a, b in zip(("status", "trailer", "arena", "windows", "bitmaps", "desc"), g, w):
        assert np.array_equal(a, b), name
    st, tr, out = g[0], g[1], g[2]
    assert not st[real].any() and np.array_equal(st[src < 0], h_cst[src < 0])
    assert (tr[real] < 0).all() and not tr[src < 0].any()             # TR_VALID is the sign bit
    lasts = g[3].view(REPLAY_DTYPE)["last"]
    assert lasts[sids[1]] == (3 << 32) | max(s for s, k in zip(seqs, sa_idx) if k == 1)
    assert lasts[sids[0]] == max(s for s, k in zip(seqs, sa_idx) if k == 0)
    for j in real:
        i, k = src[j], int(sa_idx[src[j]])
        o, ro, ln = int(h_desc["off4"][j]) * 4, int(rdesc["off4"][i]) * 4, int(rdesc["len"][i])
        a, b = sas[k].hlen, ln - sas[k].mlen
        assert np.array_equal(out[o + a:o + b], want[ro + a:ro + b]), (j, i)
        assert g[5]["esn_hi"][j] == his[i]
    # the first batch again, the windows where that run left them
    st2 = inbound(g_tab, g_words, True)[0]
    assert (st2[real] == EACCES).all() and np.array_equal(st2[src < 0], h_cst[src < 0])
    for s in sids:
        drv.freesession(s)
