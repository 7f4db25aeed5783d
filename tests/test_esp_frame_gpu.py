"""espgpu_esp_frame_batch (frame.hip): esp_output's framing for a
device-resident batch.  Every test compares the device batch with the host
rule espgpu_esp_frame (pinned against esp.py's restatement of esp_output in
test_esp_frame.py) applied in index order: the whole arena with random guard
bytes between the records, d_desc, d_fstatus, and every outsa entry with
guard entries past nout."""
import numpy as np
import pytest

import oracle as O
from ah_helpers import AhSA
from frame_helpers import EINVAL, host_frame_batch, layout, record_len, sa_kinds
from helpers import EtaSA, GcmSA

SORT_TILE = 2048           # records per workgroup of a radix pass (sa_group.h kSortTile)
NSES = 1100                # sessions of the module's driver
DIGEST_SID, FREED_SID = 38, 39
M64 = 2**64 - 1


def _torch():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.fail("GPU test run without a visible HIP device")
    return torch


class Env:
    """A driver whose sessions 0 .. NSES - 1 cycle through every ESP kind,
    except DIGEST_SID (an AH session) and FREED_SID (freed again)."""

    def __init__(self, nses):
        from espgpu.opencrypto import GpuCryptoDriver
        rng = np.random.default_rng(11)
        self.drv = GpuCryptoDriver(max_sessions=nses + 4, batch_records=1024, batch_bytes=1 << 20, nbatches=1)
        kinds = sa_kinds(rng)
        cheap = [EtaSA(rng, ctr=True, noauth=True), EtaSA(rng, null=True), EtaSA(rng, noauth=True),
                 EtaSA(rng, ctr=True, sha=256)]
        self.sas, self.kflags = [], []
        for k in range(nses):
            if k == DIGEST_SID:
                sa, kf = AhSA(rng, 256), 0
                csp = sa.csp()
            else:
                # the first 38 take every kind in turn; the many behind them are cheap to set up
                _, sa, kf = kinds[k % len(kinds)] if k < 48 else (None, cheap[k % len(cheap)], 0)
                csp = sa.esp_sa().csp()
            rc, sid = self.drv.newsession(csp)
            assert rc == 0 and sid == k, (rc, sid, k)
            self.sas.append(sa)
            self.kflags.append(kf)
        self.drv.freesession(FREED_SID)

    def shapes(self, flags):
        """The shape of every session under flags[sa] (None: no ESP session)."""
        from espgpu import esp as E
        out = []
        for k, sa in enumerate(self.sas):
            f = int(flags[k]) if k < len(flags) else 0
            out.append(None if k in (DIGEST_SID, FREED_SID) else E.esp_frame_shape(sa.esp_sa(), f))
        return out

    def outsa(self, rng, nout, count0=None, flags=None):
        """nout entries with random counters, flags and salts, the session
        kind's own flag (CTRCOMPAT) where it has one."""
        from espgpu import _lib as L
        from espgpu.batch import OUTSA_DTYPE
        t = np.zeros(nout, dtype=OUTSA_DTYPE)
        t["count"] = rng.integers(0, 2**31, nout) if count0 is None else count0
        t["cntr"] = rng.integers(0, 2**62, nout)
        t["spi"] = rng.integers(256, 2**32, nout)
        t["salt"] = rng.integers(0, 2**32, nout)
        pads = np.array([0, L.OUT_PAD_SEQ, L.OUT_PAD_ZERO, L.OUT_PAD_RAND])
        t["flags"] = (pads[rng.integers(0, 4, nout)] | rng.choice([0, L.OUT_ESN], nout)) if flags is None else flags
        k = min(nout, len(self.kflags))
        t["flags"][:k] |= np.array(self.kflags[:k], dtype=np.uint32)
        t["pad_"] = 0x0badf00d
        return t


@pytest.fixture(scope="module")
def env():
    _torch()
    e = Env(NSES)
    yield e
    e.drv.close()
    import gc
    gc.collect()


def _frame_words(rng, rlen):
    return (np.asarray(rlen, dtype=np.int64) | (rng.integers(0, 256, len(rlen)) << 16) |
            (rng.integers(0, 256, len(rlen)) << 24)).astype(np.uint32)     # bits 24-31 are ignored


def _run_and_compare(drv, shapes, arena, desc, frame, outsa, calls=None, stream=None, between=None):
    """Upload, esp_frame (once, or per (start, count, nout) slice of `calls`
    back to back without a sync, between(k) called after the k-th), download, and compare everything with the
    host rule applied to the same calls.  The outsa tensor has three guard
    entries past its end.  Returns the device (arena, desc, fstatus, outsa)."""
    torch = _torch()
    from espgpu.batch import OUTSA_DTYPE, esp_frame
    n, nout = len(desc), len(outsa)
    calls = calls or [(0, n, nout)]
    guard = np.zeros(3, dtype=OUTSA_DTYPE)
    guard.view(np.uint8)[:] = 0xC3
    d_arena = torch.from_numpy(arena).cuda()
    d_desc = torch.from_numpy(desc.view(np.uint8).copy()).cuda()
    d_frame = torch.from_numpy(frame.view(np.int32).copy()).cuda()
    d_out = torch.from_numpy(np.concatenate([outsa, guard]).view(np.uint8).copy()).cuda()
    d_fst = torch.full((n + 8,), 0x77, dtype=torch.uint8, device="cuda")
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
    for k, (a, cnt, no) in enumerate(calls):
        esp_frame(drv, d_arena, d_desc[a * 16:], d_frame[a:], cnt, d_out[:no * OUTSA_DTYPE.itemsize], d_fst[a:],
                  stream=stream)
        if between is not None:
            between(k)
    if stream is not None:
        stream.synchronize()
    else:
        torch.cuda.synchronize()
    w_arena, w_desc, w_out = arena, desc.copy(), outsa.copy()
    w_fst = np.full(n, 0x77, dtype=np.uint8)
    for a, cnt, no in calls:
        w_arena, w_desc[a:a + cnt], w_fst[a:a + cnt], w_out[:no] = host_frame_batch(
            w_arena, w_desc[a:a + cnt], frame[a:a + cnt], w_out[:no], shapes)
    g_arena, g_desc = d_arena.cpu().numpy(), d_desc.cpu().numpy().view(desc.dtype)
    g_fst, g_out = d_fst.cpu().numpy(), d_out.cpu().numpy().view(OUTSA_DTYPE)
    bad = np.flatnonzero(g_fst[:n] != w_fst)
    assert bad.size == 0, ("fstatus", bad[:8], g_fst[bad[:8]], w_fst[bad[:8]], desc["sa"][bad[:8]])
    assert (g_fst[n:] == 0x77).all()
    for fld in ("off4", "len", "sa", "esn_hi", "salt"):
        bad = np.flatnonzero(g_desc[fld] != w_desc[fld])
        assert bad.size == 0, ("desc." + fld, bad[:8], g_desc[fld][bad[:8]], w_desc[fld][bad[:8]])
    for fld in ("count", "cntr", "spi", "salt", "flags", "pad_"):
        bad = np.flatnonzero(g_out[fld][:nout] != w_out[fld])
        assert bad.size == 0, ("outsa." + fld, bad[:8], g_out[fld][bad[:8]], w_out[fld][bad[:8]])
    assert np.array_equal(g_out[nout:].view(np.uint8), guard.view(np.uint8)), "outsa guard entries written"
    bad = np.flatnonzero(g_arena != w_arena)
    assert bad.size == 0, ("arena", bad[:16], g_arena[bad[:16]], w_arena[bad[:16]])
    return g_arena, g_desc, g_fst[:n], g_out[:nout]


def _batch(env, rng, sa, nout, rlen_max=96, outsa=None, wrong_len=0.0, calls=None, stream=None, rlen=None,
           between=None):
    """Records of the sessions sa[i] with random payload lengths against a
    random (or the given) outsa table: frame on the device, compare."""
    sa = np.asarray(sa, dtype=np.int64)
    outsa = env.outsa(rng, nout) if outsa is None else outsa
    shapes = env.shapes(outsa["flags"])
    rlen = rng.integers(0, rlen_max + 1, len(sa)) if rlen is None else rlen
    arena, desc = layout(rng, shapes, sa, rlen)
    if wrong_len:
        bad = rng.random(len(sa)) < wrong_len
        desc["len"][bad] += rng.choice([-4, 4, 1, 16], int(bad.sum())).astype(np.uint16)
    got = _run_and_compare(env.drv, shapes, arena, desc, _frame_words(rng, rlen), outsa, calls=calls, stream=stream,
                           between=between)
    return got, desc, outsa


@pytest.mark.gpu
def test_mixed_batch(env):
    """40 interleaved SAs of every kind, rlen 0 .. 1460, with records that
    take no part: sa >= nout, a freed session, a DIGEST session, a wrong len."""
    rng = np.random.default_rng(1)
    n, nout = 6000, 40
    sa = rng.integers(0, nout + 3, n)                 # 40 .. 42: sessions exist, but sa >= nout
    (_, g_desc, g_fst, g_out), desc, outsa = _batch(env, rng, sa, nout, rlen_max=1460, wrong_len=0.05)
    for s in (DIGEST_SID, FREED_SID, 40, 41, 42):
        assert (sa == s).sum() > 50 and (g_fst[sa == s] == EINVAL).all() and (g_desc["len"][sa == s] == 0).all()
    ok = g_fst == 0
    assert 4500 < ok.sum() < n
    # refused records consume no numbers
    for s in range(nout):
        assert int(g_out["count"][s]) == int(outsa["count"][s]) + int((ok & (sa == s)).sum())
    assert g_out["count"][DIGEST_SID] == outsa["count"][DIGEST_SID]


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 2047, 2048, 2049, 4096])
def test_tile_wave_and_workgroup_edges(env, n):
    rng = np.random.default_rng(n)
    _batch(env, rng, rng.integers(0, 12, n), 12, wrong_len=0.05)


@pytest.mark.gpu
@pytest.mark.parametrize("nout", [255, 256, 257, 65536])
def test_radix_passes_and_the_sentinel_key(env, nout):
    """One, two and three 8-bit passes; the key of a record that takes no part
    is nout (65536 for the largest table, above every 16-bit sa)."""
    rng = np.random.default_rng(nout)
    n = 3000
    sa = rng.integers(0, min(nout, NSES) + 2, n)
    sa[rng.random(n) < 0.1] = nout - 1
    if nout > NSES:
        sa[rng.random(n) < 0.1] = rng.integers(NSES + 4, nout)     # below nout, but no session behind it
    (_, _, g_fst, _), _, _ = _batch(env, rng, sa, nout, wrong_len=0.03)
    assert (g_fst[sa >= min(nout, NSES)] == EINVAL).all()
    assert (g_fst[sa < DIGEST_SID] == 0).sum() > 0 and (g_fst[(sa > 200) & (sa < min(nout, NSES))] == 0).sum() > 0


@pytest.mark.gpu
def test_a_segment_that_crosses_tiles(env):
    """One SA with 3500 records between 39 short ones."""
    rng = np.random.default_rng(3)
    sa = np.r_[np.full(3500, 17), rng.integers(0, 17, 300), rng.integers(18, 38, 300)]
    rng.shuffle(sa)
    (_, _, g_fst, g_out), _, outsa = _batch(env, rng, sa, 40)
    assert (g_fst == 0).all() and int(g_out["count"][17]) == int(outsa["count"][17]) + 3500


@pytest.mark.gpu
def test_nearly_every_position_a_segment_head(env):
    """1024 SAs with 1 to 3 records each."""
    rng = np.random.default_rng(4)
    ids = np.array([k for k in range(1030) if k not in (DIGEST_SID, FREED_SID)][:1024])
    sa = np.repeat(ids, rng.integers(1, 4, 1024))
    rng.shuffle(sa)
    (_, _, g_fst, _), _, _ = _batch(env, rng, sa, 1030)
    assert (g_fst == 0).all()


@pytest.mark.gpu
def test_counter_edges_inside_one_batch(env):
    """The counter edges of test_esp_frame.py on the device.  SA 0's WRAPCHECK
    limit falls in the middle of its segment, which spans a tile boundary."""
    from espgpu import _lib as L
    rng = np.random.default_rng(5)
    nout = 12
    W, E_, C_ = L.OUT_WRAPCHECK, L.OUT_ESN, L.OUT_CYCSEQ
    edges = {0: (2**32 - 1 - 1500, W | L.OUT_PAD_SEQ),        # refused from rank 1500 on, of 3000
             1: (2**32 - 3, E_),                               # the high word changes inside the run
             2: (2**32 - 3, 0),                                # the low word wraps, as in the reference
             3: (2**32 - 3, W),                                # two accepted, then EINVAL
             4: (2**32 - 3, W | C_),                           # never refused
             5: (M64 - 2, W | E_),                             # the top of the ESN space
             6: (M64 - 2, W | E_ | C_),
             8: (2**32 - 3, W | E_),                           # ESN passes the 32-bit limit
             9: (5 * 2**32 - 2, W),                            # wrapped before: the next low-word limit
             10: (2**32 - 1, W),                               # at the limit already: nothing accepted
             11: (M64 - 1, E_)}                                # count++ wraps the 64-bit counter
    outsa = env.outsa(rng, nout)
    for k, (c0, f) in edges.items():
        outsa["count"][k] = np.uint64(c0)
        outsa["flags"][k] = f | env.kflags[k]
    sa = np.r_[np.full(3000, 0), np.repeat(np.arange(1, nout), 9)]
    rng.shuffle(sa)
    assert SORT_TILE < 3000 and 1500 < SORT_TILE           # SA 0's segment: grouped positions 0 .. 2999
    (_, g_desc, g_fst, g_out), _, _ = _batch(env, rng, sa, nout, outsa=outsa)
    st0 = g_fst[sa == 0]
    assert (st0[:1500] == 0).all() and (st0[1500:] == EINVAL).all() and int(g_out["count"][0]) == 2**32 - 1
    assert list(g_fst[sa == 3]) == [0, 0] + [EINVAL] * 7 and int(g_out["count"][3]) == 2**32 - 1
    assert list(g_desc["esn_hi"][sa == 1]) == [0, 0] + [1] * 7
    assert (g_fst[sa == 4] == 0).all() and (g_fst[sa == 6] == 0).all() and (g_fst[sa == 8] == 0).all()
    assert list(g_fst[sa == 5]) == [0, 0] + [EINVAL] * 7 and int(g_out["count"][5]) == M64
    assert (g_fst[sa == 10] == EINVAL).all() and int(g_out["cntr"][10]) == int(outsa["cntr"][10])
    assert int(g_out["count"][2]) == 2**32 + 6 and int(g_out["count"][11]) == 7


@pytest.mark.gpu
def test_two_calls_without_a_sync_then_growth():
    """The second call continues the first's counters; then n and nout grow
    (the workspace with them).  Once on the default stream, once on a
    caller's stream."""
    torch = _torch()
    e = Env(48)
    try:
        for stream in (None, torch.cuda.Stream()):
            rng = np.random.default_rng(6)
            sa = np.r_[rng.integers(0, 20, 1000), rng.integers(0, 47, 3000)]
            calls = [(0, 500, 20), (500, 500, 20), (1000, 3000, 47)]
            (_, _, g_fst, g_out), _, outsa = _batch(e, rng, sa, 47, calls=calls, stream=stream, wrong_len=0.03)
            for s in range(20):
                assert int(g_out["count"][s]) == int(outsa["count"][s]) + int(((g_fst == 0) & (sa == s)).sum())
    finally:
        e.drv.close()


@pytest.mark.gpu
def test_window_update_grows_the_workspace_a_framing_call_sized():
    """Both stages carve one per-ctx workspace, sized in bytes by whoever asks.
    On a fresh driver and one stream, with no sync in between: a framing call
    of one record past a sort tile over 3 SAs allocates the (smaller) framing
    layout, a window update of as many records over 257 windows (two radix
    passes) has to grow it while the framing may still run, and a framing call
    of 64 records is then carved from the larger buffer.  All three against
    the host rules."""
    torch = _torch()
    from espgpu.batch import replay_update
    from test_replay_update_gpu import _compare, _host_run, _records, _tables
    rng = np.random.default_rng(9)
    n, nwin = SORT_TILE + 1, 257
    wins = [(1000 + 3 * k, 8, O.Replay(8).bitmap.size, O.REPLAY_ESN if k % 2 else 0, None) for k in range(nwin)]
    tab, words = _tables(wins)
    usa = rng.integers(0, nwin, n).astype(np.uint16)
    useq = (1000 + 3 * usa.astype(np.int64) + rng.integers(-80, 40, n)).astype(np.uint32)
    uarena, udesc = _records(usa, useq)
    ustatus = np.where(rng.random(n) < 0.1, 80, 0).astype(np.uint8)
    want = _host_run(tab, words, udesc, useq, ustatus)
    assert (want[0] == 0).sum() > 200 and (want[0] != 0).sum() > 200
    d_upd = [torch.from_numpy(x).cuda() for x in (uarena, udesc.view(np.uint8).copy(), ustatus, tab.view(np.uint8).copy(),
                                                  words.view(np.int32).copy())]
    d_ust = torch.full((n,), 0x77, dtype=torch.uint8, device="cuda")
    e = Env(48)
    try:
        def update_after_the_first(k):
            if k == 0:
                replay_update(e.drv, d_upd[0], d_upd[1], n, d_upd[2], d_upd[3], d_upd[4], d_ust)
        sa = rng.integers(0, 3, n + 64)
        (_, _, g_fst, _), _, _ = _batch(e, rng, sa, 3, calls=[(0, n, 3), (n, 64, 3)], between=update_after_the_first)
        assert (g_fst == 0).all()
        _compare((d_ust.cpu().numpy(), d_upd[3].cpu().numpy().view(tab.dtype), d_upd[4].cpu().numpy().view(np.uint32)),
                 want, n_guard_words=2 * (nwin + 1))
    finally:
        e.drv.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["gcm", "cbc-sha1"])
def test_frame_encrypt_merge_then_inbound(kind):
    """esp_frame -> encrypt_batch -> replay_merge equals the oracle's
    encryption of the host-framed records; then the inbound sequence accepts
    every record, with the pad length in the trailer word and each window's
    `last` at its SA's count."""
    torch = _torch()
    from espgpu import _lib as L
    from espgpu import esp as E
    from espgpu.batch import (OUTSA_DTYPE, REPLAY_DTYPE, decrypt_batch, encrypt_batch, esp_frame, replay_check,
                              replay_merge, replay_update)
    from espgpu.opencrypto import GpuCryptoDriver
    rng = np.random.default_rng(8)
    nsa = 6
    sas = [GcmSA(rng, 16 if k % 2 else 32, esn=k % 3 == 0) if kind == "gcm" else EtaSA(rng, esn=k % 3 == 0)
           for k in range(nsa)]
    drv = GpuCryptoDriver(max_sessions=16, batch_records=1024, batch_bytes=1 << 20, nbatches=1)
    try:
        for k, s in enumerate(sas):
            rc, sid = drv.newsession(s.esp_sa().csp())
            assert rc == 0 and sid == k
        outsa = np.zeros(nsa, dtype=OUTSA_DTYPE)
        for k, s in enumerate(sas):
            f = L.OUT_PAD_SEQ | (L.OUT_ESN if s.esn else 0)
            outsa[k] = (10 + k, 1000 * k, s.spi, int.from_bytes(s.salt, "little"), f, 0)
        outsa["count"][5] = 2**32 - 1 - 40               # non-ESN (5 % 3 != 0): WRAPCHECK refuses its tail
        outsa["flags"][5] |= L.OUT_WRAPCHECK
        shapes = [E.esp_frame_shape(s.esp_sa(), int(outsa["flags"][k])) for k, s in enumerate(sas)]
        n = 700
        sa = rng.integers(0, nsa + 1, n)                 # sa == nsa: takes no part
        rlen = rng.integers(0, 1400, n)
        arena, desc = layout(rng, shapes, sa, rlen)
        nh = rng.integers(0, 59, n)
        frame = (rlen | (nh << 16)).astype(np.uint32)
        h_arena, h_desc, h_fst, h_out = host_frame_batch(arena, desc, frame, outsa, shapes)
        acc = h_fst == 0
        assert (h_fst[sa == nsa] == EINVAL).all() and 40 < (~acc & (sa == 5)).sum() and acc.sum() > 500
        want = h_arena.copy()
        O.batch([s.oracle for s in sas], want, h_desc["off4"][acc], h_desc["len"][acc], h_desc["sa"][acc],
                esn_hi=h_desc["esn_hi"][acc].copy(), nthreads=4, encrypt=True)

        d_arena = torch.from_numpy(arena).cuda()
        d_desc = torch.from_numpy(desc.view(np.uint8).copy()).cuda()
        d_out = torch.from_numpy(outsa.view(np.uint8).copy()).cuda()
        d_fst = torch.zeros(n, dtype=torch.uint8, device="cuda")
        d_st = torch.full((n,), 0x55, dtype=torch.uint8, device="cuda")
        esp_frame(drv, d_arena, d_desc, torch.from_numpy(frame.view(np.int32).copy()).cuda(), n, d_out, d_fst)
        encrypt_batch(drv, d_arena, d_desc, n, d_st)
        replay_merge(drv, d_st, d_fst, n)
        torch.cuda.synchronize()
        st = d_st.cpu().numpy()
        assert (st[acc] == 0).all() and (st[~acc] == EINVAL).all()
        g = d_arena.cpu().numpy()
        bad = np.flatnonzero(g != want)                  # refused records included: still plaintext
        assert bad.size == 0, (bad[:16], g[bad[:16]], want[bad[:16]])
        g_out = d_out.cpu().numpy().view(OUTSA_DTYPE)
        assert np.array_equal(g_out.view(np.uint8), h_out.view(np.uint8))

        # the peer: windows at the counters the batch started from
        tab = np.zeros(nsa, dtype=REPLAY_DTYPE)
        for k in range(nsa):
            rf = (L.REPLAY_ESN if sas[k].esn else 0)
            tab[k] = (outsa["count"][k], 16, 8, 8 * k, rf)
        d_tab = torch.from_numpy(tab.view(np.uint8).copy()).cuda()
        d_words = torch.zeros(8 * nsa, dtype=torch.int32, device="cuda")
        d_rst = torch.zeros(n, dtype=torch.uint8, device="cuda")
        d_ust = torch.zeros(n, dtype=torch.uint8, device="cuda")
        d_st2 = torch.full((n,), 0x55, dtype=torch.uint8, device="cuda")
        d_tr = torch.zeros(n, dtype=torch.int32, device="cuda")
        d_pt = torch.zeros_like(d_arena)
        replay_check(drv, d_arena, d_desc, n, d_tab, d_words, d_rst)
        decrypt_batch(drv, d_arena, d_desc, n, d_st2, out=d_pt, trailer=d_tr)
        replay_update(drv, d_arena, d_desc, n, d_st2, d_tab, d_words, d_ust)
        replay_merge(drv, d_st2, d_rst, n)
        replay_merge(drv, d_st2, d_ust, n)
        torch.cuda.synchronize()
        st2, tr, pt = d_st2.cpu().numpy(), d_tr.cpu().numpy().view(np.uint32), d_pt.cpu().numpy()
        assert (st2[acc] == 0).all(), np.flatnonzero(acc & (st2 != 0))[:8]
        assert (st2[~acc] != 0).all()
        for i in np.flatnonzero(acc):
            sh = shapes[sa[i]]
            padlen = record_len(sh, int(rlen[i])) - 8 - sh.ivlen - sh.alen - int(rlen[i]) - 2
            assert int(tr[i]) == (int(nh[i]) | (padlen << 8) | L.TR_VALID), (i, hex(int(tr[i])))
            o = int(desc["off4"][i]) * 4 + 8 + sh.ivlen
            assert np.array_equal(pt[o:o + int(rlen[i])], arena[o:o + int(rlen[i])])
        last = d_tab.cpu().numpy().view(REPLAY_DTYPE)["last"]
        assert np.array_equal(last, g_out["count"]), (last, g_out["count"])
    finally:
        drv.close()
