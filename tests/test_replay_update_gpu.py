"""espgpu_replay_update_batch (replay.hip): esp_input_cb's window update for a
device-resident batch.  The device result is compared with the host
espgpu_replay_update64 (pinned against the oracle in test_replay_update64.py)
applied to each SA's taking-part records one after another in index order:
d_ustatus for every record, `last` and every bitmap word for every SA, guard
words between and around the windows, and d_desc / d_status unmodified."""
import ctypes as C

import numpy as np
import pytest

import oracle as O
from helpers import GcmSA, build_records, oracle_decrypt
from test_replay_update64 import _seqs, _windows

EACCES, EINVAL = 13, 22
GUARD = 0xDEADBEEF
SCAN_BLOCK = 1024          # grouped positions per workgroup of the max-scan (kReplayScanBlock)
SORT_TILE = 2048           # records per workgroup of a radix pass (sa_group.h kSortTile)
DESC = np.dtype([("off4", "<u4"), ("len", "<u2"), ("sa", "<u2"), ("esn_hi", "<u4"), ("salt", "<u4")])


def _torch():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.fail("GPU test run without a visible HIP device")
    return torch


@pytest.fixture(scope="module")
def drv():
    _torch()
    from espgpu.opencrypto import GpuCryptoDriver
    # only the device-resident batch entries are used here: one small staging slot
    d = GpuCryptoDriver(max_sessions=64, batch_records=1024, batch_bytes=1 << 20, nbatches=1)
    yield d
    d.close()
    import gc
    gc.collect()           # the batches' arrays and device tensors go now, not during a later module


def _tables(wins, gap=2):
    """wins: (last, wsize, bitmap words, flags, initial words or None).  The
    windows lie `gap` guard words apart in one bitmap array."""
    from espgpu.batch import REPLAY_DTYPE
    tab = np.zeros(len(wins), dtype=REPLAY_DTYPE)
    words, off = [np.full(gap, GUARD, dtype=np.uint32)], gap
    for k, (last, wsize, nb, flags, init) in enumerate(wins):
        tab[k] = (last, wsize, nb, off, flags)
        words.append(np.zeros(nb, dtype=np.uint32) if init is None else init.astype(np.uint32))
        words.append(np.full(gap, GUARD, dtype=np.uint32))
        off += nb + gap
    return tab, np.concatenate(words)


def _records(sa, seq, length=None):
    """16-byte records carrying seq big-endian at byte 4, and their descriptors."""
    n = len(sa)
    rng = np.random.default_rng(n + 1)
    arena = rng.integers(0, 256, n * 16 + 64, dtype=np.uint8)
    seq = np.asarray(seq, dtype=np.uint64)
    for k in range(4):
        arena[np.arange(n) * 16 + 4 + k] = ((seq >> np.uint64(24 - 8 * k)) & np.uint64(0xFF)).astype(np.uint8)
    desc = np.zeros(n, dtype=DESC)
    desc["off4"] = np.arange(n) * 4
    desc["len"] = 16 if length is None else length
    desc["sa"] = sa
    desc["esn_hi"] = (seq >> np.uint64(32)).astype(np.uint32)
    return arena, desc


def _host_run(tab, words, desc, seq32, status):
    """The sequential definition: espgpu_replay_update64 per taking-part
    record in index order.  Returns (ustatus, tab, words) after the batch."""
    import espgpu
    from espgpu._lib import Replay
    L = espgpu.lib()
    tab, words = tab.copy(), words.copy()
    rps = [Replay(int(t["last"]), int(t["wsize"]), int(t["bitmap_size"]), int(t["bitmap_off"]), int(t["flags"]))
           for t in tab]
    wp = words.ctypes.data_as(C.POINTER(C.c_uint32))
    ust = np.zeros(len(desc), dtype=np.uint8)
    sa, ln, hi = desc["sa"], desc["len"], desc["esn_hi"]
    for i in np.flatnonzero((status == 0) & (sa < len(tab)) & (ln >= 8)):
        rp = rps[sa[i]]
        if rp.wsize == 0:
            continue
        s64 = (int(hi[i]) << 32) | int(seq32[i])
        ust[i] = L.espgpu_replay_update64(C.byref(rp), wp, s64)
    for k, rp in enumerate(rps):
        tab["last"][k] = rp.last
    return ust, tab, words


def _device_run(drv, tab, words, arena, desc, status, calls=None, stream=None):
    """Upload, run replay_update (once, or per (start, count) or (start,
    count, nreplay) slice of `calls` back to back without a sync; nreplay
    passes only the table's first entries), download.  With `stream`, the
    calls go to that stream once it has waited for the uploads."""
    torch = _torch()
    from espgpu.batch import replay_update, REPLAY_DTYPE
    n = len(desc)
    d_arena = torch.from_numpy(arena).cuda()
    d_desc = torch.from_numpy(desc.view(np.uint8).copy()).cuda()
    d_status = torch.from_numpy(status.copy()).cuda()
    d_tab = torch.from_numpy(tab.view(np.uint8).copy()).cuda()
    d_words = torch.from_numpy(words.view(np.int32).copy()).cuda()
    d_ust = torch.full((max(n, 1),), 0x77, dtype=torch.uint8, device="cuda")
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
    for a, cnt, *nrp in (calls or [(0, n)]):
        rtab = d_tab[:nrp[0] * REPLAY_DTYPE.itemsize] if nrp else d_tab
        replay_update(drv, d_arena, d_desc[a * 16:], cnt, d_status[a:], rtab, d_words, d_ust[a:], stream=stream)
    if stream is not None:
        stream.synchronize()
    else:
        torch.cuda.synchronize()
    assert np.array_equal(d_desc.cpu().numpy(), desc.view(np.uint8)), "d_desc modified"
    assert np.array_equal(d_status.cpu().numpy(), status), "d_status modified"
    return (d_ust.cpu().numpy()[:n], d_tab.cpu().numpy().view(tab.dtype),
            d_words.cpu().numpy().view(np.uint32))


def _compare(got, want, n_guard_words=None):
    gu, gt, gw = got
    wu, wt, ww = want
    bad = np.flatnonzero(gu != wu)
    assert bad.size == 0, ("ustatus", bad[:8], gu[bad[:8]], wu[bad[:8]])
    assert np.array_equal(gt["last"], wt["last"]), np.flatnonzero(gt["last"] != wt["last"])[:8]
    assert np.array_equal(gt.view(np.uint8), wt.view(np.uint8))
    badw = np.flatnonzero(gw != ww)                    # window words and guards alike
    assert badw.size == 0, ("bitmap", badw[:8], gw[badw[:8]], ww[badw[:8]])
    if n_guard_words is not None:
        assert (gw == GUARD).sum() >= n_guard_words


def _grid_windows(rng):
    """The window grid, each window used before the batch, and a wsize 0 entry."""
    wins = []
    for wsize, flags, last in _windows():
        r = O.Replay(wsize, last=last, flags=flags)
        for sn in _seqs(rng, last, wsize * 8, 100):
            r.update(sn)
        wins.append((r.last, wsize, r.bitmap.size, flags, r.bitmap.copy()))
    wins.append((0, 0, 0, 0, None))
    return wins


@pytest.mark.gpu
def test_update_many_interleaved_sas(drv):
    torch = _torch()
    from espgpu.batch import replay_check
    rng = np.random.default_rng(23)
    wins = _grid_windows(rng)
    tab, words = _tables(wins)
    nw, n = len(wins), 40000
    sa = rng.integers(0, nw + 3, n).astype(np.uint16)          # some sa >= nreplay
    seq = np.zeros(n, dtype=np.uint32)
    for s in range(nw + 3):
        at = np.flatnonzero(sa == s)
        last, wsize = (wins[s][0], wins[s][1]) if s < nw else (1000, 8)
        seq[at] = _seqs(rng, last, max(wsize, 1) * 8, at.size)
    far = rng.integers(0, n // 2, 400)                         # repeats far apart in the batch
    sa[far + n // 2] = sa[far]
    seq[far + n // 2] = seq[far]
    length = np.where(rng.random(n) < 0.03, 4, 16).astype(np.uint16)   # some len < 8
    arena, desc = _records(sa, seq, length)
    desc["esn_hi"] = 0xA5A5A5A5
    # esn_hi (and len 0 for what the window refuses) from the pre-filter itself
    d_desc = torch.from_numpy(desc.view(np.uint8).copy()).cuda()
    rst = torch.zeros(n, dtype=torch.uint8, device="cuda")
    replay_check(drv, torch.from_numpy(arena).cuda(), d_desc, n,
                 torch.from_numpy(tab.view(np.uint8).copy()).cuda(),
                 torch.from_numpy(words.view(np.int32).copy()).cuda(), rst)
    torch.cuda.synchronize()
    desc = d_desc.cpu().numpy().view(DESC).copy()
    status = np.where(rng.random(n) < 0.1, 80, 0).astype(np.uint8)     # about 10 % did not authenticate
    want = _host_run(tab, words, desc, seq, status)
    got = _device_run(drv, tab, words, arena, desc, status)
    _compare(got, want, n_guard_words=2 * (nw + 1))
    took = (status == 0) & (desc["sa"] < nw) & (desc["len"] >= 8)
    assert (want[0][took] == 0).sum() > 300 and (want[0] == EACCES).sum() > 300
    assert (want[1]["last"] != tab["last"]).sum() > nw // 2


def _one_sa_batch():
    """One ESN window of 128 bytes; three scan blocks plus one record, all of
    one SA, so grouped position = index and the workgroup boundaries of the
    max-scan lie at multiples of SCAN_BLOCK."""
    rng = np.random.default_rng(3)
    n, w = 3 * SCAN_BLOCK + 1, 1024
    t0 = (5 << 32) | (0xFFFFFFFF - 1500)               # the top crosses 2^32 inside the batch
    s64 = t0 - 200 + np.arange(n, dtype=np.int64)
    for a in range(0, n, 1500):                        # a local shuffle wider than the window
        seg = s64[a:a + 1500]
        s64[a:a + 1500] = seg[rng.permutation(seg.size)]
    for src, dst in ((SCAN_BLOCK - 5, SCAN_BLOCK + 3), (2 * SCAN_BLOCK - 1, 2 * SCAN_BLOCK),
                     (2 * SCAN_BLOCK + 7, 2 * SCAN_BLOCK + 9), (3 * SCAN_BLOCK - 2, 3 * SCAN_BLOCK)):
        s64[dst] = s64[src]                            # exact repeats across and beside block boundaries
    r = O.Replay(128, last=t0, flags=O.REPLAY_ESN)
    for sn in (t0 & 0xFFFFFFFF) - rng.integers(0, w, 200):     # a used window, top where it was
        r.update(int(sn))
    assert r.last == t0
    wins = [(r.last, 128, r.bitmap.size, O.REPLAY_ESN, r.bitmap.copy())]
    return wins, s64.astype(np.uint64)


@pytest.mark.gpu
def test_update_one_sa_across_scan_blocks(drv):
    wins, s64 = _one_sa_batch()
    tab, words = _tables(wins)
    n = len(s64)
    arena, desc = _records(np.zeros(n, dtype=np.uint16), s64)
    status = np.zeros(n, dtype=np.uint8)
    seq32 = (s64 & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    want = _host_run(tab, words, desc, seq32, status)
    got = _device_run(drv, tab, words, arena, desc, status)
    _compare(got, want, n_guard_words=4)
    assert want[1]["last"][0] >> 32 == 6               # crossed 2^32
    below = np.flatnonzero(want[0] == EACCES)
    assert below.size > 50                             # fell below the moving bottom, or repeats
    for dst in (SCAN_BLOCK + 3, 2 * SCAN_BLOCK, 2 * SCAN_BLOCK + 9, 3 * SCAN_BLOCK):
        assert want[0][dst] == EACCES


def _small(drv, wins, sa, s64, status=None, calls=None, n_guard=None):
    tab, words = _tables(wins)
    s64 = np.asarray(s64, dtype=np.uint64)
    arena, desc = _records(np.asarray(sa, dtype=np.uint16), s64)
    status = np.zeros(len(sa), dtype=np.uint8) if status is None else np.asarray(status, dtype=np.uint8)
    want = _host_run(tab, words, desc, (s64 & np.uint64(0xFFFFFFFF)).astype(np.uint32), status)
    got = _device_run(drv, tab, words, arena, desc, status, calls=calls)
    _compare(got, want, n_guard_words=n_guard)
    return want, tab, words


@pytest.mark.gpu
def test_update_edges(drv):
    rng = np.random.default_rng(9)
    used = O.Replay(8, last=5000)
    for sn in range(4950, 5000, 3):
        used.update(sn)
    wins = [(used.last, 8, used.bitmap.size, 0, used.bitmap.copy()),
            (0, 4, 2, 0, None),
            ((1 << 32) | 77, 32, 16, O.REPLAY_ESN, None)]
    # n = 0: nothing happens
    want, tab, words = _small(drv, wins, [], [])
    assert np.array_equal(want[1], tab) and np.array_equal(want[2], words)
    # n = 1
    want, _, _ = _small(drv, wins, [0], [5001])
    assert want[0][0] == 0 and want[1]["last"][0] == 5001
    want, _, _ = _small(drv, wins, [0], [4950])
    assert want[0][0] == EACCES
    # every record refused before the update: the windows stay as they are
    sa = rng.integers(0, 3, 300)
    want, tab, words = _small(drv, wins, sa, 5000 + rng.integers(0, 50, 300), status=np.full(300, 80))
    assert not want[0].any() and np.array_equal(want[1], tab) and np.array_equal(want[2], words)
    # one record advances further than the ring, among records before and after it
    want, _, _ = _small(drv, wins, [0, 0, 0, 0, 1, 0], [5001, 4999, 5001 + 4 * 32 * 7 + 3, 5003, 9, 5001 + 4 * 32 * 7])
    assert list(want[0]) == [0, 0, 0, EACCES, 0, 0]
    # seq 0 on an empty window, then inside it once the top has moved
    want, _, _ = _small(drv, wins, [1, 1, 1, 1], [0, 3, 0, 0])
    assert list(want[0]) == [EACCES, 0, 0, EACCES]
    # a window without the redundant block: EINVAL for its records only
    bad = wins + [(100, 8, 2, 0, None), (100, 8, 3, 0, None)]
    want, tab, words = _small(drv, bad, [3, 0, 4, 3, 2], [101, 5002, 101, 90, (1 << 32) | 78])
    assert list(want[0]) == [EINVAL, 0, EINVAL, EINVAL, 0]
    assert want[1]["last"][3] == 100 and want[1]["last"][4] == 100


@pytest.mark.gpu
def test_update_two_calls_back_to_back(drv):
    """Two calls on one stream without a sync between them: the second sees
    the windows the first left, so the result is the sequential run over the
    concatenation."""
    rng = np.random.default_rng(41)
    wins = _grid_windows(rng)[::5]
    nw, n = len(wins), 6000
    sa = rng.integers(0, nw, n)
    s64 = np.zeros(n, dtype=np.uint64)
    for s in range(nw):
        at = np.flatnonzero(sa == s)
        last, wsize, flags = wins[s][0], wins[s][1], wins[s][3]
        lo = np.array(_seqs(rng, last, max(wsize, 1) * 8, at.size), dtype=np.uint64)
        s64[at] = lo | (np.uint64(last >> 32 << 32) if flags & O.REPLAY_ESN else np.uint64(0))
    cut = 2500
    _small(drv, wins, sa, s64, calls=[(0, cut), (cut, n - cut)], n_guard=2 * (nw + 1))


@pytest.mark.gpu
def test_check_decrypt_update_merge(drv):
    """The whole inbound sequence on GCM records: pre-filter, verify + decrypt,
    window update, merge.  One record is in the batch twice: both copies pass
    the pre-filter and authenticate, and the update refuses exactly the later
    one.  A second batch replaying the first is refused entirely by the
    pre-filter, from the windows left in device memory."""
    torch = _torch()
    from espgpu.batch import (decrypt_batch, descs_to_tensor, replay_check, replay_merge, replay_update,
                              REPLAY_DTYPE)
    rng = np.random.default_rng(17)
    sas = [GcmSA(rng, esn=True), GcmSA(rng)]
    sids = []
    for s in sas:
        rc, sid = drv.newsession(s.esp_sa().csp())
        assert rc == 0
        sids.append(sid)
    start = {0: ((4 << 32) | 0xFFFFFFF0, O.REPLAY_ESN), 1: (5000, 0)}
    n = 200
    sa_idx = rng.integers(0, 2, n)
    sa_idx[[10, 150]] = 0
    seqs, his = [], []
    for i, s in enumerate(sa_idx):                     # fresh, ascending: all pass the check
        seqs.append((0xFFFFFFF0 + 1 + i) & 0xFFFFFFFF if s == 0 else 5001 + i)
        his.append((4 if 0xFFFFFFF0 + 1 + i < 2**32 else 5) if s == 0 else 0)
    seqs[150], his[150] = seqs[10], his[10]            # record 10 again, 140 records later
    plain, ct, descs, esn_hi = build_records(rng, sas, sa_idx, [96] * n, seqs=seqs,
                                             esn_hi=np.array(his, dtype=np.uint32))
    o10, o150, L = int(descs["off4"][10]) * 4, int(descs["off4"][150]) * 4, int(descs["len"][10])
    ct[o150:o150 + L] = ct[o10:o10 + L]                # the same bytes on the wire
    want, wst = oracle_decrypt(sas, ct, descs, esn_hi)
    assert not wst.any()
    descs["sa"] = [sids[s] for s in sa_idx]
    descs["esn_hi"] = 0                                # only the window knows it
    wins = [(0, 0, 0, 0, None)] * (max(sids) + 1)      # indexed by session id
    for k in (0, 1):
        wins[sids[k]] = (start[k][0], 32, 16, start[k][1], None)   # 256 packets: the whole batch stays inside
    tab, words = _tables(wins)
    d_tab = torch.from_numpy(tab.view(np.uint8).copy()).cuda()
    d_words = torch.from_numpy(words.view(np.int32).copy()).cuda()

    def inbound():
        d_arena = torch.from_numpy(ct.copy()).cuda()
        d_desc = descs_to_tensor(descs, "cuda")
        rst = torch.zeros(n, dtype=torch.uint8, device="cuda")
        ust = torch.zeros(n, dtype=torch.uint8, device="cuda")
        st = torch.zeros(n, dtype=torch.uint8, device="cuda")
        out = torch.zeros_like(d_arena)
        replay_check(drv, d_arena, d_desc, n, d_tab, d_words, rst)
        decrypt_batch(drv, d_arena, d_desc, n, st, out=out)
        replay_update(drv, d_arena, d_desc, n, st, d_tab, d_words, ust)
        replay_merge(drv, st, rst, n)
        replay_merge(drv, st, ust, n)
        torch.cuda.synchronize()
        return st.cpu().numpy(), rst.cpu().numpy(), out.cpu().numpy()

    st, rst, out = inbound()
    assert not rst.any()
    assert st[150] == EACCES and (np.delete(st, 150) == 0).all()
    for i in range(n):
        if i != 150:
            o = int(descs["off4"][i]) * 4
            assert np.array_equal(out[o + 16:o + L - 16], want[o + 16:o + L - 16]), i
    lasts = d_tab.cpu().numpy().view(REPLAY_DTYPE)["last"]
    assert lasts[sids[0]] == max((h << 32) | s for h, s, k in zip(his, seqs, sa_idx) if k == 0)
    assert lasts[sids[1]] == max(s for s, k in zip(seqs, sa_idx) if k == 1)
    # the same batch again: the windows in device memory refuse all of it
    st, rst, _ = inbound()
    assert (rst == EACCES).all() and (st == EACCES).all()
    for s in sids:
        drv.freesession(s)
