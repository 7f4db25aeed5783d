"""espgpu_esp_decap_batch (decap.hip): esp_input_cb's tail and
ipsec4/6_common_input_cb for a device-resident batch.  Every test compares the
device batch with the host rule espgpu_esp_decap (pinned against esp.py's
restatement of the reference in test_esp_decap.py) applied in index order: all
of d_ipkt and d_dstatus with guard entries past n, the whole of d_out with the
random bytes between the packets, every espgpu_insa and the guard entries
after it, d_arena unchanged when out of place, and d_pkt, d_desc, d_trailer
and d_status unchanged."""
import numpy as np
import pytest

from ah_helpers import AhSA
from classify_helpers import ipv4, ipv6
from decap_helpers import EINVAL, ENODATA, EPFNOSUPPORT, host_decap_batch, layout, packet, trailer_of
from frame_helpers import record_len, sa_kinds
from helpers import DESC, EtaSA, GcmSA

EACCES, EBADMSG, ENOTSUP = 13, 74, 95
GUARD = 5
NSES = 1064                 # sessions of the module's driver
DIGEST_SID, FREED_SID = 21, 22
NMIX = 40                   # the SAs of the mixed batches: every kind, mode and family


def _torch():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.fail("GPU test run without a visible HIP device")
    return torch


def _up(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()


class Env:
    """A driver whose sessions 0 .. NSES - 1 cycle through every ESP kind,
    except DIGEST_SID (an AH session) and FREED_SID (freed again); shapes[sa]
    is (ivlen, alen), None for those two."""

    def __init__(self, nses):
        from espgpu import esp as E
        from espgpu.opencrypto import GpuCryptoDriver
        rng = np.random.default_rng(31)
        self.drv = GpuCryptoDriver(max_sessions=nses + 4, batch_records=1024, batch_bytes=1 << 20, nbatches=1)
        kinds = [sa for _, sa, _ in sa_kinds(rng)] + [GcmSA(rng, mlen=12), GcmSA(rng, mlen=8), EtaSA(rng, sha=384),
                                                      EtaSA(rng, sha=512), EtaSA(rng, null=True, sha=512)]
        cheap = [EtaSA(rng, ctr=True, noauth=True), EtaSA(rng, null=True), EtaSA(rng, noauth=True)]
        self.shapes = []
        for k in range(nses):
            if k == DIGEST_SID:
                csp, shape = AhSA(rng, 256).csp(), None
            else:
                sa = kinds[k % len(kinds)] if k < NMIX else cheap[k % len(cheap)]
                csp = sa.esp_sa().csp()
                s = E.esp_frame_shape(sa.esp_sa(), 0)
                shape = (s.ivlen, s.alen)
            rc, sid = self.drv.newsession(csp)
            assert rc == 0 and sid == k, (rc, sid, k)
            self.shapes.append(shape)
        self.drv.freesession(FREED_SID)
        self.shapes[FREED_SID] = None
        assert {s for s in self.shapes[:NMIX] if s} >= {(8, 16), (8, 12), (8, 8), (16, 12), (16, 24), (16, 32), (0, 12),
                                                         (0, 32), (16, 0), (8, 0)}


@pytest.fixture(scope="module")
def env():
    _torch()
    e = Env(NSES)
    yield e
    e.drv.close()
    import gc
    gc.collect()


def _insa(rng, nin, flags=None):
    from espgpu.batch import INSA_DTYPE
    t = np.zeros(nin, dtype=INSA_DTYPE)
    t["bytes"] = rng.integers(0, 2**40, nin)
    t["packets"] = rng.integers(0, 2**20, nin)
    # every mode, family and PAD_RAND; a few unusable ones
    t["flags"] = rng.integers(0, 16, nin) if flags is None else flags
    t["pad_"] = 0x0badf00d
    return t


def _synth(env, rng, sa, insa, defects=0.15, q=None):
    """Decrypted packets for the sessions sa[i] as the decrypt leaves them in
    place: (arena, PKT rec, DESC desc, trailer words).  A record of a session
    the ctx does not hold as ESP, or past the insa table, gets the shape (8,
    16); `defects` of them a bad pad byte, a lying pad length or IPPROTO_NONE."""
    pkts, skips, rlens, trs = [], [], [], []
    for i, s in enumerate(sa):
        s = int(s)
        shape = env.shapes[s] if s < len(env.shapes) and env.shapes[s] else (8, 16)
        af6 = bool(insa["flags"][s] & 8) if s < len(insa) else False
        kw = {}
        nxt = int(rng.choice([4, 41, 6, 17, 50, 4]))
        if rng.random() < defects:
            d = int(rng.integers(3))
            if d == 0:
                kw["lastpad"] = 0xee
            elif d == 1:
                kw["padbyte"] = 0xf0
            else:
                nxt = 59
        qq = int(rng.choice([0, 19, 20, 39, 40, 64, int(rng.integers(0, 300))])) if q is None else q
        p, skip, rlen = packet(rng, af6, shape[0], shape[1], qq, nxt, ihl=int(rng.integers(5, 16)), **kw)
        pkts.append(p)
        skips.append(skip)
        rlens.append(rlen)
        trs.append(trailer_of(p, skip, rlen, shape[0], shape[1]))
    arena, rec = layout(rng, pkts)
    desc = np.zeros(len(sa), dtype=DESC)
    desc["off4"] = rec["off4"] + np.array(skips, dtype=np.int64) // 4
    desc["len"], desc["sa"] = rlens, sa
    desc["esn_hi"], desc["salt"] = 0x5a5a5a5a, 0xa5a5a5a5
    return arena, rec, desc, np.array(trs, dtype=np.uint32)


def _run(env, arena, rec, desc, trailer, status, insa, inplace=True, calls=None, stream=None):
    """Upload, esp_decap (once, or per (start, count, nin) of `calls` back to
    back without a sync), download and compare everything with the host rule
    applied to the same calls.  Out of place, d_out starts as the arena with
    every outer header overwritten, so the header can only come from d_arena.
    Returns the device (out, ipkt, dstatus, insa)."""
    torch = _torch()
    from espgpu.batch import INSA_DTYPE, PKT_DTYPE, esp_decap
    n, nin = len(rec), len(insa)
    calls = calls or [(0, n, nin)]
    out0 = arena
    if not inplace:
        out0 = arena.copy()
        for i in range(n):
            o, skip = int(rec["off4"][i]) * 4, (int(desc["off4"][i]) - int(rec["off4"][i])) * 4
            out0[o:o + skip] = 0x99
    iguard = np.zeros(3, dtype=INSA_DTYPE)
    iguard.view(np.uint8)[:] = 0xC3
    d_arena = _up(torch, arena)
    d_out = d_arena if inplace else _up(torch, out0)
    d_rec, d_desc, d_st = _up(torch, rec), _up(torch, desc), _up(torch, status)
    d_tr = torch.from_numpy(trailer.view(np.int32).copy()).cuda()
    d_in = _up(torch, np.concatenate([insa, iguard]))
    d_ipkt = torch.full(((n + GUARD) * 8,), 0xC3, dtype=torch.uint8, device="cuda")
    d_dst = torch.full((n + GUARD,), 0x77, dtype=torch.uint8, device="cuda")
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
    for a, cnt, ni in calls:
        esp_decap(env.drv, d_arena, d_out, d_rec[a * 8:], d_desc[a * 16:], d_tr[a:], d_st[a:], cnt,
                  d_in[:ni * INSA_DTYPE.itemsize], d_ipkt[a * 8:], d_dst[a:], stream=stream)
    if stream is not None:
        stream.synchronize()
    else:
        torch.cuda.synchronize()
    w_out, w_in = out0, insa.copy()
    w_ipkt, w_dst = np.zeros(n, dtype=PKT_DTYPE), np.zeros(n, dtype=np.uint8)
    for a, cnt, ni in calls:
        sl = slice(a, a + cnt)
        w_out, w_ipkt[sl], w_dst[sl], w_in[:ni] = host_decap_batch(
            arena if not inplace else w_out, w_out, rec[sl], desc[sl], trailer[sl], status[sl], w_in[:ni], env.shapes)
    g_out, g_dst = d_out.cpu().numpy(), d_dst.cpu().numpy()
    g_ipkt, g_in = d_ipkt.cpu().numpy(), d_in.cpu().numpy().view(INSA_DTYPE)
    bad = np.flatnonzero(g_dst[:n] != w_dst)
    assert bad.size == 0, ("dstatus", bad[:8], g_dst[bad[:8]], w_dst[bad[:8]], desc["sa"][bad[:8]])
    gp = g_ipkt[:n * 8].view(PKT_DTYPE)
    bad = np.flatnonzero(gp != w_ipkt)
    assert bad.size == 0, ("ipkt", bad[:8], gp[bad[:8]], w_ipkt[bad[:8]])
    assert (g_dst[n:] == 0x77).all() and (g_ipkt[n * 8:] == 0xC3).all(), "wrote past n"
    for fld in ("bytes", "packets", "flags", "pad_"):
        bad = np.flatnonzero(g_in[fld][:nin] != w_in[fld])
        assert bad.size == 0, ("insa." + fld, bad[:8], g_in[fld][bad[:8]], w_in[fld][bad[:8]], insa[fld][bad[:8]])
    assert np.array_equal(g_in[nin:].view(np.uint8), iguard.view(np.uint8)), "insa guard entries written"
    bad = np.flatnonzero(g_out != w_out)
    assert bad.size == 0, ("out", bad[:16], g_out[bad[:16]], w_out[bad[:16]])
    if not inplace:
        assert np.array_equal(d_arena.cpu().numpy(), arena), "arena modified"
    assert np.array_equal(d_rec.cpu().numpy(), rec.view(np.uint8)), "d_pkt modified"
    assert np.array_equal(d_desc.cpu().numpy(), desc.view(np.uint8)), "d_desc modified"
    assert np.array_equal(d_tr.cpu().numpy().view(np.uint32), trailer), "d_trailer modified"
    assert np.array_equal(d_st.cpu().numpy(), status), "d_status modified"
    return g_out, gp, g_dst[:n], g_in[:nin]


@pytest.fixture(scope="module")
def mixed(env):
    """The module's pool: 3000 packets over the 40 SAs of every shape, mode and
    family, laid out once, with records that take no part."""
    rng = np.random.default_rng(32)
    n = 3000
    insa = _insa(rng, NMIX + 3)
    insa["flags"][:12] = [0, 1, 2, 8, 9, 10, 4, 5, 6, 12, 13, 14]
    sa = rng.integers(0, NMIX, n)
    sa[rng.random(n) < 0.03] = NMIX + 3 + 2                  # sa >= nin, a session the ctx holds
    sa[rng.random(n) < 0.01] = 0xffff
    arena, rec, desc, trailer = _synth(env, rng, sa, insa)
    status = np.zeros(n, dtype=np.uint8)
    failed = rng.random(n) < 0.1
    status[failed] = rng.choice([EACCES, EBADMSG, EINVAL, 2, ENOTSUP], int(failed.sum()))
    trailer[failed & (rng.random(n) < 0.7)] = 0
    return arena, rec, desc, trailer, status, insa


@pytest.mark.gpu
@pytest.mark.parametrize("inplace", [True, False], ids=["inplace", "outofplace"])
def test_mixed_batch(env, mixed, inplace):
    arena, rec, desc, trailer, status, insa = mixed
    assert {DIGEST_SID, FREED_SID} <= set(desc["sa"].tolist())
    _, ipkt, dst, g_in = _run(env, arena, rec, desc, trailer, status, insa, inplace)
    assert {int(x) for x in np.unique(dst)} == {0, EINVAL, ENODATA, EPFNOSUPPORT}
    ok = (dst == 0) & (status == 0)
    assert 1000 < ok.sum() < 2600
    assert (dst[status != 0] == 0).all() and (ipkt["len"][~ok] == 0).all()
    assert np.array_equal(ipkt["off4"][~ok], rec["off4"][~ok])
    for s in (DIGEST_SID, FREED_SID):
        assert (dst[(desc["sa"] == s) & (status == 0)] == EINVAL).all()
        assert (g_in["bytes"][s], g_in["packets"][s]) == (insa["bytes"][s], insa["packets"][s])
    assert (dst[(desc["sa"] >= len(insa)) & (status == 0)] == EINVAL).all()
    tunnel = ok & (ipkt["off4"] - rec["off4"] >= 7)          # skip + hlen >= 28 > 24 >= hlen
    assert 100 < tunnel.sum() < ok.sum() - 100
    assert int((g_in["packets"] - insa["packets"]).sum()) == int(ok.sum())
    assert int((g_in["bytes"] - insa["bytes"]).sum()) == int(ipkt["len"][ok].sum())


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 1025])
def test_launch_edges(env, mixed, n):
    arena, rec, desc, trailer, status, insa = mixed
    sl = slice(11, 11 + n)
    _run(env, arena, rec[sl], desc[sl], trailer[sl], status[sl], insa, n & 1 == 1)


@pytest.mark.gpu
def test_one_sa_with_a_counter_at_the_carry(env):
    """20 000 records of one SA: 313 waves add to one pair of counters, and
    bytes crosses 2^32."""
    rng = np.random.default_rng(33)
    n = 20000
    insa = _insa(rng, 8, flags=[1, 2, 0, 0, 1, 9, 10, 8])
    insa["bytes"][3], insa["packets"][3] = 2**32 - 100, 2**32 - 7
    arena, rec, desc, trailer = _synth(env, rng, np.full(n, 3), insa, defects=0.02, q=24)
    _, _, dst, g_in = _run(env, arena, rec, desc, trailer, np.zeros(n, dtype=np.uint8), insa)
    assert 12000 < (dst == 0).sum() < n
    assert g_in["bytes"][3] > 2**32 and g_in["packets"][3] == 2**32 - 7 + (dst == 0).sum()


@pytest.mark.gpu
def test_sa_patterns_inside_a_wave_and_a_workgroup(env):
    """Workgroup by workgroup (256 records, four waves): two SAs alternating
    lane by lane and a wave with no accepted lane; a wave whose only accepted
    lane is lane 63, a wave of 64 different SAs and two waves of runs; four
    waves of one SA each, not all the same; one SA in two waves and nothing
    accepted in the other two; a last workgroup of ten records."""
    rng = np.random.default_rng(34)
    insa = _insa(rng, NSES, flags=np.where(np.arange(NSES) & 1, 0, 1))      # wildcard and transport: q 40 passes
    sa = np.r_[np.tile([5, 8], 96), np.full(64, 5),
               np.full(64, 8), 100 + np.arange(64), np.tile([6, 7, 7], 43)[:128],
               np.full(64, 5), np.full(64, 8), np.full(128, 5),
               np.full(256, 9),
               np.full(10, 5)]
    n = len(sa)
    assert n == 4 * 256 + 10
    arena, rec, desc, trailer = _synth(env, rng, sa, insa, defects=0.0, q=40)
    status = np.zeros(n, dtype=np.uint8)
    status[192:256] = EBADMSG                                # the fourth wave: nothing accepted
    status[256:319] = EACCES                                 # the fifth: lane 63 alone
    status[768 + 3:768 + 60] = EBADMSG                       # a few lanes of one SA ...
    status[768 + 64:768 + 128] = EACCES                      # ... no lane ...
    status[768 + 192:1024] = EINVAL                          # ... a whole wave, no lane
    _, _, dst, g_in = _run(env, arena, rec, desc, trailer, status, insa, inplace=False)
    taking = status == 0
    assert (dst[taking] == 0).all() and taking[319] and not taking[192:319].any()
    for s, cnt in ((5, 96 + 64 + 128 + 10), (8, 96 + 1 + 64), (9, 7 + 64), (6, 43), (7, 85), (131, 1)):
        assert g_in["packets"][s] - insa["packets"][s] == cnt, s


@pytest.mark.gpu
def test_a_thousand_sas_with_one_to_three_records_each(env):
    rng = np.random.default_rng(35)
    insa = _insa(rng, NSES, flags=rng.choice([0, 1, 2, 8, 9, 10, 6], NSES))
    sa = np.repeat(40 + np.arange(1024), rng.integers(1, 4, 1024))
    rng.shuffle(sa)
    arena, rec, desc, trailer = _synth(env, rng, sa, insa, defects=0.05)
    _, _, dst, g_in = _run(env, arena, rec, desc, trailer, np.zeros(len(sa), dtype=np.uint8), insa)
    touched = np.flatnonzero(g_in["packets"] != insa["packets"])
    assert 600 < touched.size <= 1024 and touched.min() >= 40


@pytest.mark.gpu
def test_two_calls_on_a_callers_stream(env, mixed):
    """No sync between the calls: the second call's counters continue from the
    first's, and its nin is smaller."""
    torch = _torch()
    arena, rec, desc, trailer, status, insa = mixed
    cut = 1300
    _, _, dst, g_in = _run(env, arena, rec, desc, trailer, status, insa, inplace=False,
                           calls=[(0, cut, len(insa)), (cut, len(rec) - cut, 30)], stream=torch.cuda.Stream())
    late = (desc["sa"][cut:] >= 30) & (status[cut:] == 0)
    assert late.sum() > 100 and (dst[cut:][late] == EINVAL).all()
    both = np.flatnonzero((g_in["packets"][:30] - insa["packets"][:30]) > 0)
    assert both.size >= 25


@pytest.mark.gpu
def test_zero_packets_and_arguments(env, mixed):
    torch = _torch()
    from espgpu.batch import INSA_DTYPE
    arena, rec, desc, trailer, status, insa = mixed
    lib, ctx = env.drv.lib, env.drv.ctx
    d_arena, d_rec, d_desc, d_st = _up(torch, arena[:8192]), _up(torch, rec[:4]), _up(torch, desc[:4]), _up(torch, status[:4])
    d_tr = torch.from_numpy(trailer[:4].view(np.int32).copy()).cuda()
    d_in = _up(torch, insa)
    d_ipkt = torch.zeros(32, dtype=torch.uint8, device="cuda")
    d_dst = torch.zeros(4, dtype=torch.uint8, device="cuda")
    args = (d_arena.data_ptr(), d_arena.data_ptr(), d_rec.data_ptr(), d_desc.data_ptr(), d_tr.data_ptr(),
            d_st.data_ptr(), 4, d_in.data_ptr(), len(insa), d_ipkt.data_ptr(), d_dst.data_ptr(), None)
    assert lib.espgpu_esp_decap_batch(ctx, None, None, None, None, None, None, 0, None, 0, None, None, None) == 0
    assert lib.espgpu_esp_decap_batch(None, *args) == EINVAL
    for k, v in ((0, None), (1, None), (2, None), (3, None), (4, None), (5, None), (7, None), (9, None), (10, None),
                 (0, d_arena.data_ptr() + 2), (1, d_arena.data_ptr() + 1)):
        a = list(args)
        a[k] = v
        assert lib.espgpu_esp_decap_batch(ctx, *a) == EINVAL, (k, v)
    torch.cuda.synchronize()
    assert np.array_equal(d_in.cpu().numpy().view(INSA_DTYPE), insa) and not d_dst.cpu().numpy().any()
    assert lib.espgpu_health(ctx) == 0
    # nin 0 needs no table: every record with status 0 is refused
    a = list(args)
    a[7], a[8] = None, 0
    assert lib.espgpu_esp_decap_batch(ctx, *a) == 0
    torch.cuda.synchronize()
    assert np.array_equal(d_dst.cpu().numpy(), np.where(status[:4] == 0, EINVAL, 0))
    assert lib.espgpu_esp_decap_batch(ctx, *args) == 0
    torch.cuda.synchronize()


# ---- end to end ----------------------------------------------------------------
def _outer(meta, body_len, proto):
    """The outer header of an SA's packets around body_len bytes of `proto`."""
    if meta["af"] == 6:
        return ipv6(meta["dst"], b"", nxt=proto, plen=body_len)
    return ipv4(meta["dst"], b"", ihl=meta["ihl"], proto=proto, ip_len=meta["ihl"] * 4 + body_len, opts=meta["opts"])


def _outbound(drv, rng, sas, metas, outsa, shapes, items):
    """items (SA index, payload, next header) through esp_frame ->
    encrypt_batch -> replay_merge; outsa (a device tensor) advances.  Returns
    the packets as they go on the wire, each under its SA's outer header."""
    torch = _torch()
    from espgpu.batch import encrypt_batch, esp_frame, replay_merge
    n = len(items)
    desc = np.zeros(n, dtype=DESC)
    frame = np.zeros(n, dtype=np.uint32)
    pos, place = 0, []
    for i, (k, payload, nh) in enumerate(items):
        rl = record_len(shapes[k], len(payload))
        desc[i] = (pos // 4, rl, k, 0, 0)
        frame[i] = len(payload) | nh << 16
        place.append(pos)
        pos += (rl + 3 & ~3) + 4 * int(rng.integers(0, 4))
    arena = rng.integers(0, 256, pos + 64, dtype=np.uint8)
    for (k, payload, _), o in zip(items, place):
        a = o + 8 + shapes[k].ivlen
        arena[a:a + len(payload)] = np.frombuffer(payload, dtype=np.uint8)
    d_arena, d_desc = _up(torch, arena), _up(torch, desc)
    d_fst = torch.zeros(n, dtype=torch.uint8, device="cuda")
    d_st = torch.full((n,), 0x55, dtype=torch.uint8, device="cuda")
    esp_frame(drv, d_arena, d_desc, torch.from_numpy(frame.view(np.int32).copy()).cuda(), n, outsa, d_fst)
    encrypt_batch(drv, d_arena, d_desc, n, d_st)
    replay_merge(drv, d_st, d_fst, n)
    torch.cuda.synchronize()
    assert not d_st.cpu().numpy().any()
    g = d_arena.cpu().numpy()
    return [_outer(metas[k], int(desc["len"][i]), 50) + g[o:o + int(desc["len"][i])].tobytes()
            for i, ((k, _, _), o) in enumerate(zip(items, place))]


def _inbound(drv, d_arena, d_rec, n, d_sad, d_tab, d_words, d_in, ivalens):
    """The whole inbound sequence in place, on d_rec (a PKT tensor).  Before
    the decapsulation everything is downloaded, so that step is compared with
    the host rule as in every other test here.  Returns (final status, ipkt,
    dstatus, final arena, status before the decapsulation)."""
    torch = _torch()
    from espgpu.batch import (INSA_DTYPE, PKT_DTYPE, decrypt_batch, esp_classify, esp_decap, replay_check,
                              replay_merge, replay_update)
    mk = lambda: torch.zeros(n, dtype=torch.uint8, device="cuda")
    cst, rst, ust, st, dst = mk(), mk(), mk(), mk(), mk()
    tr = torch.zeros(n, dtype=torch.int32, device="cuda")
    d_desc = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
    d_ipkt = torch.zeros(n * 8, dtype=torch.uint8, device="cuda")
    esp_classify(drv, d_arena, d_rec, n, d_sad, d_desc, cst, flags=1)
    replay_check(drv, d_arena, d_desc, n, d_tab, d_words, rst)
    decrypt_batch(drv, d_arena, d_desc, n, st, trailer=tr)
    replay_update(drv, d_arena, d_desc, n, st, d_tab, d_words, ust)
    replay_merge(drv, st, rst, n)
    replay_merge(drv, st, ust, n)
    replay_merge(drv, st, cst, n)
    torch.cuda.synchronize()
    pre = (d_arena.cpu().numpy(), d_rec.cpu().numpy().view(PKT_DTYPE), d_desc.cpu().numpy().view(DESC),
           tr.cpu().numpy().view(np.uint32), st.cpu().numpy(), d_in.cpu().numpy().view(INSA_DTYPE))
    esp_decap(drv, d_arena, d_arena, d_rec, d_desc, tr, st, n, d_in, d_ipkt, dst)
    replay_merge(drv, st, dst, n)
    torch.cuda.synchronize()
    w_out, w_ipkt, w_dst, w_in = host_decap_batch(pre[0], pre[0], pre[1], pre[2], pre[3], pre[4], pre[5], ivalens)
    g_arena, g_ipkt, g_dst = d_arena.cpu().numpy(), d_ipkt.cpu().numpy().view(PKT_DTYPE), dst.cpu().numpy()
    assert np.array_equal(g_dst, w_dst) and np.array_equal(g_ipkt, w_ipkt)
    assert np.array_equal(g_arena, w_out), np.flatnonzero(g_arena != w_out)[:16]
    assert np.array_equal(d_in.cpu().numpy(), w_in.view(np.uint8))
    return st.cpu().numpy(), d_ipkt, g_dst, g_arena, pre[4]


@pytest.mark.gpu
def test_outbound_then_inbound_end_to_end():
    """Host-built inner packets -> esp_frame -> encrypt -> outer IPv4 (with
    options) and IPv6 headers -> the inbound sequence with the decapsulation at
    its end, on GCM and CBC+HMAC SAs in tunnel, transport and wildcard mode.
    Tunnel results are the inner packets byte for byte, transport results the
    original transport packets; a tunnel packet whose inner packet is itself
    ESP goes round again through esp_classify on d_ipkt; replayed and forged
    records stay refused, keep their bytes and book nothing."""
    torch = _torch()
    from espgpu import _lib as L
    from espgpu import esp as E
    from espgpu.batch import INSA_DTYPE, OUTSA_DTYPE, PKT_DTYPE, REPLAY_DTYPE, SAD_DTYPE, sad_build
    from espgpu.opencrypto import GpuCryptoDriver
    rng = np.random.default_rng(36)
    sas = [GcmSA(rng), GcmSA(rng, 32), EtaSA(rng), EtaSA(rng, sha256=True), GcmSA(rng, mlen=12), GcmSA(rng)]
    modes = [L.IN_TUNNEL, L.IN_TRANSPORT, L.IN_TRANSPORT, L.IN_TUNNEL, 0, L.IN_TUNNEL]
    afs, ihls = [4, 6, 4, 6, 4, 4], [6, 0, 9, 0, 5, 5]
    NEST = 5                                                 # the SA inside SA 0's tunnel
    nsa = len(sas)
    metas = []
    for k in range(nsa):
        dst = rng.integers(1, 255, 4 if afs[k] == 4 else 16, dtype=np.uint8)
        dst[0] = 0x20
        metas.append(dict(af=afs[k], ihl=ihls[k], dst=dst.tobytes(),
                          opts=rng.integers(0, 256, max(ihls[k] * 4 - 20, 0), dtype=np.uint8).tobytes()))
    drv = GpuCryptoDriver(max_sessions=16, batch_records=1024, batch_bytes=1 << 20, nbatches=1)
    try:
        for k, s in enumerate(sas):
            rc, sid = drv.newsession(s.esp_sa().csp())
            assert rc == 0 and sid == k
        outsa = np.zeros(nsa, dtype=OUTSA_DTYPE)
        for k, s in enumerate(sas):
            outsa[k] = (100 * k, 5000 * k, s.spi, int.from_bytes(s.salt, "little"), L.OUT_PAD_SEQ, 0)
        shapes = [E.esp_frame_shape(s.esp_sa(), L.OUT_PAD_SEQ) for s in sas]
        ivalens = [(s.ivlen, s.alen) for s in shapes]
        d_outsa = _up(torch, outsa)

        def inner(kind):
            body = rng.integers(0, 256, int(rng.integers(8, 300)), dtype=np.uint8).tobytes()
            if kind == 4:
                return ipv4(rng.integers(1, 255, 4, dtype=np.uint8).tobytes(), body, proto=17)
            return ipv6(rng.integers(1, 255, 16, dtype=np.uint8).tobytes(), body, nxt=17)

        # the nested SA's packets first: they are SA 0's payloads
        innermost = [inner(4) for _ in range(12)]
        nested = _outbound(drv, rng, sas, metas, d_outsa, shapes, [(NEST, p, 4) for p in innermost])
        items, want = [], []
        for p in nested:
            items.append((0, p, 4))
            want.append(p)
        for _ in range(150):
            k = int(rng.integers(0, 5))
            if modes[k] == L.IN_TRANSPORT or (modes[k] == 0 and rng.random() < 0.5):
                nh = int(rng.choice([6, 17]))
                payload = rng.integers(0, 256, int(rng.integers(0, 300)), dtype=np.uint8).tobytes()
                items.append((k, payload, nh))
                want.append(_outer(metas[k], len(payload), nh) + payload)
            else:
                nh = int(rng.choice([4, 41]))
                items.append((k, inner(nh), nh))
                want.append(items[-1][1])
        order = rng.permutation(len(items))                  # (the framing numbers each SA's records in this order)
        items, want = [items[i] for i in order], [want[i] for i in order]
        wire = _outbound(drv, rng, sas, metas, d_outsa, shapes, items)
        n1 = len(wire)
        # replays and forgeries at the end of the batch
        replays = [int(x) for x in rng.choice(n1, 10, replace=False)]
        forged = [int(x) for x in rng.choice(n1, 10, replace=False)]
        pkts = list(wire) + [wire[i] for i in replays]
        for i in forged:
            b = bytearray(wire[i])
            b[len(b) - 1 - int(rng.integers(0, 8))] ^= 0x10
            pkts.append(bytes(b))
        n = len(pkts)
        arena, rec = layout(rng, pkts)

        ent = np.zeros(nsa, dtype=SAD_DTYPE)
        for k, s in enumerate(sas):
            ent["spi"][k], ent["sa"][k], ent["proto"][k], ent["af"][k] = s.spi, k, 50, afs[k]
            ent["salt"][k] = int.from_bytes(s.salt, "little")
            ent["dst"][k, :len(metas[k]["dst"])] = np.frombuffer(metas[k]["dst"], dtype=np.uint8)
        d_sad = _up(torch, sad_build(ent, 16))
        tab = np.zeros(nsa, dtype=REPLAY_DTYPE)
        for k in range(nsa):
            tab[k] = (outsa["count"][k], 64, 32, 32 * k, 0)
        d_tab, d_words = _up(torch, tab), torch.zeros(32 * nsa, dtype=torch.int32, device="cuda")
        insa = np.zeros(nsa + 2, dtype=INSA_DTYPE)
        insa["flags"][:nsa] = [m | (L.IN_AF6 if a == 6 else 0) for m, a in zip(modes, afs)]
        insa["bytes"], insa["packets"] = 1000, 10
        d_in = _up(torch, insa)

        d_arena, d_rec = _up(torch, arena), _up(torch, rec)
        st, d_ipkt, dst, out, pre_st = _inbound(drv, d_arena, d_rec, n, d_sad, d_tab, d_words, d_in, ivalens)
        assert not st[:n1].any(), (np.flatnonzero(st[:n1])[:8], st[:n1][st[:n1] != 0][:8])
        assert (st[n1:n1 + 10] == EACCES).all() and (st[n1 + 10:] == EBADMSG).all()
        assert not dst[n1:].any()
        ipkt = d_ipkt.cpu().numpy().view(PKT_DTYPE)
        assert not ipkt["len"][n1:].any()
        for j in range(n1, n):                               # refused: the bytes the step found are the bytes it left
            o = int(rec["off4"][j]) * 4
            src = pkts[j]
            if j >= n1 + 10:                                 # forged: still the ciphertext
                assert out[o:o + len(src)].tobytes() == src
        for i in range(n1):
            o = int(ipkt["off4"][i]) * 4
            got = out[o:o + int(ipkt["len"][i])].tobytes()
            assert got == want[i], (i, items[i][0], items[i][2])
            k, _, nh = items[i]
            if nh not in (4, 41):                            # transport: a header ip_input takes
                assert got[0] >> 4 == afs[k]
                rc, _ = E.ipsec_input_classify({}, got, ipcsum=True)
                assert rc == ENOTSUP                         # sane, and no longer ESP
                if afs[k] == 4:
                    assert E.in_cksum(got[:ihls[k] * 4]) == 0
        g_in = d_in.cpu().numpy().view(INSA_DTYPE)
        for k in range(5):
            mine = [i for i in range(n1) if items[i][0] == k]
            assert g_in["packets"][k] == 10 + len(mine) and g_in["bytes"][k] == 1000 + sum(len(want[i]) for i in mine)
        assert (g_in["packets"][NEST], g_in["bytes"][NEST]) == (10, 1000)

        # round two: d_ipkt as it stands is the next round's d_pkt
        st2, d_ipkt2, dst2, out2, _ = _inbound(drv, d_arena, d_ipkt, n, d_sad, d_tab, d_words, d_in, ivalens)
        ipkt2 = d_ipkt2.cpu().numpy().view(PKT_DTYPE)
        isnest = np.array([i < n1 and items[i][0] == 0 and items[i][1] in nested for i in range(n)])
        assert isnest.sum() == 12 and not st2[isnest].any() and st2[~isnest].all()
        found = []
        for i in np.flatnonzero(isnest):
            o = int(ipkt2["off4"][i]) * 4
            found.append(out2[o:o + int(ipkt2["len"][i])].tobytes())
        assert sorted(found) == sorted(innermost)
        g_in = d_in.cpu().numpy().view(INSA_DTYPE)
        assert (g_in["packets"][NEST], g_in["bytes"][NEST]) == (22, 1000 + sum(len(p) for p in innermost))
    finally:
        drv.close()
