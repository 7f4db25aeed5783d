"""espgpu_esp_encap_batch and espgpu_esp_sent_batch (encap.hip): the first and
the last step of the outbound sequence on a device-resident batch.  Every test
compares the device batch with the host rules espgpu_esp_encap / espgpu_esp_sent
(pinned against esp.py's restatement of the reference in test_esp_encap.py)
applied in index order: the whole arena with the random bytes between the
spans, all of d_desc, d_frame, d_opkt and d_estatus with guard entries past n,
every espgpu_encsa and the guard entries after it, and the inputs unchanged."""
import struct

import numpy as np
import pytest

from ah_helpers import AhSA
from classify_helpers import ipv4, ipv6
from encap_helpers import (EAFNOSUPPORT, EINVAL, EMSGSIZE, ENOBUFS, ENOTSUP, addr, host_encap_batch,
                           host_sent_batch, inner4, inner6, layout)
from frame_helpers import sa_kinds
from helpers import DESC, EtaSA, GcmSA

EACCES, EBADMSG = 13, 74
GUARD = 5
NSES = 48                   # sessions of the module's driver
DIGEST_SID, FREED_SID = 21, 22
NMIX = 40                   # the SAs of the mixed batches: every kind, mode and family
HEAD, TAIL = 56, 40         # short for a CBC SA's IPv6 tunnel (24 + 40) and for 32-byte ICVs behind long padding


def _torch():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.fail("GPU test run without a visible HIP device")
    return torch


def _up(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()


class Env:
    """A driver whose sessions 0 .. NSES - 1 cycle through every ESP kind,
    except DIGEST_SID (an AH session) and FREED_SID (freed again); outsa holds
    each session's framing flags (CTRCOMPAT where the kind asks for it) and
    shapes[sa] its L.EShape under them, None for those two."""

    def __init__(self, nses):
        from espgpu import _lib as L
        from espgpu import esp as E
        from espgpu.batch import OUTSA_DTYPE
        from espgpu.opencrypto import GpuCryptoDriver
        rng = np.random.default_rng(61)
        self.drv = GpuCryptoDriver(max_sessions=nses + 4, batch_records=1024, batch_bytes=1 << 20, nbatches=1)
        kinds = [(sa, fl) for _, sa, fl in sa_kinds(rng)] + [(s, 0) for s in (
            GcmSA(rng, mlen=12), GcmSA(rng, mlen=8), EtaSA(rng, sha=384), EtaSA(rng, sha=512),
            EtaSA(rng, null=True, sha=512))]
        self.shapes, self.sas = [], []
        self.outsa = np.zeros(nses, dtype=OUTSA_DTYPE)
        for k in range(nses):
            if k == DIGEST_SID:
                csp, shape, sa = AhSA(rng, 256).csp(), None, None
            else:
                sa, fl = kinds[k % len(kinds)]
                csp = sa.esp_sa().csp()
                shape = E.esp_frame_shape(sa.esp_sa(), fl)
                self.outsa[k] = (10 * k, 1000 * k, sa.spi, int.from_bytes(sa.salt, "little"), fl | L.OUT_PAD_SEQ, 0)
            rc, sid = self.drv.newsession(csp)
            assert rc == 0 and sid == k, (rc, sid, k)
            self.shapes.append(shape)
            self.sas.append(sa)
        self.drv.freesession(FREED_SID)
        self.shapes[FREED_SID] = None
        assert {(s.ivlen, s.blks, s.alen) for s in self.shapes[:NMIX] if s} >= {
            (8, 4, 16), (8, 4, 12), (8, 4, 8), (16, 16, 12), (16, 16, 24), (16, 16, 32), (0, 4, 12), (0, 4, 32),
            (16, 16, 0), (8, 4, 0), (8, 16, 16)}


@pytest.fixture(scope="module")
def env():
    _torch()
    e = Env(NSES)
    yield e
    e.drv.close()
    import gc
    gc.collect()


def _enc_table(rng, nenc):
    """SAs of every policy; a few unusable ones at fixed places."""
    from espgpu import _lib as L
    from espgpu.batch import ENCSA_DTYPE
    t = np.zeros(nenc, dtype=ENCSA_DTYPE)
    t["bytes"] = rng.integers(0, 2**40, nenc)
    t["packets"] = rng.integers(0, 2**20, nenc)
    t["ttl"] = rng.integers(1, 256, nenc)
    t["pad_"] = 0xa7
    for k in range(nenc):
        af6 = bool(k & 1)
        fl = ((L.ENC_TUNNEL if k & 2 else 0) | (L.ENC_AF6 if af6 else 0) | int(rng.choice([0, 4, 8])) |
              int(rng.choice([0, 0x10, 0x20])) | (L.ENC_RFC6864 if k & 4 else 0))
        t["flags"][k] = fl
        for f in ("src", "dst"):
            a = addr(rng, af6)
            t[f][k, :len(a)] = np.frombuffer(a, dtype=np.uint8)
    if nenc <= 35:
        return t
    t["flags"][30] = 0x0c                                    # both DF bits
    t["flags"][31] = 0x30 | L.ENC_AF6                        # both ECN bits
    t["flags"][32] = 0x180
    t["src"][33] = 0                                         # an AF6 SA (odd id) with no source
    t["dst"][35, :2] = [0xfe, 0x80]                          # link-local
    t["dst"][34] = 0                                         # AF_INET wildcard: transport, or EINVAL in a tunnel
    t["flags"][34] &= ~np.uint32(L.ENC_TUNNEL)
    return t


def _packets(env, rng, sa, enc):
    """Cleartext packets for the SAs sa[i]: both families, half of them to
    their SA's destination, with a few the rule refuses."""
    pkts = []
    for i, s in enumerate(sa):
        s = int(s)
        e = enc[s] if s < len(enc) else enc[0]
        v6 = bool(rng.integers(2)) if rng.random() < 0.3 else bool(e["flags"] & 2)
        dst = None
        if rng.random() < 0.6 and v6 == bool(e["flags"] & 2):
            dst = e["dst"][:16 if v6 else 4].tobytes()
        plen = int(rng.choice([0, 1, 2, 3, 40, int(rng.integers(0, 400))]))
        p = inner6(rng, plen, dst=dst) if v6 else inner4(rng, int(rng.integers(5, 16)), plen, dst=dst)
        r = rng.random()
        if r < 0.02:
            p = bytes([int(rng.choice([0, 5, 7])) << 4 | 5]) + p[1:]
        elif r < 0.04:
            p = p[:int(rng.integers(0, 20))]
        elif r < 0.05 and not v6:
            p = p[:4 * (p[0] & 0xf) - 1]
        pkts.append(p)
    return pkts


def _run(env, arena, rec, sa, enc, id0=0xfff0, calls=None, stream=None, headroom=HEAD, tailroom=TAIL):
    """Upload, esp_encap (once, or per (start, count, nenc) of `calls` back to
    back without a sync), download and compare everything with the host rule
    applied to the same calls.  Returns the device (arena, desc, frame, opkt,
    estatus)."""
    torch = _torch()
    from espgpu.batch import ENCSA_DTYPE, PKT_DTYPE, esp_encap
    n, nenc = len(rec), len(enc)
    calls = calls or [(0, n, nenc)]
    eguard = np.zeros(3, dtype=ENCSA_DTYPE)
    eguard.view(np.uint8)[:] = 0xC3
    sa16 = np.ascontiguousarray(sa, dtype=np.uint16)
    frame0 = np.full(n + GUARD, 0x77777777, dtype=np.uint32)
    d_arena, d_rec, d_sa = _up(torch, arena), _up(torch, rec), torch.from_numpy(sa16.view(np.int16).copy()).cuda()
    d_enc, d_out = _up(torch, np.concatenate([enc, eguard])), _up(torch, env.outsa)
    d_desc = torch.full(((n + GUARD) * 16,), 0xC3, dtype=torch.uint8, device="cuda")
    d_frame = torch.from_numpy(frame0.view(np.int32).copy()).cuda()
    d_opkt = torch.full(((n + GUARD) * 8,), 0xC3, dtype=torch.uint8, device="cuda")
    d_est = torch.full((n + GUARD,), 0x77, dtype=torch.uint8, device="cuda")
    if stream is not None:
        stream.wait_stream(torch.cuda.current_stream())
    for a, cnt, ne in calls:
        assert ne <= len(env.outsa)
        esp_encap(env.drv, d_arena, d_rec[a * 8:], d_sa[a:], cnt, d_enc[:ne * ENCSA_DTYPE.itemsize],
                  d_out, headroom, tailroom, id0 + a, d_desc[a * 16:], d_frame[a:], d_opkt[a * 8:], d_est[a:],
                  stream=stream)
    if stream is not None:
        stream.synchronize()
    else:
        torch.cuda.synchronize()
    w_arena = arena
    w_desc, w_frame = np.zeros(n, dtype=DESC), frame0[:n].copy()
    w_opkt, w_est = np.zeros(n, dtype=PKT_DTYPE), np.zeros(n, dtype=np.uint8)
    for a, cnt, ne in calls:
        sl = slice(a, a + cnt)
        w_arena, w_desc[sl], w_frame[sl], w_opkt[sl], w_est[sl] = host_encap_batch(
            w_arena, rec[sl], sa16[sl], enc[:ne], env.shapes, headroom, tailroom, id0 + a, frame0[sl])
    g_est = d_est.cpu().numpy()
    bad = np.flatnonzero(g_est[:n] != w_est)
    assert bad.size == 0, ("estatus", bad[:8], g_est[bad[:8]], w_est[bad[:8]], sa16[bad[:8]])
    g_desc = d_desc.cpu().numpy()
    gd = g_desc[:n * 16].view(DESC)
    bad = np.flatnonzero(gd != w_desc)
    assert bad.size == 0, ("desc", bad[:8], gd[bad[:8]], w_desc[bad[:8]])
    g_opkt = d_opkt.cpu().numpy()
    gp = g_opkt[:n * 8].view(PKT_DTYPE)
    bad = np.flatnonzero(gp != w_opkt)
    assert bad.size == 0, ("opkt", bad[:8], gp[bad[:8]], w_opkt[bad[:8]])
    g_frame = d_frame.cpu().numpy().view(np.uint32)
    bad = np.flatnonzero(g_frame[:n] != w_frame)
    assert bad.size == 0, ("frame", bad[:8], g_frame[bad[:8]], w_frame[bad[:8]])
    assert (g_est[n:] == 0x77).all() and (g_desc[n * 16:] == 0xC3).all() and (g_opkt[n * 8:] == 0xC3).all()
    assert (g_frame[n:] == 0x77777777).all(), "wrote past n"
    g_arena = d_arena.cpu().numpy()
    bad = np.flatnonzero(g_arena != w_arena)
    assert bad.size == 0, ("arena", bad[:16], g_arena[bad[:16]], w_arena[bad[:16]])
    assert np.array_equal(d_enc.cpu().numpy(), np.concatenate([enc, eguard]).view(np.uint8)), "d_enc modified"
    assert np.array_equal(d_rec.cpu().numpy(), rec.view(np.uint8)), "d_pkt modified"
    assert np.array_equal(d_sa.cpu().numpy().view(np.uint16), sa16), "d_sa modified"
    assert np.array_equal(d_out.cpu().numpy(), env.outsa.view(np.uint8)), "d_out modified"
    return g_arena, gd, g_frame[:n], gp, g_est[:n]


@pytest.fixture(scope="module")
def mixed(env):
    """The module's pool: 1000 packets over the 40 SAs of every shape, policy
    and family at an irregular stride, with packets that take no part, and
    one packet too long and one whose result would be."""
    rng = np.random.default_rng(62)
    n = 1000
    enc = _enc_table(rng, NMIX + 3)
    sa = rng.integers(0, NMIX, n)
    sa[rng.random(n) < 0.03] = NMIX + 3 + 2                  # sa >= nenc, a session the ctx holds
    sa[rng.random(n) < 0.01] = 0xffff
    pkts = _packets(env, rng, sa, enc)
    sa[500], sa[501] = 0, 2
    pkts[500] = inner4(rng, 5, 65536 - 20 + 44)              # len > 65535
    pkts[501] = inner4(rng, 5, 65500 - 20)                   # total > 65535 behind a tunnel's headers
    arena, rec = layout(rng, pkts, HEAD, TAIL)
    return arena, rec, sa, enc


@pytest.mark.gpu
def test_mixed_batch(env, mixed):
    arena, rec, sa, enc = mixed
    assert {DIGEST_SID, FREED_SID} <= set(sa.tolist())
    g_arena, desc, frame, opkt, est = _run(env, arena, rec, sa, enc)
    assert {int(x) for x in np.unique(est)} == {0, EINVAL, ENOTSUP, EAFNOSUPPORT, EMSGSIZE, ENOBUFS}
    assert est[500] == EMSGSIZE and est[501] == EMSGSIZE
    ok = est == 0
    assert 500 < ok.sum() < 900
    for s in (DIGEST_SID, FREED_SID, 30, 31, 32, 33):
        assert (est[sa == s] == EINVAL).all()
    assert (est[sa == 35] == ENOTSUP).all() and (est[sa >= len(enc)] == EINVAL).all()
    assert (desc["len"][~ok] == 0).all() and (desc["sa"][~ok] == 0xffff).all() and (opkt["len"][~ok] == 0).all()
    assert np.array_equal(desc["off4"][~ok], rec["off4"][~ok]) and np.array_equal(opkt["off4"][~ok], rec["off4"][~ok])
    front = (rec["off4"][ok].astype(np.int64) - opkt["off4"][ok]) * 4
    tunnel = front >= 28
    assert 100 < tunnel.sum() < ok.sum() - 100
    assert set(np.unique(front).tolist()) >= {8, 16, 24, 28, 36, 44, 48, 56}
    # an outer IPv4 header's id is id0 + i, through the wrap at 2^16, unless RFC 6864 zeroes it
    ids = 0
    for i in np.flatnonzero(ok):
        f, o = int(enc["flags"][sa[i]]), int(opkt["off4"][i]) * 4
        if not f & 2 and (int(rec["off4"][i]) * 4 - o) >= 28:
            ident, df = struct.unpack(">H", g_arena[o + 4:o + 6].tobytes())[0], g_arena[o + 6] & 0x40
            assert ident == (0 if f & 0x40 and df else (0xfff0 + i) & 0xffff), i
            ids += 1
    assert ids > 50


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257])
def test_launch_edges(env, mixed, n):
    """(n = 1000 is test_mixed_batch.)"""
    arena, rec, sa, enc = mixed
    sl = slice(7, 7 + n)
    _run(env, arena, rec[sl], sa[sl], enc, id0=n)


@pytest.mark.gpu
def test_two_calls_on_a_callers_stream(env, mixed):
    """No sync between the calls; the second call's nenc is smaller and its
    ids go on from the first's."""
    torch = _torch()
    arena, rec, sa, enc = mixed
    cut = 430
    _, _, _, _, est = _run(env, arena, rec, sa, enc, id0=0x1fffe,
                           calls=[(0, cut, len(enc)), (cut, len(rec) - cut, 30)], stream=torch.cuda.Stream())
    late = sa[cut:] >= 30
    assert late.sum() > 50 and (est[cut:][late] == EINVAL).all()


@pytest.mark.gpu
def test_zero_packets_and_arguments(env, mixed):
    torch = _torch()
    arena, rec, sa, enc = mixed
    lib, ctx = env.drv.lib, env.drv.ctx
    n = 4
    d_arena, d_rec = _up(torch, arena[:8192]), _up(torch, rec[:n])
    d_sa = torch.from_numpy(np.ascontiguousarray(sa[:n], dtype=np.uint16).view(np.int16).copy()).cuda()
    d_enc, d_out = _up(torch, enc), _up(torch, env.outsa)
    d_desc = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
    d_frame = torch.zeros(n, dtype=torch.int32, device="cuda")
    d_opkt = torch.zeros(n * 8, dtype=torch.uint8, device="cuda")
    d_est = torch.zeros(n, dtype=torch.uint8, device="cuda")
    d_st = torch.zeros(n, dtype=torch.uint8, device="cuda")
    args = (d_arena.data_ptr(), d_rec.data_ptr(), d_sa.data_ptr(), n, d_enc.data_ptr(), d_out.data_ptr(), len(enc),
            HEAD, TAIL, 0, d_desc.data_ptr(), d_frame.data_ptr(), d_opkt.data_ptr(), d_est.data_ptr(), None)
    assert lib.espgpu_esp_encap_batch(ctx, None, None, None, 0, None, None, 0, 0, 0, 0, None, None, None, None,
                                      None) == 0
    assert lib.espgpu_esp_encap_batch(None, *args) == EINVAL
    for k, v in ((0, None), (1, None), (2, None), (4, None), (5, None), (10, None), (11, None), (12, None),
                 (13, None), (0, d_arena.data_ptr() + 2), (0, d_arena.data_ptr() + 1)):
        a = list(args)
        a[k] = v
        assert lib.espgpu_esp_encap_batch(ctx, *a) == EINVAL, (k, v)
    sargs = (d_opkt.data_ptr(), d_desc.data_ptr(), d_st.data_ptr(), n, d_enc.data_ptr(), len(enc), None)
    assert lib.espgpu_esp_sent_batch(ctx, None, None, None, 0, None, 0, None) == 0
    assert lib.espgpu_esp_sent_batch(None, *sargs) == EINVAL
    for k in (0, 1, 2, 4):
        a = list(sargs)
        a[k] = None
        assert lib.espgpu_esp_sent_batch(ctx, *a) == EINVAL, k
    torch.cuda.synchronize()
    assert np.array_equal(d_enc.cpu().numpy(), enc.view(np.uint8)) and not d_est.cpu().numpy().any()
    assert np.array_equal(d_arena.cpu().numpy(), arena[:8192])
    assert lib.espgpu_health(ctx) == 0
    # nenc 0 needs no tables: every packet takes no part
    a = list(args)
    a[4], a[5], a[6] = None, None, 0
    assert lib.espgpu_esp_encap_batch(ctx, *a) == 0
    torch.cuda.synchronize()
    assert (d_est.cpu().numpy() == EINVAL).all() and np.array_equal(d_arena.cpu().numpy(), arena[:8192])


# ---- espgpu_esp_sent_batch -------------------------------------------------------
def _sent(env, opkt_len, sa, status, enc, calls=None):
    torch = _torch()
    from espgpu.batch import ENCSA_DTYPE, PKT_DTYPE, esp_sent
    n, nenc = len(sa), len(enc)
    opkt = np.zeros(n, dtype=PKT_DTYPE)
    opkt["off4"], opkt["len"] = np.arange(n) * 400, opkt_len
    desc = np.zeros(n, dtype=DESC)
    desc["off4"], desc["len"], desc["sa"] = opkt["off4"] + 5, 100, sa
    eguard = np.zeros(3, dtype=ENCSA_DTYPE)
    eguard.view(np.uint8)[:] = 0xC3
    d_opkt, d_desc, d_st = _up(torch, opkt), _up(torch, desc), _up(torch, status)
    d_enc = _up(torch, np.concatenate([enc, eguard]))
    want = enc
    for a, cnt in calls or [(0, n)]:
        esp_sent(env.drv, d_opkt[a * 8:], d_desc[a * 16:], d_st[a:], cnt, d_enc[:nenc * ENCSA_DTYPE.itemsize])
        want = host_sent_batch(opkt[a:a + cnt], desc[a:a + cnt], status[a:a + cnt], want)
    torch.cuda.synchronize()
    got = d_enc.cpu().numpy().view(ENCSA_DTYPE)
    for fld in ("bytes", "packets"):
        bad = np.flatnonzero(got[fld][:nenc] != want[fld])
        assert bad.size == 0, ("encsa." + fld, bad[:8], got[fld][bad[:8]], want[fld][bad[:8]], enc[fld][bad[:8]])
    assert np.array_equal(got[:nenc].view(np.uint8).reshape(nenc, -1)[:, 16:],
                          enc.view(np.uint8).reshape(nenc, -1)[:, 16:]), "policy fields written"
    assert np.array_equal(got[nenc:].view(np.uint8), eguard.view(np.uint8)), "encsa guard entries written"
    assert np.array_equal(d_opkt.cpu().numpy(), opkt.view(np.uint8)) and np.array_equal(d_st.cpu().numpy(), status)
    assert np.array_equal(d_desc.cpu().numpy(), desc.view(np.uint8))
    return got[:nenc]


@pytest.mark.gpu
@pytest.mark.parametrize("n", [1, 64, 255, 256, 257, 1000])
def test_sent_one_sa_holds_the_whole_batch(env, n):
    """The workgroup path, with bytes crossing 2^32 and a second call going on
    from the first's sums."""
    rng = np.random.default_rng(63)
    enc = _enc_table(rng, 8)
    enc["bytes"][3], enc["packets"][3] = 2**32 - 70000, 2**32 - 3
    lens = rng.integers(20, 65536, n)
    lens[0] = 65535
    got = _sent(env, lens, np.full(n, 3), np.zeros(n, dtype=np.uint8), enc, calls=[(0, n), (n // 3, n - n // 3)])
    assert got["bytes"][3] == 2**32 - 70000 + int(lens.sum()) + int(lens[n // 3:].sum())
    assert got["packets"][3] == 2**32 - 3 + 2 * n - n // 3


@pytest.mark.gpu
def test_sent_sa_patterns_inside_a_wave_and_a_workgroup(env):
    """Workgroup by workgroup (256 records, four waves): two SAs alternating
    lane by lane and a wave with no accepted lane; a wave whose only accepted
    lane is lane 63, a wave of 64 different SAs and two waves of runs; four
    waves of one SA each, not all the same; one SA in two waves and nothing
    accepted in the other two, with records past nenc; a last workgroup of
    ten records."""
    rng = np.random.default_rng(64)
    nenc = 200
    enc = _enc_table(rng, nenc)
    sa = np.r_[np.tile([5, 8], 96), np.full(64, 5),
               np.full(64, 8), 100 + np.arange(64), np.tile([6, 7, 7], 43)[:128],
               np.full(64, 5), np.full(64, 8), np.full(128, 5),
               np.full(128, 9), np.full(64, nenc), np.full(64, 0xffff),
               np.full(10, 5)]
    n = len(sa)
    assert n == 4 * 256 + 10
    status = np.zeros(n, dtype=np.uint8)
    status[192:256] = EBADMSG                                # the fourth wave: nothing accepted
    status[256:319] = EACCES                                 # the fifth: lane 63 alone
    status[768 + 3:768 + 60] = EINVAL                        # a few lanes of one SA
    got = _sent(env, rng.integers(20, 1600, n), sa, status, enc)
    for s, cnt in ((5, 96 + 64 + 128 + 10), (8, 96 + 1 + 64), (9, 7 + 64), (6, 43), (7, 85), (131, 1)):
        assert got["packets"][s] - enc["packets"][s] == cnt, s


@pytest.mark.gpu
def test_sent_many_sas_and_refused_records(env):
    rng = np.random.default_rng(65)
    nenc, n = 1024, 3000
    enc = _enc_table(rng, nenc)
    sa = rng.integers(0, nenc + 20, n)
    status = np.where(rng.random(n) < 0.2, rng.choice([EINVAL, EBADMSG, ENOBUFS, 1], n), 0).astype(np.uint8)
    got = _sent(env, rng.integers(20, 65536, n), sa, status, enc)
    assert int((got["packets"] - enc["packets"]).sum()) == int(((status == 0) & (sa < nenc)).sum())


# ---- the whole loop ----------------------------------------------------------------
@pytest.mark.gpu
def test_outbound_then_inbound_end_to_end():
    """Cleartext packets -> encap -> frame -> encrypt -> merges -> sent, then
    d_opkt through classify -> replay check -> decrypt -> update -> merges ->
    decap, on GCM and CBC+HMAC SAs, tunnel and transport, IPv4 and IPv6 (with
    options): the bytes at d_ipkt are the cleartext packets that went in, and
    the oracle decrypts what lies on the wire."""
    torch = _torch()
    from espgpu import _lib as L
    from espgpu import esp as E
    from espgpu.batch import (ENCSA_DTYPE, INSA_DTYPE, OUTSA_DTYPE, PKT_DTYPE, REPLAY_DTYPE, SAD_DTYPE,
                              decrypt_batch, encrypt_batch, esp_classify, esp_decap, esp_encap, esp_frame, esp_sent,
                              replay_check, replay_merge, replay_update, sad_build)
    from espgpu.opencrypto import GpuCryptoDriver
    rng = np.random.default_rng(66)
    sas = [GcmSA(rng), GcmSA(rng, 32), EtaSA(rng), EtaSA(rng, sha256=True), GcmSA(rng, mlen=12), EtaSA(rng, sha=512)]
    tun = [True, False, False, True, True, False]
    afs = [4, 6, 4, 6, 6, 4]                                 # SA 4: IPv4 inside an IPv6 tunnel
    inner_af = [4, 6, 4, 6, 4, 4]
    nsa = len(sas)
    drv = GpuCryptoDriver(max_sessions=16, batch_records=1024, batch_bytes=1 << 20, nbatches=1)
    try:
        for k, s in enumerate(sas):
            rc, sid = drv.newsession(s.esp_sa().csp())
            assert rc == 0 and sid == k
        outsa = np.zeros(nsa, dtype=OUTSA_DTYPE)
        enc = np.zeros(nsa + 1, dtype=ENCSA_DTYPE)
        for k, s in enumerate(sas):
            outsa[k] = (100 * k, 5000 * k, s.spi, int.from_bytes(s.salt, "little"), L.OUT_PAD_SEQ, 0)
            enc["flags"][k] = (L.ENC_TUNNEL if tun[k] else 0) | (L.ENC_AF6 if afs[k] == 6 else 0) | L.ENC_DF_COPY
            enc["ttl"][k] = 40 + k
            for f in ("src", "dst"):
                a = addr(rng, afs[k] == 6)
                enc[f][k, :len(a)] = np.frombuffer(a, dtype=np.uint8)
        enc["bytes"], enc["packets"] = 1000, 10
        shapes = [E.esp_frame_shape(s.esp_sa(), L.OUT_PAD_SEQ) for s in sas]
        n = 180
        sa = rng.integers(0, nsa, n)
        pkts = []
        for k in sa:
            dst = enc["dst"][k, :16 if afs[k] == 6 else 4].tobytes() if not tun[k] else addr(rng, inner_af[k] == 6)
            body = rng.integers(0, 256, int(rng.integers(0, 300)), dtype=np.uint8).tobytes()
            if inner_af[k] == 6:
                pkts.append(ipv6(dst, body, nxt=int(rng.choice([6, 17]))))
            else:
                ihl = int(rng.integers(5, 16))
                pkts.append(ipv4(dst, body, ihl=ihl, proto=int(rng.choice([6, 17])),
                                 opts=rng.integers(0, 256, ihl * 4 - 20, dtype=np.uint8).tobytes()))
        head, tail = 64, 49
        arena, rec = layout(rng, pkts, head, tail)
        d_arena, d_rec = _up(torch, arena), _up(torch, rec)
        d_sa = torch.from_numpy(sa.astype(np.uint16).view(np.int16).copy()).cuda()
        d_enc, d_outsa = _up(torch, enc), _up(torch, np.concatenate([outsa, np.zeros(1, dtype=OUTSA_DTYPE)]))
        mk = lambda: torch.zeros(n, dtype=torch.uint8, device="cuda")        # noqa: E731
        est, fst, st = mk(), mk(), torch.full((n,), 0x55, dtype=torch.uint8, device="cuda")
        d_desc = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
        d_frame = torch.zeros(n, dtype=torch.int32, device="cuda")
        d_opkt = torch.zeros(n * 8, dtype=torch.uint8, device="cuda")
        # outbound, no sync in between
        esp_encap(drv, d_arena, d_rec, d_sa, n, d_enc, d_outsa, head, tail, 7, d_desc, d_frame, d_opkt, est)
        esp_frame(drv, d_arena, d_desc, d_frame, n, d_outsa, fst)
        encrypt_batch(drv, d_arena, d_desc, n, st)
        replay_merge(drv, st, fst, n)
        replay_merge(drv, st, est, n)
        esp_sent(drv, d_opkt, d_desc, st, n, d_enc)
        torch.cuda.synchronize()
        assert not st.cpu().numpy().any(), (est.cpu().numpy(), fst.cpu().numpy(), st.cpu().numpy())
        wire = d_arena.cpu().numpy()
        opkt, desc = d_opkt.cpu().numpy().view(PKT_DTYPE), d_desc.cpu().numpy().view(DESC)
        g_enc = d_enc.cpu().numpy().view(ENCSA_DTYPE)
        for k in range(nsa):
            assert g_enc["packets"][k] == 10 + (sa == k).sum()
            assert g_enc["bytes"][k] == 1000 + int(opkt["len"][sa == k].sum())
        assert (g_enc["packets"][nsa], g_enc["bytes"][nsa]) == (10, 1000)
        for i, k in enumerate(sa):                           # the oracle opens every record on the wire
            o, ln = int(desc["off4"][i]) * 4, int(desc["len"][i])
            rc, pt = sas[k].oracle.esp_decrypt(wire[o:o + ln].tobytes(), 0)
            assert rc == 0
            hl, p = 8 + shapes[k].ivlen, pkts[i]
            inner = p if tun[k] else p[40 if inner_af[k] == 6 else 4 * (p[0] & 0xf):]
            assert pt[hl:hl + len(inner)] == inner
            w0 = int(opkt["off4"][i]) * 4
            assert wire[w0] >> 4 == afs[k]
            if afs[k] == 4:
                assert E.in_cksum(wire[w0:w0 + 4 * (int(wire[w0]) & 0xf)].tobytes()) == 0
        # inbound: d_opkt as it stands is the received-packet list
        ent = np.zeros(nsa, dtype=SAD_DTYPE)
        for k, s in enumerate(sas):
            ent["spi"][k], ent["sa"][k], ent["proto"][k], ent["af"][k] = s.spi, k, 50, afs[k]
            ent["salt"][k] = int.from_bytes(s.salt, "little")
            ent["dst"][k] = enc["dst"][k]
        d_sad = _up(torch, sad_build(ent, 16))
        tab = np.zeros(nsa, dtype=REPLAY_DTYPE)
        for k in range(nsa):
            tab[k] = (outsa["count"][k], 64, 32, 32 * k, 0)
        d_tab, d_words = _up(torch, tab), torch.zeros(32 * nsa, dtype=torch.int32, device="cuda")
        insa = np.zeros(nsa, dtype=INSA_DTYPE)
        insa["flags"] = [(L.IN_TUNNEL if t else L.IN_TRANSPORT) | (L.IN_AF6 if a == 6 else 0) for t, a in zip(tun, afs)]
        d_in = _up(torch, insa)
        cst, rst, ust, ist, dst = mk(), mk(), mk(), mk(), mk()
        tr = torch.zeros(n, dtype=torch.int32, device="cuda")
        d_idesc = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
        d_ipkt = torch.zeros(n * 8, dtype=torch.uint8, device="cuda")
        esp_classify(drv, d_arena, d_opkt, n, d_sad, d_idesc, cst, flags=1)
        replay_check(drv, d_arena, d_idesc, n, d_tab, d_words, rst)
        decrypt_batch(drv, d_arena, d_idesc, n, ist, trailer=tr)
        replay_update(drv, d_arena, d_idesc, n, ist, d_tab, d_words, ust)
        replay_merge(drv, ist, rst, n)
        replay_merge(drv, ist, ust, n)
        replay_merge(drv, ist, cst, n)
        esp_decap(drv, d_arena, d_arena, d_opkt, d_idesc, tr, ist, n, d_in, d_ipkt, dst)
        replay_merge(drv, ist, dst, n)
        torch.cuda.synchronize()
        assert not ist.cpu().numpy().any(), (cst.cpu().numpy(), rst.cpu().numpy(), ist.cpu().numpy(), dst.cpu().numpy())
        idesc = d_idesc.cpu().numpy().view(DESC)
        for fld in ("off4", "len", "sa"):                    # classification finds the records the encapsulation made
            assert np.array_equal(idesc[fld], desc[fld]), fld
        out, ipkt = d_arena.cpu().numpy(), d_ipkt.cpu().numpy().view(PKT_DTYPE)
        for i, p in enumerate(pkts):
            o = int(ipkt["off4"][i]) * 4
            assert int(ipkt["len"][i]) == len(p) and out[o:o + len(p)].tobytes() == p, (i, int(sa[i]))
            assert o == int(rec["off4"][i]) * 4              # and they lie where they lay
        g_in = d_in.cpu().numpy().view(INSA_DTYPE)
        for k in range(nsa):
            assert g_in["packets"][k] == (sa == k).sum() and g_in["bytes"][k] == sum(len(pkts[i]) for i in
                                                                                   np.flatnonzero(sa == k))
    finally:
        drv.close()
