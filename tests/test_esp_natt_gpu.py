"""NAT-T on the device-resident batch path: cls_kernel, dcp_kernel, enc_kernel and
snt_kernel with UDP-encapsulated packets and NAT-T SAs, and the checksum
kernels of natt.hip.  Every test compares the device batch with the host rules
(pinned against esp.py's restatements of the reference in test_esp_natt.py)
applied in index order: whole arenas with the random bytes between the
packets, every output array, the SA tables, and the inputs unchanged.  Each
test asserts that its batch holds every class it names."""
import struct

import numpy as np
import pytest

import classify_helpers as CH
import decap_helpers as DH
import encap_helpers as EH
import natt_helpers as NH
from frame_helpers import sa_kinds
from helpers import DESC, EtaSA, GcmSA

EINVAL, ENOTSUP, ENOENT, EBADMSG = 22, 95, 2, 74
PORT = NH.PORT
EDGES = [1, 63, 64, 65, 255, 256, 257, 1025]


def _torch():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.fail("GPU test run without a visible HIP device")
    return torch


def _up(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()


class Env:
    """A driver with one session per ESP kind; shapes[sa] is its L.EShape."""

    def __init__(self):
        from espgpu import _lib as L
        from espgpu import esp as E
        from espgpu.batch import OUTSA_DTYPE
        from espgpu.opencrypto import GpuCryptoDriver
        rng = np.random.default_rng(1301)
        kinds = [(sa, fl) for _, sa, fl in sa_kinds(rng)] + [(GcmSA(rng, mlen=12), 0), (EtaSA(rng, sha=512), 0)]
        self.drv = GpuCryptoDriver(max_sessions=len(kinds) + 4, batch_records=1024, batch_bytes=1 << 20, nbatches=1)
        self.shapes, self.outsa = [], np.zeros(len(kinds), dtype=OUTSA_DTYPE)
        for k, (sa, fl) in enumerate(kinds):
            rc, sid = self.drv.newsession(sa.esp_sa().csp())
            assert rc == 0 and sid == k
            self.shapes.append(E.esp_frame_shape(sa.esp_sa(), fl))
            self.outsa[k] = (10 * k, 1000 * k, sa.spi, int.from_bytes(sa.salt, "little"), fl | L.OUT_PAD_SEQ, 0)
        self.nsa = len(kinds)
        assert {s.ivlen for s in self.shapes} == {0, 8, 16}


@pytest.fixture(scope="module")
def env():
    _torch()
    e = Env()
    yield e
    e.drv.close()
    import gc
    gc.collect()


# ---- (a) classification ------------------------------------------------------------
@pytest.fixture(scope="module")
def cls_batch():
    from espgpu.batch import sad_build
    rng = np.random.default_rng(1302)
    db = NH.NattSadb(rng)
    pkts = [(k, NH.natt_packet(rng, db, PORT, k)) for k in NH.NATT_KINDS for _ in range(60)]
    pkts += CH.random_packets(rng, db, 2048 - len(pkts) + 37)
    order = rng.permutation(len(pkts))
    pkts = [pkts[j] for j in order]
    arena, rec = CH.layout(rng, [p for _, p in pkts])
    return db, sad_build(db.entries, 128), [k for k, _ in pkts], arena, rec


def _classify(env, table, arena, rec, flags):
    torch = _torch()
    from espgpu.batch import esp_classify
    n = len(rec)
    d_arena, d_rec, d_tab = _up(torch, arena), _up(torch, rec), _up(torch, table)
    d_desc = torch.full(((n + 3) * 16,), 0xC3, dtype=torch.uint8, device="cuda")
    d_st = torch.full((n + 3,), 0x77, dtype=torch.uint8, device="cuda")
    esp_classify(env.drv, d_arena, d_rec, n, d_tab, d_desc, d_st, flags=flags)
    torch.cuda.synchronize()
    w_desc, w_st = CH.host_classify_batch(table, arena, rec, flags)
    g_st, g_desc = d_st.cpu().numpy(), d_desc.cpu().numpy()
    bad = np.flatnonzero(g_st[:n] != w_st)
    assert bad.size == 0, ("cstatus", bad[:8], g_st[bad[:8]], w_st[bad[:8]])
    gd = g_desc[:n * 16].view(DESC)
    bad = np.flatnonzero(gd != w_desc)
    assert bad.size == 0, ("desc", bad[:8], gd[bad[:8]], w_desc[bad[:8]])
    assert (g_st[n:] == 0x77).all() and (g_desc[n * 16:] == 0xC3).all(), "wrote past n"
    assert np.array_equal(d_arena.cpu().numpy(), arena) and np.array_equal(d_tab.cpu().numpy(), table.view(np.uint8))
    return gd, g_st[:n]


@pytest.mark.gpu
def test_classify_mixed_batch_with_the_port_and_without(env, cls_batch):
    from espgpu import _lib as L
    db, table, kinds, arena, rec = cls_batch
    assert len(rec) > 2048 and set(kinds) >= set(NH.NATT_KINDS) | set(CH.KINDS)
    desc, st = _classify(env, table, arena, rec, L.CLS_NATT_PORT(PORT))
    kinds = np.array(kinds)
    for k, want in NH.NATT_KINDS.items():
        assert (st[kinds == k] == want).all(), (k, st[kinds == k])
    natt_ok = np.isin(kinds, ["good", "trim", "tail"])
    assert natt_ok.sum() == 180 and (desc["len"][natt_ok] >= 8).all()
    for i in np.flatnonzero(natt_ok)[:50]:
        o = int(rec["off4"][i]) * 4
        assert int(desc["off4"][i]) == int(rec["off4"][i]) + (int(arena[o]) & 0xf) + 2
    # port 0 on the same arena: today's rule; every UDP packet is the host's
    desc0, st0 = _classify(env, table, arena, rec, 0)
    udp = np.array([arena[int(r["off4"]) * 4 + 9] == 17 and arena[int(r["off4"]) * 4] >> 4 == 4 and r["len"] >= 20
                    for r in rec])
    isnatt = np.isin(kinds, list(NH.NATT_KINDS))
    assert (st0[isnatt & udp & (kinds != "frag")] == ENOTSUP).all() and (desc0["len"][isnatt] == 0).all()
    assert np.array_equal(st0[~isnatt], st[~isnatt]) and np.array_equal(desc0[~isnatt], desc[~isnatt])
    # and, beside the NAT-T SAs' own packets, what the restatement of before gives
    from espgpu import esp as E
    plain = {spi: v[:5] for spi, v in db.ref.items()}
    for i in np.flatnonzero(~isnatt)[::7]:
        o = int(rec["off4"][i]) * 4
        p = arena[o:o + int(rec["len"][i])].tobytes()
        w = E.ipsec_input_classify(plain, p, int(rec["off4"][i]))
        if w[0] == 0 and db.ref[struct.unpack(">I", p[(w[1][0] - int(rec["off4"][i])) * 4:][:4])[0]][5]:
            assert st0[i] == ENOTSUP
        else:
            assert (int(st0[i]), tuple(int(x) for x in desc0[i])) == w, kinds[i]


@pytest.mark.gpu
@pytest.mark.parametrize("n", EDGES[:-1])
def test_classify_launch_edges(env, cls_batch, n):
    from espgpu import _lib as L
    _, table, _, arena, rec = cls_batch
    _classify(env, table, arena, rec[11:11 + n], L.CLS_NATT_PORT(PORT) | L.CLS_IPCSUM)


# ---- (b) decapsulation and encapsulation ----------------------------------------------
@pytest.fixture(scope="module")
def dcp_batch(env):
    """1025 decrypted packets, NAT-T and plain SAs lane by lane: insa[k] is
    session k's, odd ones NAT-T."""
    from espgpu import _lib as L
    from espgpu.batch import INSA_DTYPE
    rng = np.random.default_rng(1303)
    n, nsa = 1025, env.nsa
    insa = np.zeros(nsa + 2, dtype=INSA_DTYPE)
    insa["bytes"], insa["packets"] = rng.integers(0, 2**40, nsa + 2), rng.integers(0, 2**20, nsa + 2)
    for k in range(nsa + 2):
        insa["flags"][k] = DH.in_flags(DH.MODES[k % 3]) | (L.IN_NATT if k & 1 else 0)
        insa["pad_"][k] = int(rng.integers(0, 65536))
    sa = rng.integers(0, nsa, n)
    sa[256:320] = 1                                                  # a wave of one NAT-T SA
    sa[320:384] = 2                                                  # and one of a plain SA
    pkts, skips, rlens = [], [], []
    for i in range(n):
        s = env.shapes[sa[i]]
        q, nxt, ihl = int(rng.choice([0, 20, 40, 77])), int(rng.choice([6, 17, 4, 41, 50])), int(rng.integers(5, 16))
        if sa[i] & 1:
            p, skip, rlen = NH.natt_in_packet(rng, s.ivlen, s.alen, q, nxt, ihl=ihl)
        else:
            p, skip, rlen = DH.packet(rng, False, s.ivlen, s.alen, q, nxt, ihl=ihl)
        pkts.append(p), skips.append(skip), rlens.append(rlen)
    arena, rec = DH.layout(rng, pkts)
    desc = np.zeros(n, dtype=DESC)
    desc["off4"], desc["len"], desc["sa"] = rec["off4"] + np.array(skips) // 4, rlens, sa
    trailer = np.array([DH.trailer_of(p, sk, rl, env.shapes[s].ivlen, env.shapes[s].alen)
                        for p, sk, rl, s in zip(pkts, skips, rlens, sa)], dtype=np.uint32)
    status = np.where(rng.random(n) < 0.1, EBADMSG, 0).astype(np.uint8)
    # a NAT-T SA's packet whose skip lacks the UDP header, and a plain SA's with it: refused
    desc["off4"][5] = rec["off4"][5] + (5 if sa[5] & 1 else 17)
    return arena, rec, desc, trailer, status, insa, sa


def _decap(env, b, sl):
    torch = _torch()
    from espgpu.batch import INSA_DTYPE, PKT_DTYPE, esp_decap
    arena, rec, desc, trailer, status, insa, _ = b
    rec, desc, trailer, status = rec[sl], desc[sl], trailer[sl], status[sl]
    n = len(rec)
    d_arena, d_rec, d_desc = _up(torch, arena), _up(torch, rec), _up(torch, desc)
    d_tr, d_st, d_in = torch.from_numpy(trailer.view(np.int32).copy()).cuda(), _up(torch, status), _up(torch, insa)
    d_ipkt = torch.full(((n + 3) * 8,), 0xC3, dtype=torch.uint8, device="cuda")
    d_dst = torch.full((n + 3,), 0x77, dtype=torch.uint8, device="cuda")
    esp_decap(env.drv, d_arena, d_arena, d_rec, d_desc, d_tr, d_st, n, d_in, d_ipkt, d_dst)
    torch.cuda.synchronize()
    shapes = [(s.ivlen, s.alen) for s in env.shapes]
    w_out, w_ipkt, w_dst, w_in = NH.host_decap_batch(arena, arena, rec, desc, trailer, status, insa, shapes)
    g_dst = d_dst.cpu().numpy()
    bad = np.flatnonzero(g_dst[:n] != w_dst)
    assert bad.size == 0, ("dstatus", bad[:8], g_dst[bad[:8]], w_dst[bad[:8]])
    g_ipkt = d_ipkt.cpu().numpy()
    gp = g_ipkt[:n * 8].view(PKT_DTYPE)
    bad = np.flatnonzero(gp != w_ipkt)
    assert bad.size == 0, ("ipkt", bad[:8], gp[bad[:8]], w_ipkt[bad[:8]])
    assert (g_dst[n:] == 0x77).all() and (g_ipkt[n * 8:] == 0xC3).all(), "wrote past n"
    g_arena = d_arena.cpu().numpy()
    bad = np.flatnonzero(g_arena != w_out)
    assert bad.size == 0, ("arena", bad[:16])
    g_in = d_in.cpu().numpy().view(INSA_DTYPE)
    assert np.array_equal(g_in, w_in), ("insa", g_in, w_in)
    return gp, g_dst[:n], g_in


@pytest.mark.gpu
@pytest.mark.parametrize("n", EDGES)
def test_decap_launch_edges_natt_and_plain_mixed(env, dcp_batch, n):
    from espgpu import _lib as L
    sl = slice(0, n) if n == 1025 else slice(3, 3 + n)
    ipkt, dst, g_in = _decap(env, dcp_batch, sl)
    if n == 1025:
        arena, rec, desc, trailer, status, insa, sa = dcp_batch
        assert dst[5] == EINVAL and status[5] == 0
        ok = (dst == 0) & (status == 0)
        natt = (insa["flags"][sa] & L.IN_NATT) != 0
        skip = (desc["off4"].astype(np.int64) - rec["off4"]) * 4
        hlen = np.array([8 + env.shapes[s].ivlen for s in sa])
        off = (ipkt["off4"].astype(np.int64) - rec["off4"]) * 4
        tunnel = ok & (off == skip + hlen)
        for cls in (ok & natt & tunnel, ok & natt & ~tunnel, ok & ~natt & tunnel, ok & ~natt & ~tunnel):
            assert cls.sum() > 40
        assert (off[ok & natt & ~tunnel] == hlen[ok & natt & ~tunnel] + 8).all()
        assert set(np.unique(dst).tolist()) >= {0, EINVAL, 96}
        assert (g_in["packets"] - insa["packets"]).sum() == ok.sum()


def _enc_table(env, rng):
    from espgpu import _lib as L
    from espgpu.batch import ENCSA_DTYPE
    t = np.zeros(env.nsa + 2, dtype=ENCSA_DTYPE)
    t["bytes"], t["packets"] = rng.integers(0, 2**40, len(t)), rng.integers(0, 2**20, len(t))
    t["ttl"] = rng.integers(1, 256, len(t))
    for k in range(len(t)):
        t["flags"][k] = ((L.ENC_TUNNEL if k & 2 else 0) | (L.ENC_NATT if k & 1 else 0) | int(rng.choice([0, 4, 8])) |
                         int(rng.choice([0, 0x10, 0x20])))
        for f in ("src", "dst"):
            t[f][k, :4] = np.frombuffer(EH.addr(rng, False), dtype=np.uint8)
        if k & 1:
            t["dst"][k, 4:8] = np.frombuffer(struct.pack(">HH", 2000 + k, PORT), dtype=np.uint8)
    t["flags"][env.nsa] |= L.ENC_AF6                                 # NAT-T on an AF_INET6 SA (an id the ctx lacks)
    return t


@pytest.fixture(scope="module")
def enc_batch(env):
    rng = np.random.default_rng(1304)
    n = 1025
    enc = _enc_table(env, rng)
    sa = rng.integers(0, env.nsa, n)
    sa[256:320] = 1
    sa[320:384] = 2
    pkts = []
    for s in sa:
        e = enc[s]
        v6 = rng.random() < 0.2
        dst = e["dst"][:4].tobytes() if (not v6 and rng.random() < 0.6) else None
        plen = int(rng.choice([0, 1, 2, 3, 40, int(rng.integers(0, 300))]))
        pkts.append(EH.inner6(rng, plen) if v6 else EH.inner4(rng, int(rng.integers(5, 16)), plen, dst=dst))
    head, tail = 52, 40                                              # 52: short by 4 for a CBC tunnel with NAT-T
    arena, rec = EH.layout(rng, pkts, head, tail)
    return arena, rec, sa, enc, head, tail


def _encap(env, b, sl):
    torch = _torch()
    from espgpu.batch import ENCSA_DTYPE, PKT_DTYPE, esp_encap, esp_sent
    arena, rec, sa, enc, head, tail = b
    rec, sa16 = rec[sl], np.ascontiguousarray(sa[sl], dtype=np.uint16)
    n = len(rec)
    frame0 = np.full(n + 3, 0x77777777, dtype=np.uint32)
    d_arena, d_rec = _up(torch, arena), _up(torch, rec)
    d_sa = torch.from_numpy(sa16.view(np.int16).copy()).cuda()
    d_enc, d_out = _up(torch, enc), _up(torch, np.concatenate([env.outsa, env.outsa[:2]]))
    d_desc = torch.full(((n + 3) * 16,), 0xC3, dtype=torch.uint8, device="cuda")
    d_frame = torch.from_numpy(frame0.view(np.int32).copy()).cuda()
    d_opkt = torch.full(((n + 3) * 8,), 0xC3, dtype=torch.uint8, device="cuda")
    d_est = torch.full((n + 3,), 0x77, dtype=torch.uint8, device="cuda")
    esp_encap(env.drv, d_arena, d_rec, d_sa, n, d_enc, d_out, head, tail, 0xfff0, d_desc, d_frame, d_opkt, d_est)
    esp_sent(env.drv, d_opkt, d_desc, d_est, n, d_enc)               # the encap status stands for the merged one
    torch.cuda.synchronize()
    w_arena, w_desc, w_frame, w_opkt, w_est = EH.host_encap_batch(arena, rec, sa16, enc, env.shapes + [None, None],
                                                                  head, tail, 0xfff0, frame0)
    w_enc = EH.host_sent_batch(w_opkt, w_desc, w_est, enc)
    g_est = d_est.cpu().numpy()
    bad = np.flatnonzero(g_est[:n] != w_est)
    assert bad.size == 0, ("estatus", bad[:8], g_est[bad[:8]], w_est[bad[:8]], sa16[bad[:8]])
    gd = d_desc.cpu().numpy()
    assert np.array_equal(gd[:n * 16].view(DESC), w_desc) and (gd[n * 16:] == 0xC3).all()
    gp = d_opkt.cpu().numpy()
    assert np.array_equal(gp[:n * 8].view(PKT_DTYPE), w_opkt) and (gp[n * 8:] == 0xC3).all()
    gf = d_frame.cpu().numpy().view(np.uint32)
    assert np.array_equal(gf[:n], w_frame) and (gf[n:] == 0x77777777).all() and (g_est[n:] == 0x77).all()
    g_arena = d_arena.cpu().numpy()
    bad = np.flatnonzero(g_arena != w_arena)
    assert bad.size == 0, ("arena", bad[:16])
    g_enc = d_enc.cpu().numpy().view(ENCSA_DTYPE)
    assert np.array_equal(g_enc, w_enc), "encsa"
    return g_arena, gp[:n * 8].view(PKT_DTYPE), g_est[:n], g_enc


@pytest.mark.gpu
@pytest.mark.parametrize("n", EDGES)
def test_encap_and_sent_launch_edges_natt_and_plain_mixed(env, enc_batch, n):
    from espgpu import _lib as L
    sl = slice(0, n) if n == 1025 else slice(3, 3 + n)
    g_arena, opkt, est, g_enc = _encap(env, enc_batch, sl)
    if n == 1025:
        arena, rec, sa, enc, head, tail = enc_batch
        ok = est == 0
        natt = (enc["flags"][sa] & L.ENC_NATT) != 0
        front = (rec["off4"].astype(np.int64) - opkt["off4"]) * 4
        hlen = np.array([8 + env.shapes[s].ivlen for s in sa])
        tunnel = ok & (front - np.where(natt, 8, 0) > hlen)
        for cls in (ok & natt & tunnel, ok & natt & ~tunnel, ok & ~natt & tunnel, ok & ~natt & ~tunnel):
            assert cls.sum() > 40
        assert ((est == L.ENOBUFS) & natt).sum() > 0                 # the 8 bytes count against the headroom
        for i in np.flatnonzero(ok & natt)[:80]:
            o = int(opkt["off4"][i]) * 4
            hl = (int(g_arena[o]) & 0xf) * 4
            assert g_arena[o + 9] == 17
            assert struct.unpack(">HHHH", g_arena[o + hl:o + hl + 8].tobytes()) == (
                2000 + sa[i], PORT, int(opkt["len"][i]) - hl, 0)
        booked = g_enc["bytes"].astype(np.int64) - enc["bytes"].astype(np.int64)
        for k in range(env.nsa):
            m = ok & (sa == k)
            assert booked[k] == int(opkt["len"][m].sum()) - (8 * int(m.sum()) if k & 1 else 0), k


# ---- (c) the checksum kernels ----------------------------------------------------------
@pytest.fixture(scope="module")
def sum_batch():
    """Decapsulated packets as espgpu_esp_decap_batch leaves them: every segment
    length 0..530 for both protocols with every ip_hl, a 65535-byte packet
    between short ones, and packets that take no part for every reason, also
    as a whole lane group and as a whole wave of lane groups."""
    from espgpu import _lib as L
    from espgpu.batch import INSA_DTYPE
    rng = np.random.default_rng(1305)
    insa = np.zeros(6, dtype=INSA_DTYPE)
    insa["flags"] = [L.IN_TRANSPORT | L.IN_NATT, L.IN_TRANSPORT, L.IN_NATT, L.IN_NATT | L.IN_PAD_RAND,
                     L.IN_TUNNEL | L.IN_NATT, L.IN_TRANSPORT | L.IN_NATT]
    insa["pad_"] = [0x1234, 0x4321, 0, 0xffff, 0x8001, 0xabcd0000]      # (the last: high bits only, delta 0)
    insa["bytes"], insa["packets"] = 77, 5
    natt_sas = [0, 2, 3, 4, 5]
    pkts, sa, nxt, st, dst, why = [], [], [], [], [], []

    def add(p, s, proto, status=0, dstatus=0, tag="part"):
        pkts.append(p), sa.append(s), nxt.append(proto), st.append(status), dst.append(dstatus), why.append(tag)

    k = 0
    for seglen in range(0, 531):
        for proto in (6, 17):
            k += 1
            add(NH.tpacket(rng, proto, seglen, ihl=5 + k % 11, field=0 if k % 29 == 0 else None),
                natt_sas[k % 5], proto)
            r = k % 16
            if r == 3:
                add(NH.tpacket(rng, proto, 100), 1, proto, tag="plain_sa")
            elif r == 5:
                add(NH.tpacket(rng, proto, 100), 0, proto, status=EBADMSG, tag="status")
            elif r == 7:
                add(NH.tpacket(rng, proto, 100), 0, proto, dstatus=EINVAL, tag="dstatus")
            elif r == 9:
                add(NH.tpacket(rng, 4, 100), 0, 4, tag="nxt")
            elif r == 11:
                add(NH.tpacket(rng, proto, 100), 6 + k % 3, proto, tag="sa_past_nin")
            elif r == 13:
                add(NH.tpacket(rng, 17, 100, ulen=int(rng.choice([0, 7, 101, 60000]))), 0, 17, tag="ulen")
    while len(pkts) % 4 != 1:                                        # a short one first in the wave of 16-lane groups
        add(NH.tpacket(rng, 6, 30), 0, 6)
    add(NH.tpacket(rng, 6, 65535 - 20), 0, 6, tag="big")
    add(NH.tpacket(rng, 17, 65535 - 24, ihl=6), 4, 17, tag="big")
    add(NH.tpacket(rng, 17, 30), 0, 17)                              # and a short one last
    for _ in range(40):                                              # ten waves of lane groups that take no part
        add(NH.tpacket(rng, 6, 300), 1, 6, tag="plain_sa")
    for j in range(20):
        add(NH.tpacket(rng, 17 if j & 1 else 6, 200 + j), 0, 17 if j & 1 else 6)
    arena, ipkt = DH.layout(rng, pkts)
    n = len(pkts)
    desc = np.zeros(n, dtype=DESC)
    desc["off4"], desc["len"], desc["sa"] = ipkt["off4"], 0, sa
    trailer = (np.array(nxt, dtype=np.uint32) | 0x300 | L.TR_VALID).astype(np.uint32)
    return (arena, ipkt, desc, trailer, np.array(st, dtype=np.uint8), np.array(dst, dtype=np.uint8), insa,
            np.array(why))


def _natt_cksum(env, b, policy, with_cflags, sl=slice(None)):
    torch = _torch()
    from espgpu.batch import esp_natt_cksum
    arena, ipkt, desc, trailer, st, dst, insa, _ = b
    ipkt, desc, trailer, st, dst = ipkt[sl], desc[sl], trailer[sl], st[sl], dst[sl]
    n = len(ipkt)
    d_out, d_ipkt, d_desc = _up(torch, arena), _up(torch, ipkt), _up(torch, desc)
    d_tr, d_st, d_dst, d_in = (torch.from_numpy(trailer.view(np.int32).copy()).cuda(), _up(torch, st), _up(torch, dst),
                               _up(torch, insa))
    d_cf = torch.full((n + 3,), 0x77, dtype=torch.uint8, device="cuda") if with_cflags else None
    esp_natt_cksum(env.drv, d_out, d_ipkt, d_desc, d_tr, d_st, d_dst, n, d_in, policy=policy, cflags=d_cf)
    torch.cuda.synchronize()
    w_out, w_cf = NH.host_natt_batch(arena, ipkt, desc, trailer, st, dst, insa, policy)
    g_out = d_out.cpu().numpy()
    bad = np.flatnonzero(g_out != w_out)
    assert bad.size == 0, ("arena", policy, bad[:16], g_out[bad[:16]], w_out[bad[:16]])
    if with_cflags:
        g_cf = d_cf.cpu().numpy()
        assert np.array_equal(g_cf[:n], w_cf) and (g_cf[n:] == 0x77).all(), "cflags"
    for d, h in ((d_ipkt, ipkt), (d_desc, desc), (d_st, st), (d_dst, dst), (d_in, insa)):
        assert np.array_equal(d.cpu().numpy(), np.ascontiguousarray(h).view(np.uint8)), "an input was written"
    assert np.array_equal(d_tr.cpu().numpy().view(np.uint32), trailer)
    return g_out, w_cf


@pytest.mark.gpu
@pytest.mark.parametrize("with_cflags", [True, False], ids=["cflags", "null"])
@pytest.mark.parametrize("policy", [0, 1], ids=["auto", "recompute"])
def test_cksum_batch_every_length_and_class(env, sum_batch, policy, with_cflags):
    from espgpu import _lib as L
    arena, ipkt, desc, trailer, st, dst, insa, why = sum_batch
    assert set(why) == {"part", "plain_sa", "status", "dstatus", "nxt", "sa_past_nin", "ulen", "big"}
    i0 = int(np.flatnonzero(why == "big")[0])
    assert i0 % 4 == 1 and why[i0 - 1] == "part" and why[i0 + 2] == "part" and int(ipkt["len"][i0]) == 65535
    quiet = np.flatnonzero(why == "plain_sa")
    assert any((why[a:a + 8] == "plain_sa").all() for a in quiet if a % 4 == 0)     # whole waves of idle groups
    g_out, cf = _natt_cksum(env, sum_batch, policy, with_cflags)
    changed = np.array([not np.array_equal(g_out[int(r["off4"]) * 4:int(r["off4"]) * 4 + int(r["len"])],
                                           arena[int(r["off4"]) * 4:int(r["off4"]) * 4 + int(r["len"])]) for r in ipkt])
    assert not changed[~np.isin(why, ["part", "big", "ulen"])].any()
    assert changed[why == "big"].all() and changed[why == "part"].sum() > (400 if policy == 0 else 900)
    if policy:
        assert not changed[why == "ulen"].any() and not cf.any()
    else:
        assert (cf == L.NATT_CSUM_VALID).sum() > 50 and set(np.unique(cf).tolist()) == {0, L.NATT_CSUM_VALID}


@pytest.mark.gpu
@pytest.mark.parametrize("n", EDGES[:-1])
def test_cksum_batch_launch_edges(env, sum_batch, n):
    _natt_cksum(env, sum_batch, 1, True, slice(5, 5 + n))
    _natt_cksum(env, sum_batch, 0, True, slice(5, 5 + n))


@pytest.mark.gpu
@pytest.mark.parametrize("lanes", [8, 32])
def test_cksum_batch_other_lane_groups(env, sum_batch, lanes):
    """set_tuning "natt_lanes": the same bytes with 8 and with 32 lanes per packet."""
    assert env.drv.set_tuning("natt_lanes", 7) == EINVAL
    assert env.drv.set_tuning("natt_lanes", lanes) == 0
    try:
        _natt_cksum(env, sum_batch, 1, True)
    finally:
        assert env.drv.set_tuning("natt_lanes", 0) == 0


@pytest.mark.gpu
def test_cksum_batch_arguments(env, sum_batch):
    torch = _torch()
    lib, ctx = env.drv.lib, env.drv.ctx
    arena, ipkt, desc, trailer, st, dst, insa, _ = sum_batch
    n = 4
    d_out, d_ipkt, d_desc = _up(torch, arena[:4096]), _up(torch, ipkt[:n]), _up(torch, desc[:n])
    d_tr, d_st, d_dst = torch.zeros(n, dtype=torch.int32, device="cuda"), _up(torch, st[:n]), _up(torch, dst[:n])
    d_in = _up(torch, insa)
    args = [d_out.data_ptr(), d_ipkt.data_ptr(), d_desc.data_ptr(), d_tr.data_ptr(), d_st.data_ptr(),
            d_dst.data_ptr(), n, d_in.data_ptr(), len(insa), 1, None, None]
    assert lib.espgpu_esp_natt_cksum_batch(ctx, None, None, None, None, None, None, 0, None, 0, 1, None, None) == 0
    assert lib.espgpu_esp_natt_cksum_batch(None, *args) == EINVAL
    for k, v in ((0, None), (1, None), (2, None), (3, None), (4, None), (5, None), (7, None),
                 (0, d_out.data_ptr() + 2)):
        a = list(args)
        a[k] = v
        assert lib.espgpu_esp_natt_cksum_batch(ctx, *a) == EINVAL, (k, v)
    torch.cuda.synchronize()
    assert np.array_equal(d_out.cpu().numpy(), arena[:4096]) and lib.espgpu_health(ctx) == 0


# ---- (d) the whole loop ------------------------------------------------------------------
def end_to_end_packets(policy):
    """The loop's sessions and cleartext packets, seeded by policy (no GPU):
    -> (sas, tun, natt, delta, outsa, enc, sa, pkts, protos, head, tail, arena, rec)."""
    from espgpu import _lib as L
    from espgpu.batch import ENCSA_DTYPE, OUTSA_DTYPE
    rng = np.random.default_rng(1306 + policy)
    sas = [GcmSA(rng), EtaSA(rng), GcmSA(rng, 32), EtaSA(rng, sha256=True), GcmSA(rng), EtaSA(rng)]
    tun = [False, False, True, True, False, True]
    natt = [True, True, True, True, False, False]                   # two plain SAs beside them
    delta = [0x1234, 0, 0x00ff, 0, 0x7777, 0]
    nsa = len(sas)
    outsa = np.zeros(nsa, dtype=OUTSA_DTYPE)
    enc = np.zeros(nsa, dtype=ENCSA_DTYPE)
    for k, s in enumerate(sas):
        outsa[k] = (100 * k, 5000 * k, s.spi, int.from_bytes(s.salt, "little"), L.OUT_PAD_SEQ, 0)
        enc["flags"][k] = (L.ENC_TUNNEL if tun[k] else 0) | (L.ENC_NATT if natt[k] else 0) | L.ENC_DF_COPY
        enc["ttl"][k] = 40 + k
        for f in ("src", "dst"):
            enc[f][k, :4] = np.frombuffer(EH.addr(rng, False), dtype=np.uint8)
        if natt[k]:
            enc["dst"][k, 4:8] = np.frombuffer(struct.pack(">HH", 3000 + k, PORT), dtype=np.uint8)
    enc["bytes"], enc["packets"] = 1000, 10
    n = 200
    sa = rng.integers(0, nsa, n)
    pkts, protos = [], []
    for k in sa:
        proto = int(rng.choice([6, 17, 1]))
        body = bytearray(rng.integers(0, 256, int(rng.integers(0, 300)), dtype=np.uint8).tobytes())
        if proto == 17 and len(body) >= 8:
            body[4:6] = struct.pack(">H", len(body))
        if tun[k] and rng.random() < 0.3:
            pkts.append(CH.ipv6(EH.addr(rng, True), body, nxt=proto))
        else:
            dst = EH.addr(rng, False) if tun[k] else enc["dst"][k, :4].tobytes()
            ihl = int(rng.integers(5, 16))
            pkts.append(CH.ipv4(dst, body, ihl=ihl, proto=proto,
                                opts=rng.integers(0, 256, ihl * 4 - 20, dtype=np.uint8).tobytes()))
        protos.append(proto)
    head, tail = 72, 49
    arena, rec = EH.layout(rng, pkts, head, tail)
    return sas, tun, natt, delta, outsa, enc, sa, pkts, protos, head, tail, arena, rec


def _back(place, a):
    """A structured array the device wrote, its off4 as at base 0."""
    if place is None:
        return a
    a = a.copy()
    a["off4"] = place.back(a["off4"])
    return a


@pytest.mark.gpu
@pytest.mark.parametrize("policy", [0, 1], ids=["auto", "recompute"])
def test_outbound_then_inbound_end_to_end_with_natt(policy):
    """Cleartext packets -> encap(NATT) -> frame -> encrypt -> merges -> sent,
    then d_opkt through classify(port) -> check -> decrypt_trailer -> update ->
    merges -> decap -> natt_cksum, on GCM and CBC+HMAC SAs in transport and
    tunnel mode: the results are the packets that went in, with the checksum
    esp.udp_ipsec_adjust_cksum predicts for the transport ones."""
    end_to_end(policy)


def end_to_end(policy, placed=None):
    """The loop with its arena at base 0 of a tensor of its own, or (placed: a
    function from the arena and the packet list to a
    high_offset_helpers.Placed) at a high offset of a large one: only the
    cleartext packet list is relocated by the test; every later offset is the
    device's own and is compared after subtracting base / 4."""
    torch = _torch()
    from espgpu import _lib as L
    from espgpu import esp as E
    from espgpu.batch import (ENCSA_DTYPE, INSA_DTYPE, PKT_DTYPE, REPLAY_DTYPE, SAD_DTYPE,
                              decrypt_batch, encrypt_batch, esp_classify, esp_decap, esp_encap, esp_frame,
                              esp_natt_cksum, esp_sent, replay_check, replay_merge, replay_update, sad_build)
    from espgpu.opencrypto import GpuCryptoDriver
    sas, tun, natt, delta, outsa, enc, sa, pkts, protos, head, tail, arena, rec = end_to_end_packets(policy)
    nsa, n = len(sas), len(pkts)
    drv = GpuCryptoDriver(max_sessions=16, batch_records=1024, batch_bytes=1 << 20, nbatches=1)
    place = None
    try:
        for k, s in enumerate(sas):
            rc, sid = drv.newsession(s.esp_sa().csp())
            assert rc == 0 and sid == k
        place = placed(arena, rec) if placed else None
        if place is None:
            d_arena = win = _up(torch, arena)
            d_rec = _up(torch, rec)
        else:
            d_arena, win = place.load(arena)                 # win: the layout's bytes inside d_arena
            d_rec = _up(torch, place.relocate(rec))
        d_sa = torch.from_numpy(sa.astype(np.uint16).view(np.int16).copy()).cuda()
        d_enc, d_outsa = _up(torch, enc), _up(torch, outsa)
        mk = lambda: torch.zeros(n, dtype=torch.uint8, device="cuda")        # noqa: E731
        est, fst, st = mk(), mk(), torch.full((n,), 0x55, dtype=torch.uint8, device="cuda")
        d_desc = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
        d_frame = torch.zeros(n, dtype=torch.int32, device="cuda")
        d_opkt = torch.zeros(n * 8, dtype=torch.uint8, device="cuda")
        esp_encap(drv, d_arena, d_rec, d_sa, n, d_enc, d_outsa, head, tail, 7, d_desc, d_frame, d_opkt, est)
        esp_frame(drv, d_arena, d_desc, d_frame, n, d_outsa, fst)
        encrypt_batch(drv, d_arena, d_desc, n, st)
        replay_merge(drv, st, fst, n)
        replay_merge(drv, st, est, n)
        esp_sent(drv, d_opkt, d_desc, st, n, d_enc)
        torch.cuda.synchronize()
        assert not st.cpu().numpy().any(), (est.cpu().numpy(), fst.cpu().numpy(), st.cpu().numpy())
        wire = win.cpu().numpy()
        opkt = _back(place, d_opkt.cpu().numpy().view(PKT_DTYPE))
        desc = _back(place, d_desc.cpu().numpy().view(DESC))
        g_enc = d_enc.cpu().numpy().view(ENCSA_DTYPE)
        for k in range(nsa):
            m = sa == k
            assert m.sum() > 10 and g_enc["packets"][k] == 10 + m.sum()
            assert g_enc["bytes"][k] == 1000 + int(opkt["len"][m].sum()) - (8 * int(m.sum()) if natt[k] else 0)
        for i, k in enumerate(sa):                           # on the wire: IP, UDP to the port, a record the oracle opens
            w0 = int(opkt["off4"][i]) * 4
            hl = (int(wire[w0]) & 0xf) * 4
            assert E.in_cksum(wire[w0:w0 + hl].tobytes()) == 0 and wire[w0 + 9] == (17 if natt[k] else 50)
            o, ln = int(desc["off4"][i]) * 4, int(desc["len"][i])
            if natt[k]:
                assert struct.unpack(">HHHH", wire[w0 + hl:w0 + hl + 8].tobytes()) == (
                    3000 + k, PORT, int(opkt["len"][i]) - hl, 0) and o == w0 + hl + 8
            rc, pt = sas[k].oracle.esp_decrypt(wire[o:o + ln].tobytes(), 0)
            assert rc == 0
        # inbound: d_opkt as it stands is the received-packet list
        ent = np.zeros(nsa, dtype=SAD_DTYPE)
        for k, s in enumerate(sas):
            ent["spi"][k], ent["sa"][k], ent["proto"][k], ent["af"][k] = s.spi, k, 50, 4
            ent["salt"][k] = int.from_bytes(s.salt, "little")
            ent["dst"][k] = enc["dst"][k]
            ent["flags"][k] = L.SAD_NATT if natt[k] else 0
        d_sad = _up(torch, sad_build(ent, 16))
        tab = np.zeros(nsa, dtype=REPLAY_DTYPE)
        for k in range(nsa):
            tab[k] = (outsa["count"][k], 64, 32, 32 * k, 0)
        d_tab, d_words = _up(torch, tab), torch.zeros(32 * nsa, dtype=torch.int32, device="cuda")
        insa = np.zeros(nsa, dtype=INSA_DTYPE)
        insa["flags"] = [(L.IN_TUNNEL if t else L.IN_TRANSPORT) | (L.IN_NATT if x else 0) for t, x in zip(tun, natt)]
        insa["pad_"] = delta
        d_in = _up(torch, insa)
        cst, rst, ust, ist, dst, cf = mk(), mk(), mk(), mk(), mk(), mk()
        tr = torch.zeros(n, dtype=torch.int32, device="cuda")
        d_idesc = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
        d_ipkt = torch.zeros(n * 8, dtype=torch.uint8, device="cuda")
        esp_classify(drv, d_arena, d_opkt, n, d_sad, d_idesc, cst, flags=L.CLS_IPCSUM | L.CLS_NATT_PORT(PORT))
        replay_check(drv, d_arena, d_idesc, n, d_tab, d_words, rst)
        decrypt_batch(drv, d_arena, d_idesc, n, ist, trailer=tr)
        replay_update(drv, d_arena, d_idesc, n, ist, d_tab, d_words, ust)
        replay_merge(drv, ist, rst, n)
        replay_merge(drv, ist, ust, n)
        replay_merge(drv, ist, cst, n)
        esp_decap(drv, d_arena, d_arena, d_opkt, d_idesc, tr, ist, n, d_in, d_ipkt, dst)
        esp_natt_cksum(drv, d_arena, d_ipkt, d_idesc, tr, ist, dst, n, d_in, policy=policy, cflags=cf)
        replay_merge(drv, ist, dst, n)
        torch.cuda.synchronize()
        assert not ist.cpu().numpy().any(), (cst.cpu().numpy(), rst.cpu().numpy(), ist.cpu().numpy(), dst.cpu().numpy())
        idesc = _back(place, d_idesc.cpu().numpy().view(DESC))
        for fld in ("off4", "len", "sa"):
            assert np.array_equal(idesc[fld], desc[fld]), fld
        out, ipkt, g_cf = win.cpu().numpy(), _back(place, d_ipkt.cpu().numpy().view(PKT_DTYPE)), cf.cpu().numpy()
        fixed = valid = 0
        for i, p in enumerate(pkts):
            k = sa[i]
            want, v = p, False
            if natt[k] and not tun[k] and protos[i] in (6, 17):
                want, v = E.udp_ipsec_adjust_cksum(p, delta[k], protos[i], (p[0] & 0xf) * 4, policy)
            o = int(ipkt["off4"][i]) * 4
            assert int(ipkt["len"][i]) == len(p) and out[o:o + len(p)].tobytes() == want, (i, int(k), protos[i])
            assert o == int(rec["off4"][i]) * 4 and g_cf[i] == (L.NATT_CSUM_VALID if v else 0)
            fixed += want != p
            valid += v
        assert fixed > 10 and (policy or valid > 1)              # (about 30 and 10 of 200 are expected)
        g_in = d_in.cpu().numpy().view(INSA_DTYPE)
        for k in range(nsa):
            assert g_in["packets"][k] == (sa == k).sum() and g_in["bytes"][k] == sum(len(pkts[i]) for i in
                                                                                   np.flatnonzero(sa == k))
            assert g_in["pad_"][k] == delta[k]
    finally:
        drv.close()
        if place is not None:
            place.finish()
