"""Inbound AH on the device-resident batch path (classify.hip with
ESPGPU_CLS_AH, replay.hip with ESPGPU_REPLAY_AH, ah_in.hip): every test
compares the device batch with the host rules (pinned against ah.py's
restatements of the reference in test_ah_in.py) applied in index order: the
whole arena with the random bytes between the packets, every output array with
guard entries past n, d_hsave, the SA tables, and the inputs unchanged.  The
whole sequence is also compared with the restatement itself, HMAC by hashlib."""
import hmac as pyhmac
import struct

import numpy as np
import pytest

import ah_in_helpers as H
import classify_helpers as CH
import natt_helpers as NH
from ah_helpers import AhSA
from helpers import DESC, GcmSA
from espgpu import _lib as L
from espgpu import ah as A
from espgpu import esp as E

EINVAL, EACCES, EBADMSG, EMSGSIZE, ENOTSUP, ENOENT, EPFNOSUPPORT = 22, 13, 74, 90, 95, 2, 96
SLOT = H.SLOT
GUARD = 5
NAH = 40                    # sessions 0 .. NAH - 1 are AH SAs: sha cycles 1, 256, 384, 512
ESP0, NESP = 40, 4          # then four ESP (GCM) sessions
FREED = 44                  # and a slot freed again
BADFLAGS, NATTFLAGS = 38, 39    # AH sessions whose espgpu_insa lacks ESPGPU_IN_AH / carries ESPGPU_IN_NATT
SHAS = (1, 256, 384, 512)
EDGES = [1, 63, 64, 65, 255, 256, 257, 1025]


def _torch():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.fail("GPU test run without a visible HIP device")
    return torch


def _up(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()


class Env:
    def __init__(self):
        from espgpu.opencrypto import GpuCryptoDriver
        rng = np.random.default_rng(6101)
        self.drv = GpuCryptoDriver(max_sessions=64, batch_records=1024, batch_bytes=1 << 20, nbatches=1)
        self.sas, self.mlens, self.esp = [], [], []
        for k in range(FREED + 1):
            if k < NAH or k == FREED:
                sa = AhSA(rng, SHAS[k % 4], esn=bool(k // 4 & 1))
                csp, mlen, esp = sa.csp(), sa.mlen, False
            else:
                sa = GcmSA(rng)
                csp, mlen, esp = sa.esp_sa().csp(), None, True
            rc, sid = self.drv.newsession(csp)
            assert rc == 0 and sid == k, (rc, sid, k)
            self.sas.append(sa)
            self.mlens.append(mlen)
            self.esp.append(esp)
        self.drv.freesession(FREED)
        self.mlens[FREED] = None
        assert sorted(set(m for m in self.mlens if m)) == [12, 16, 24, 32]


@pytest.fixture(scope="module")
def env():
    _torch()
    e = Env()
    yield e
    e.drv.close()
    import gc
    gc.collect()


def _af6(k):
    return k % 5 in (1, 3)


def _insa(rng, nin=FREED + 3):
    """Every mode, both families, KEEPTOS here and there; two unusable AH SAs."""
    from espgpu.batch import INSA_DTYPE
    t = np.zeros(nin, dtype=INSA_DTYPE)
    t["bytes"] = rng.integers(0, 2**40, nin)
    t["packets"] = rng.integers(0, 2**20, nin)
    for k in range(nin):
        t["flags"][k] = H.ah_flags(k % 3, _af6(k), k % 7 == 0) if k < NAH else (k % 3) | (8 if k & 1 else 0)
    t["flags"][BADFLAGS] &= 0xffffffff ^ L.IN_AH
    t["flags"][NATTFLAGS] |= L.IN_NATT
    t["pad_"] = 0x0badf00d
    return t


KINDS = ("ok", "ok", "ok", "ok", "badopt", "badlen", "short", "jumbo", "wrongfam", "badflags", "natflags", "esp",
         "len0", "bigsa", "nosess", "nosa", "cut")


def _one(rng, env, kind, sa, opts_ok=True, nxt=None, q=None, min_ihl=5):
    """One record of `kind` for AH SA `sa`: (packet bytes, (len, sa, salt),
    skip).  opts_ok False: IPv4 headers have no options."""
    af6 = _af6(sa)
    mlen = env.mlens[sa]
    nxt = int(rng.choice([4, 41, 6, 17, 50])) if nxt is None else nxt
    q = int(rng.choice([0, 19, 20, 39, 40, int(rng.integers(0, 200))])) if q is None else q
    kw = {}
    if kind == "badlen":
        kw["ah_len"] = (A.ah_hdrsiz(mlen, af6) - 8) // 4 + int(rng.choice([-1, 1]))
    if kind == "short":
        kw["cut"] = q + 1
    if af6:
        if kind == "jumbo":
            kw["plen"] = 0
        p, skip = H.ah_packet6(rng, nxt, mlen, q, seq=int(rng.integers(1, 2**32)), **kw)
        if rng.random() < 0.3:                             # a link-local source
            p = p[:8] + b"\xfe\x80" + p[10:]
    else:
        ihl = int(rng.integers(min_ihl, 16)) if opts_ok else 5
        if kind == "badopt":
            ihl = max(ihl, 6)
            opts = H.bad_options(rng, ihl * 4 - 20, str(rng.choice(["lone", "len0", "len1", "past"])))
        else:
            opts = H.good_options(rng, ihl * 4 - 20)
        p, skip = H.ah_packet4(rng, ihl, opts, nxt, mlen, q, seq=int(rng.integers(1, 2**32)), **kw)
    ln = len(p)
    if kind == "cut":                                      # the descriptor ends inside struct newah
        ln = skip + int(rng.integers(0, 12))
    return p, (ln, sa, skip + 12), skip


def _pool(rng, env, n, insa, sas=None, kinds=KINDS, opts="all"):
    """n records: (arena, DESC desc, kinds).  opts: "all" any ip_hl, "none" no
    IPv4 options anywhere, "one" only lane 17 of every wave has options."""
    pkts, meta, names = [], [], []
    good = [k for k in range(NAH) if k not in (BADFLAGS, NATTFLAGS)]
    for i in range(n):
        kind = kinds[int(rng.integers(len(kinds)))]
        sa = int(rng.choice(good if sas is None else sas))
        opts_ok = opts == "all" or (opts == "one" and i % 64 == 17)
        if opts == "one" and i % 64 == 17:
            sa = next(k for k in range(sa, sa + NAH) if not _af6(k % NAH) and k % NAH in good) % NAH
            kind = "ok" if i & 64 else "badopt"
        if kind == "badopt" and (_af6(sa) or not opts_ok):
            kind = "ok"
        if kind == "jumbo" and not _af6(sa):
            kind = "badlen"
        if kind == "wrongfam":                             # a packet of the other family than its SA's
            other = next(k for k in range(sa + 1, sa + NAH) if _af6(k % NAH) != _af6(sa) and k % NAH in good) % NAH
            p, (ln, _, salt), skip = _one(rng, env, "ok", other, opts_ok)
            m = (ln, sa, salt)                             # (an IPv4 header of ip_hl 10 has IPv6's skip)
        elif kind in ("badflags", "natflags"):
            sa = BADFLAGS if kind == "badflags" else NATTFLAGS
            p, m, skip = _one(rng, env, "ok", sa, opts_ok)
        elif kind == "esp":                                # an ESP record: descriptor past the IP header
            p, (ln, _, salt), skip = _one(rng, env, "ok", sa, opts_ok)
            m = (ln - skip, ESP0 + int(rng.integers(NESP)), 0xa5a5a5a5)
        else:
            p, m, skip = _one(rng, env, kind if kind in ("ok", "badopt", "badlen", "short", "jumbo", "cut") else "ok",
                              sa, opts_ok, min_ihl=6 if opts == "one" and opts_ok else 5)
            if kind == "len0":
                m = (0, m[1], m[2])
            elif kind == "bigsa":
                m = (m[0], len(insa) + int(rng.integers(0, 3)), m[2])
            elif kind == "nosess":
                m = (m[0], FREED, m[2])
            elif kind == "nosa":
                m = (m[0], 0xffff, m[2])
        pkts.append(p)
        meta.append((m, skip if kind == "esp" else 0))
        names.append(kind)
    arena, rec = H.layout(rng, pkts)
    desc = np.zeros(n, dtype=DESC)
    for i, ((ln, sa, salt), fwd) in enumerate(meta):
        desc[i] = (int(rec["off4"][i]) + fwd // 4, ln, sa, 0x5a5a5a5a, salt)
    return arena, desc, np.array(names)


def _run_input(env, arena, desc, insa, nin=None):
    """Upload, ah_input, download, compare everything with the host rule.
    Returns (arena, desc, hsave, astatus) as the device left them."""
    torch = _torch()
    from espgpu.batch import INSA_DTYPE, ah_input
    n = len(desc)
    nin = len(insa) if nin is None else nin
    rng = np.random.default_rng(n)
    hs0 = rng.integers(0, 256, (n + GUARD) * SLOT, dtype=np.uint8)
    dguard = np.zeros(GUARD, dtype=DESC)
    dguard.view(np.uint8)[:] = 0xC3
    d_arena, d_desc = _up(torch, arena), _up(torch, np.concatenate([desc, dguard]))
    d_in, d_hs = _up(torch, insa), _up(torch, hs0)
    d_ast = torch.full((n + GUARD,), 0x77, dtype=torch.uint8, device="cuda")
    ah_input(env.drv, d_arena, d_desc, n, d_in[:nin * INSA_DTYPE.itemsize], d_hs, d_ast)
    torch.cuda.synchronize()
    w_arena, w_desc, w_hs, w_ast = H.host_ah_input_batch(arena, desc, insa[:nin], env.mlens, hs0)
    g_ast, g_desc = d_ast.cpu().numpy(), d_desc.cpu().numpy().view(DESC)
    bad = np.flatnonzero(g_ast[:n] != w_ast)
    assert bad.size == 0, ("astatus", bad[:8], g_ast[bad[:8]], w_ast[bad[:8]], desc[bad[:8]])
    assert (g_ast[n:] == 0x77).all() and np.array_equal(g_desc[n:], dguard), "wrote past n"
    bad = np.flatnonzero(g_desc[:n] != w_desc)
    assert bad.size == 0, ("desc", bad[:8], g_desc[bad[:8]], w_desc[bad[:8]])
    g_arena, g_hs = d_arena.cpu().numpy(), d_hs.cpu().numpy()
    bad = np.flatnonzero(g_arena != w_arena)
    assert bad.size == 0, ("arena", bad[:16], g_arena[bad[:16]], w_arena[bad[:16]])
    bad = np.flatnonzero(g_hs != w_hs)
    assert bad.size == 0, ("hsave", bad[:16] // SLOT, bad[:16] % SLOT)
    assert np.array_equal(d_in.cpu().numpy(), insa.view(np.uint8)), "the SA table was written"
    return g_arena, g_desc[:n], g_hs[:n * SLOT], g_ast[:n]


def _run_decap(env, arena, desc, status, insa, hsave, nin=None):
    """Upload, ah_decap, download, compare everything with the host rule.
    Returns (arena, ipkt, dstatus, insa) as the device left them."""
    torch = _torch()
    from espgpu.batch import INSA_DTYPE, PKT_DTYPE, ah_decap
    n = len(desc)
    nin = len(insa) if nin is None else nin
    iguard = np.zeros(3, dtype=INSA_DTYPE)
    iguard.view(np.uint8)[:] = 0xC3
    ipkt0 = np.zeros(n + GUARD, dtype=PKT_DTYPE)
    ipkt0.view(np.uint8)[:] = 0xC3
    hs = np.concatenate([hsave, np.full(GUARD * SLOT, 0x3C, dtype=np.uint8)])
    d_arena, d_desc, d_st = _up(torch, arena), _up(torch, desc), _up(torch, status)
    d_in, d_hs, d_ipkt = _up(torch, np.concatenate([insa[:nin], iguard])), _up(torch, hs), _up(torch, ipkt0)
    d_dst = torch.full((n + GUARD,), 0x77, dtype=torch.uint8, device="cuda")
    ah_decap(env.drv, d_arena, d_desc, d_st, n, d_in[:nin * INSA_DTYPE.itemsize], d_hs, d_ipkt, d_dst)
    torch.cuda.synchronize()
    w_arena, w_ipkt, w_dst, w_in = H.host_ah_decap_batch(arena, desc, status, insa[:nin], env.mlens, env.esp, hsave,
                                                         ipkt0[:n])
    g_dst, g_ipkt = d_dst.cpu().numpy(), d_ipkt.cpu().numpy().view(PKT_DTYPE)
    g_in = d_in.cpu().numpy().view(INSA_DTYPE)
    bad = np.flatnonzero(g_dst[:n] != w_dst)
    assert bad.size == 0, ("dstatus", bad[:8], g_dst[bad[:8]], w_dst[bad[:8]], desc[bad[:8]])
    bad = np.flatnonzero(g_ipkt[:n] != w_ipkt)
    assert bad.size == 0, ("ipkt", bad[:8], g_ipkt[bad[:8]], w_ipkt[bad[:8]])
    assert (g_dst[n:] == 0x77).all() and np.array_equal(g_ipkt[n:], ipkt0[n:]), "wrote past n"
    for fld in ("bytes", "packets", "flags", "pad_"):
        bad = np.flatnonzero(g_in[fld][:nin] != w_in[fld])
        assert bad.size == 0, ("insa." + fld, bad[:8], g_in[fld][bad[:8]], w_in[fld][bad[:8]])
    assert np.array_equal(g_in[nin:].view(np.uint8), iguard.view(np.uint8)), "insa guard entries written"
    g_arena = d_arena.cpu().numpy()
    bad = np.flatnonzero(g_arena != w_arena)
    assert bad.size == 0, ("arena", bad[:16], g_arena[bad[:16]], w_arena[bad[:16]])
    assert np.array_equal(d_hs.cpu().numpy(), hs), "d_hsave modified"
    assert np.array_equal(d_desc.cpu().numpy(), desc.view(np.uint8)), "d_desc modified"
    assert np.array_equal(d_st.cpu().numpy(), status), "d_status modified"
    return g_arena, g_ipkt[:n], g_dst[:n], g_in[:nin]


# ---- (a) classification ---------------------------------------------------------
@pytest.mark.gpu
def test_classify_mixed_batch_with_and_without_the_flag(env):
    torch = _torch()
    from espgpu.batch import esp_classify, sad_build
    rng = np.random.default_rng(6102)
    db = NH.NattSadb(rng, nesp4=12, nesp6=8, nah=12)
    table = sad_build(db.entries, 128)
    pkts, kinds = [], []
    for kind, p in CH.random_packets(rng, db, 900):
        pkts.append(p)
        kinds.append("esp:" + kind)
    for _ in range(300):
        kind = str(rng.choice(list(NH.NATT_KINDS)))
        pkts.append(NH.natt_packet(rng, db, NH.PORT, kind))
        kinds.append("natt:" + kind)
    for _ in range(800):
        e = db.pick(rng, proto=51)
        kind = str(rng.choice(["good", "good", "good", "short11", "unknown", "espspi", "frag", "wrongdst"]))
        if kind == "frag" and e["af"] == 6:
            kind = "good"
        spi = int(e["spi"])
        if kind == "unknown":
            spi = db.unknown_spi(rng)
        if kind == "espspi":
            spi = int(db.pick(rng, proto=50, af=int(e["af"]))["spi"])
        n = 11 if kind == "short11" else int(rng.integers(12, 120))
        body = (bytes([6, 4, 0, 0]) + struct.pack(">II", spi, 7) + rng.integers(0, 256, 120, dtype=np.uint8).tobytes())[:n]
        dst = bytearray(CH.dst_of(e))
        if kind == "wrongdst":
            dst[3] ^= 4
        if e["af"] == 4:
            ihl = int(rng.integers(5, 16))
            p = CH.ipv4(dst, body, ihl=ihl, proto=51, off=0x2000 if kind == "frag" else 0,
                        opts=H.good_options(rng, ihl * 4 - 20))
        else:
            p = CH.ipv6(dst, body, nxt=51)
        pkts.append(p)
        kinds.append("ah:" + kind)
    order = rng.permutation(len(pkts))
    pkts, kinds = [pkts[i] for i in order], np.array(kinds)[order]
    n = len(pkts)
    arena, rec = CH.layout(rng, pkts)
    d_arena, d_rec, d_tab = _up(torch, arena), _up(torch, rec), _up(torch, table)
    # by the protocol field: a few of the ESP kinds carry ip_p / ip6_nxt 51 as their "other protocol"
    isah = np.array([len(p) >= 20 and ((p[0] >> 4 == 4 and p[9] == 51) or (p[0] >> 4 == 6 and len(p) >= 40 and p[6] == 51))
                     for p in pkts])
    assert isah[np.char.startswith(kinds, "ah:")].all()
    results = {}
    for flags in (L.CLS_NATT_PORT(NH.PORT) | L.CLS_IPCSUM, L.CLS_NATT_PORT(NH.PORT) | L.CLS_IPCSUM | L.CLS_AH, L.CLS_AH):
        d_desc = torch.full(((n + GUARD) * 16,), 0xC3, dtype=torch.uint8, device="cuda")
        d_cst = torch.full((n + GUARD,), 0x77, dtype=torch.uint8, device="cuda")
        esp_classify(env.drv, d_arena, d_rec, n, d_tab, d_desc, d_cst, flags=flags)
        torch.cuda.synchronize()
        w_desc, w_cst = CH.host_classify_batch(table, arena, rec, flags)
        g_desc, g_cst = d_desc.cpu().numpy(), d_cst.cpu().numpy()
        bad = np.flatnonzero(g_cst[:n] != w_cst)
        assert bad.size == 0, (flags, bad[:8], g_cst[bad[:8]], w_cst[bad[:8]], kinds[bad[:8]])
        assert np.array_equal(g_desc[:n * 16].view(DESC), w_desc)
        assert (g_desc[n * 16:] == 0xC3).all() and (g_cst[n:] == 0x77).all()
        assert np.array_equal(d_arena.cpu().numpy(), arena) and np.array_equal(d_rec.cpu().numpy(), rec.view(np.uint8))
        results[flags] = (w_cst, w_desc)
    off, on, _ = results.values()
    assert (off[0][isah] == ENOTSUP).sum() > 600           # without the flag: the host stack's (a fragment is either way)
    assert not (off[0][isah] == 0).any()
    assert np.array_equal(off[0][~isah], on[0][~isah]) and np.array_equal(off[1][~isah], on[1][~isah])
    for kind, st in (("good", 0), ("short11", EINVAL), ("unknown", ENOENT), ("espspi", ENOENT), ("frag", ENOTSUP),
                     ("wrongdst", ENOENT)):
        m = kinds == "ah:" + kind
        assert m.sum() > 20 and (on[0][m] == st).all(), kind
    good = kinds == "ah:good"
    assert np.array_equal(on[1]["off4"][good], rec["off4"][good]) and (on[1]["salt"][good] >= 32).all()
    assert (on[0][np.char.startswith(kinds, "natt:")] == 0).sum() > 20
    assert (on[0][np.char.startswith(kinds, "esp:")] == 0).sum() > 100


# ---- (b) espgpu_ah_input_batch -----------------------------------------------------
@pytest.fixture(scope="module")
def mixed(env):
    rng = np.random.default_rng(6103)
    insa = _insa(rng)
    arena, desc, kinds = _pool(rng, env, 1400, insa)
    return arena, desc, kinds, insa


def _has_all_classes(kinds, ast, desc0):
    assert {int(x) for x in np.unique(ast)} == {0, EINVAL, EACCES, EMSGSIZE}
    for kind, st in (("badopt", EINVAL), ("badlen", EACCES), ("short", EACCES), ("jumbo", EMSGSIZE),
                     ("wrongfam", EINVAL), ("badflags", EINVAL), ("natflags", EINVAL), ("cut", EINVAL)):
        m = kinds == kind
        assert m.sum() > 0 and (ast[m] == st).all(), (kind, ast[m][:8])
    for kind in ("esp", "len0", "bigsa", "nosess", "nosa"):
        m = kinds == kind
        assert m.sum() > 0 and not ast[m].any(), kind
    ok = kinds == "ok"
    assert not ast[ok].any()
    skips = set((desc0["salt"][ok] - 12).tolist())
    assert skips == set(range(20, 64, 4))                  # every ip_hl, and IPv6's 40 among them


@pytest.mark.gpu
def test_input_mixed_batch(env, mixed):
    arena, desc, kinds, insa = mixed
    g_arena, g_desc, g_hs, ast = _run_input(env, arena, desc, insa)
    _has_all_classes(kinds, ast, desc)
    assert (g_desc["len"][ast != 0] == 0).all()
    untouched = np.isin(kinds, ["esp", "len0", "bigsa", "nosess", "nosa"])
    assert np.array_equal(g_desc[untouched], desc[untouched])
    assert (g_arena != arena).sum() > 1000                 # headers were massaged


@pytest.mark.gpu
@pytest.mark.parametrize("n", EDGES)
def test_input_launch_edges(env, mixed, n):
    arena, desc, kinds, insa = mixed
    sl = slice(7, 7 + n)
    _run_input(env, arena, desc[sl], insa, nin=len(insa) if n & 1 else NAH - 4)


@pytest.mark.gpu
@pytest.mark.parametrize("opts", ["none", "one"])
def test_input_waves_without_options_and_with_one_lane_of_them(env, opts):
    """none: no wave runs the option loop.  one: in every wave only lane 17
    has IPv4 options, good ones in every second wave and refused ones in the
    others, and the other 63 lanes go through the loop's instantiation too."""
    rng = np.random.default_rng(6104 + len(opts))
    insa = _insa(rng)
    arena, desc, kinds = _pool(rng, env, 700, insa, opts=opts)
    _, g_desc, _, ast = _run_input(env, arena, desc, insa)
    ok = (ast == 0) & (kinds == "ok")
    long_hdr = (desc["salt"] > 32) & ~np.array([_af6(int(s)) if s < NAH else True for s in desc["sa"]])
    lane17 = np.arange(len(desc)) % 64 == 17
    if opts == "none":
        assert not (long_hdr & np.isin(kinds, ["ok", "badlen", "short", "cut"])).any() and ok.sum() > 100
    else:
        assert long_hdr[lane17].all() and not (long_hdr & ~lane17 & np.isin(kinds, ["ok", "badlen", "short"])).any()
        assert (ast[lane17 & (kinds == "badopt")] == EINVAL).all() and (kinds[lane17] == "badopt").sum() >= 5
        assert not ast[lane17 & (kinds == "ok")].any() and (kinds[lane17] == "ok").sum() >= 5


# ---- (c) espgpu_ah_decap_batch ------------------------------------------------------
def _after_input(env, arena, desc, insa, rng, fail=0.1):
    """The batch as the host rule's ah_input leaves it, and a status array as
    the merges of step 5 would: ah_input's refusals, a few failures of the
    later stages, zeros."""
    n = len(desc)
    hs0 = rng.integers(0, 256, n * SLOT, dtype=np.uint8)
    a2, d2, hs, ast = H.host_ah_input_batch(arena, desc, insa, env.mlens, hs0)
    status = ast.copy()
    bad = (rng.random(n) < fail) & (status == 0)
    status[bad] = rng.choice([EACCES, EBADMSG, EINVAL, ENOENT], int(bad.sum()))
    return a2, d2, hs, status


@pytest.fixture(scope="module")
def decap_pool(env, mixed):
    arena, desc, kinds, insa = mixed
    return _after_input(env, arena, desc, insa, np.random.default_rng(6105)) + (kinds, insa)


@pytest.mark.gpu
def test_decap_many_sas_interleaved(env, decap_pool):
    """Every wave holds records of many SAs: the per-wave loop books them."""
    from espgpu.batch import PKT_DTYPE
    arena, desc, hs, status, kinds, insa = decap_pool
    _, ipkt, dst, g_in = _run_decap(env, arena, desc, status, insa, hs)
    assert {int(x) for x in np.unique(dst)} == {0, EINVAL, EPFNOSUPPORT}
    took = (status == 0) & np.isin(kinds, ["ok"])
    ok = took & (dst == 0)
    assert 200 < ok.sum() < took.sum()
    ahsize = np.array([A.ah_hdrsiz(env.mlens[s], _af6(s)) if s < NAH else 0 for s in desc["sa"].tolist()])
    tunnel = ok & ((ipkt["off4"] - desc["off4"]) * 4 == desc["salt"] - 12 + ahsize)
    assert ((ipkt["off4"] - desc["off4"])[ok & ~tunnel] * 4 == ahsize[ok & ~tunnel]).all()
    assert 30 < tunnel.sum() < ok.sum() - 30
    esp = (kinds == "esp") & (status == 0)
    assert esp.sum() > 10 and not dst[esp].any()
    assert (ipkt[esp].view(np.uint8) == 0xC3).all()        # espgpu_esp_decap_batch's entries stay
    for kind in ("len0", "bigsa", "nosess", "nosa"):
        m = (kinds == kind) & (status == 0)
        assert m.sum() > 0 and (dst[m] == EINVAL).all(), kind
    assert (dst[status != 0] == 0).all() and (ipkt["len"][status != 0] == 0).all()
    assert int((g_in["packets"] - insa["packets"]).sum()) == int(ok.sum())
    assert int((g_in["bytes"] - insa["bytes"]).sum()) == int(ipkt["len"][ok].sum())
    assert len(np.flatnonzero(g_in["packets"] != insa["packets"])) >= 30


@pytest.mark.gpu
@pytest.mark.parametrize("n", EDGES)
def test_decap_launch_edges(env, decap_pool, n):
    arena, desc, hs, status, kinds, insa = decap_pool
    sl = slice(7, 7 + n)
    _run_decap(env, arena, desc[sl], status[sl], insa, hs[7 * SLOT:(7 + n) * SLOT], nin=len(insa) if n & 1 else NAH - 4)


@pytest.mark.gpu
@pytest.mark.parametrize("sa,n", [(0, 1025), (1, 700)], ids=["inet-wildcard", "inet6-transport"])
def test_decap_one_sa_for_the_whole_batch(env, sa, n):
    """Every record of one SA: whole workgroups add once (the workgroup sum),
    and bytes crosses 2^32."""
    rng = np.random.default_rng(6106 + sa)
    insa = _insa(rng)
    insa["bytes"][sa], insa["packets"][sa] = 2**32 - 1000, 2**32 - 3
    arena, desc, kinds = _pool(rng, env, n, insa, sas=[sa], kinds=("ok",))
    a2, d2, hs, status = _after_input(env, arena, desc, insa, rng, fail=0.03)
    _, ipkt, dst, g_in = _run_decap(env, a2, d2, status, insa, hs)
    ok = (status == 0) & (dst == 0)
    assert ok.sum() > n // 2
    assert g_in["packets"][sa] == 2**32 - 3 + ok.sum() and g_in["bytes"][sa] > 2**32
    others = np.arange(len(insa)) != sa
    assert np.array_equal(g_in["packets"][others], insa["packets"][others])


@pytest.mark.gpu
def test_zero_packets_and_arguments(env, mixed):
    torch = _torch()
    arena, desc, kinds, insa = mixed
    lib, ctx = env.drv.lib, env.drv.ctx
    d_arena, d_desc, d_in = _up(torch, arena[:8192]), _up(torch, desc[:4]), _up(torch, insa)
    d_hs = torch.zeros(4 * SLOT + 4, dtype=torch.uint8, device="cuda")
    d_st = torch.zeros(4, dtype=torch.uint8, device="cuda")
    d_ipkt = torch.zeros(32, dtype=torch.uint8, device="cuda")
    d_out = torch.zeros(4, dtype=torch.uint8, device="cuda")
    assert lib.espgpu_ah_input_batch(ctx, None, None, 0, None, 0, None, None, None) == 0
    assert lib.espgpu_ah_decap_batch(ctx, None, None, None, 0, None, 0, None, None, None, None) == 0
    iargs = [d_arena.data_ptr(), d_desc.data_ptr(), 4, d_in.data_ptr(), len(insa), d_hs.data_ptr(), d_out.data_ptr(), None]
    dargs = [d_arena.data_ptr(), d_desc.data_ptr(), d_st.data_ptr(), 4, d_in.data_ptr(), len(insa), d_hs.data_ptr(),
             d_ipkt.data_ptr(), d_out.data_ptr(), None]
    assert lib.espgpu_ah_input_batch(None, *iargs) == EINVAL and lib.espgpu_ah_decap_batch(None, *dargs) == EINVAL
    for k, v in ((0, None), (1, None), (3, None), (5, None), (6, None), (0, d_arena.data_ptr() + 2),
                 (5, d_hs.data_ptr() + 1)):
        a = list(iargs)
        a[k] = v
        assert lib.espgpu_ah_input_batch(ctx, *a) == EINVAL, (k, v)
    for k, v in ((0, None), (1, None), (2, None), (4, None), (6, None), (7, None), (8, None),
                 (0, d_arena.data_ptr() + 1), (6, d_hs.data_ptr() + 2)):
        a = list(dargs)
        a[k] = v
        assert lib.espgpu_ah_decap_batch(ctx, *a) == EINVAL, (k, v)
    torch.cuda.synchronize()
    assert np.array_equal(d_arena.cpu().numpy(), arena[:8192]) and not d_hs.cpu().numpy().any()
    assert lib.espgpu_health(ctx) == 0


# ---- (d), (e) the whole sequence -----------------------------------------------------
NCH = 10                    # AH SAs of the chain: SHA-1 / SHA2-256 / -384 / -512, ESN and not, both families
WSIZE, WWORDS = 64, 32      # a 512-packet window; key_setsaval's bitmap for it


def _chain_setup(env):
    """The SAs, their SAD, windows and packets for two batches."""
    import oracle as O
    from espgpu.batch import REPLAY_DTYPE, SAD_DTYPE, sad_build
    rng = np.random.default_rng(6110)
    # SA k is session k: sha SHAS[k % 4], ESN if k // 4 & 1, family _af6(k)
    sas = list(range(NCH))
    assert {(SHAS[k % 4], bool(k // 4 & 1)) for k in sas} == {(s, e) for s in SHAS for e in (False, True)}
    assert any(_af6(k) for k in sas) and not all(_af6(k) for k in sas)
    modes = [E.IPSEC_MODE_TRANSPORT, E.IPSEC_MODE_ANY, E.IPSEC_MODE_TUNNEL, E.IPSEC_MODE_TRANSPORT, E.IPSEC_MODE_ANY,
             E.IPSEC_MODE_TRANSPORT, E.IPSEC_MODE_TUNNEL, E.IPSEC_MODE_ANY, E.IPSEC_MODE_TRANSPORT, E.IPSEC_MODE_ANY]
    dsts = [bytes([0x20, 7, k, 1]) + (rng.integers(0, 256, 12, dtype=np.uint8).tobytes() if _af6(k) else b"")
            for k in sas]
    ent = np.zeros(NCH + 2, dtype=SAD_DTYPE)
    for k in sas:
        ent[k] = (env.sas[k].sa.spi, k, 51, 6 if _af6(k) else 4, 0x77777777, 0, list(dsts[k]) + [0] * (16 - len(dsts[k])))
    bundle = [k for k in sas if modes[k] == E.IPSEC_MODE_TRANSPORT and not _af6(k)]
    assert len(bundle) == 2
    for j, k in enumerate(bundle):                         # the ESP SAs inside these SAs' transport packets: one destination
        ent[NCH + j] = (env.sas[ESP0 + j].spi, ESP0 + j, 50, 4, 0xabcd0000 + j, 0, list(dsts[k]) + [0] * 12)
    table = sad_build(ent, 64)
    insa = _insa(rng)
    for k in sas:
        insa["flags"][k] = H.ah_flags(modes[k], _af6(k), k % 7 == 0)
    last0 = [(5 << 32 | 1000) if env.sas[k].esn else 1000 for k in sas]
    tab = np.zeros(FREED + 1, dtype=REPLAY_DTYPE)
    for k in sas:
        tab[k] = (last0[k], WSIZE, WWORDS, WWORDS * k, (L.REPLAY_ESN if env.sas[k].esn else 0) | L.REPLAY_AH)
    model = [O.Replay(WSIZE, last0[k], O.REPLAY_ESN if env.sas[k].esn else 0) for k in sas]
    for k in sas:
        assert len(model[k].bitmap) == WWORDS
    return rng, sas, modes, dsts, bundle, table, insa, tab, model


def _chain_packet(rng, env, k, dst, seq, esn_hi, modes, bundle, keeptos):
    """A signed AH packet of SA k with sequence number seq; the payload fits
    the SA's mode.  Returns bytes."""
    sa = env.sas[k]
    af6 = _af6(k)
    if modes[k] == E.IPSEC_MODE_TRANSPORT and not af6:     # AH transport around ESP
        nxt, body = 50, CH.esp_payload(rng, env.sas[ESP0 + bundle.index(k)].spi, 8 + 4 * int(rng.integers(2, 30)))
    elif modes[k] == E.IPSEC_MODE_TRANSPORT or (modes[k] == E.IPSEC_MODE_ANY and rng.random() < 0.5):
        nxt, body = int(rng.choice([6, 17])), rng.integers(0, 256, int(rng.integers(0, 200)), dtype=np.uint8).tobytes()
    else:
        nxt = int(rng.choice([4, 41]))
        inner = rng.integers(0, 256, int(rng.integers(40, 200)), dtype=np.uint8).tobytes()
        body = CH.ipv4(bytes([10, 1, 1, 1]), inner, proto=17) if nxt == 4 else CH.ipv6(bytes(range(16)), inner, nxt=17)
    if af6:
        p, skip = H.ah_packet6(rng, nxt, sa.mlen, 0, spi=sa.sa.spi, seq=seq, dst=dst)
    else:
        ihl = int(rng.integers(5, 16))
        p, skip = H.ah_packet4(rng, ihl, H.good_options(rng, ihl * 4 - 20), nxt, sa.mlen, 0, spi=sa.sa.spi, seq=seq,
                               dst=dst)
    p = bytearray(p + body)
    if af6:
        p[4:6] = struct.pack(">H", len(p) - 40)
    else:
        p[2:4] = struct.pack(">H", len(p))
        p[10:12] = b"\0\0"
        p[10:12] = struct.pack(">H", E.in_cksum(bytes(p[:skip])))
    return H.sign(bytes(p), skip, sa.mlen, sa.key, sa.sha, af6, esn_hi if sa.esn else None, not keeptos), skip


def _expected(env, pkts, insa, model, modes, table_ref):
    """The restatement, packet by packet in index order, against the windows
    as the batch finds them (the check) and as they move (the update).
    Returns (final status, resulting packet or None) per packet."""
    n = len(pkts)
    out = [None] * n
    st = np.zeros(n, dtype=np.uint8)
    checked = []
    for i, p in enumerate(pkts):                           # steps 0-2 see the windows as the batch found them
        cst, d = A.ipsec_input_classify_ah(table_ref, p, 0, True)
        if cst:
            st[i] = cst
            continue
        k = d[2]
        skip = d[4] - 12
        ast, massaged, saved = A.ah_input(_af6(k), env.mlens[k], p[:d[1]], skip, not insa["flags"][k] & L.IN_AH_KEEPTOS)
        if ast:
            st[i] = ast
            continue
        seq = struct.unpack(">I", p[skip + 8:skip + 12])[0]
        ok, seqh = model[k].check(seq)
        if not ok:
            st[i] = EACCES
            continue
        checked.append((i, k, skip, seq, seqh, massaged, saved))
    for i, k, skip, seq, seqh, massaged, saved in checked:  # steps 3-6 in arrival order
        sa = env.sas[k]
        m = bytearray(massaged)
        icv = bytes(m[skip + 12:skip + 12 + sa.mlen])
        m[skip + 12:skip + 12 + sa.mlen] = bytes(sa.mlen)
        msg = bytes(m) + (struct.pack(">I", seqh) if sa.esn else b"")
        if pyhmac.new(sa.key, msg, H.HASH[sa.sha]).digest()[:sa.mlen] != icv:
            st[i] = EBADMSG
            continue
        if not model[k].update(seq):
            st[i] = EACCES
            continue
        dst, res, _ = A.ah_input_cb_decap(modes[k], _af6(k), sa.mlen, massaged, saved, skip)
        st[i] = dst
        out[i] = res if dst == 0 else None
    return st, out


def _device_chain(env, arena, rec, d_sad, d_tab, d_words, d_in, ah_windows=True):
    """Steps 0-7 on one stream, no synchronisation in between.  Returns (final
    status, d_ipkt tensor, final arena, descriptors, hsave)."""
    torch = _torch()
    from espgpu.batch import (PKT_DTYPE, ah_decap, ah_input, decrypt_batch, esp_classify, replay_check, replay_merge,
                              replay_update)
    n = len(rec)
    drv = env.drv
    mk = lambda: torch.zeros(n, dtype=torch.uint8, device="cuda")
    cst, ast, rst, ust, st, dst = mk(), mk(), mk(), mk(), mk(), mk()
    tr = torch.zeros(n, dtype=torch.int32, device="cuda")
    d_arena, d_rec = _up(torch, arena), _up(torch, rec)
    d_desc = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
    d_ipkt = torch.zeros(n * 8, dtype=torch.uint8, device="cuda")
    d_hs = torch.zeros(n * SLOT, dtype=torch.uint8, device="cuda")
    esp_classify(drv, d_arena, d_rec, n, d_sad, d_desc, cst, flags=L.CLS_IPCSUM | L.CLS_AH)
    ah_input(drv, d_arena, d_desc, n, d_in, d_hs, ast)
    replay_check(drv, d_arena, d_desc, n, d_tab, d_words, rst)
    decrypt_batch(drv, d_arena, d_desc, n, st, trailer=tr)
    replay_update(drv, d_arena, d_desc, n, st, d_tab, d_words, ust)
    for r in (ast, rst, ust, cst):
        replay_merge(drv, st, r, n)
    ah_decap(drv, d_arena, d_desc, st, n, d_in, d_hs, d_ipkt, dst)
    replay_merge(drv, st, dst, n)
    torch.cuda.synchronize()
    return st.cpu().numpy(), d_ipkt, d_arena, d_desc.cpu().numpy().view(DESC), rst.cpu().numpy()


@pytest.fixture(scope="module")
def chain(env):
    """Two batches through the whole sequence with ESPGPU_REPLAY_AH windows,
    and the first batch again through windows without the flag."""
    torch = _torch()
    from espgpu.batch import INSA_DTYPE, PKT_DTYPE, REPLAY_DTYPE
    rng, sas, modes, dsts, bundle, table, insa, tab, model = _chain_setup(env)
    table_ref = {int(e["spi"]): (int(e["sa"]), int(e["proto"]), int(e["af"]), bytes(e["dst"]), int(e["salt"]))
                 for e in table if e["spi"]}
    d_sad = _up(torch, table)
    nxt_seq = [1001] * NCH
    batches = []
    for b, npk in enumerate((1000, 200)):
        pkts, kinds = [], []
        for i in range(npk):
            k = int(rng.integers(NCH))
            seq, esn_hi = nxt_seq[k], 5
            nxt_seq[k] += int(rng.choice([1, 1, 1, 2, 5]))
            p, skip = _chain_packet(rng, env, k, dsts[k], seq, esn_hi, modes, bundle, k % 7 == 0)
            kind = str(rng.choice(["good"] * 12 + ["icv", "ttl", "src", "dup", "old", "badopt"]))
            q = bytearray(p)
            if kind == "icv":
                q[skip + 12 + int(rng.integers(env.sas[k].mlen))] ^= 0x40
            elif kind == "ttl":                            # mutable: still verifies
                q[7 if _af6(k) else 8] ^= 0x1f
                if not _af6(k):
                    q[10:12] = b"\0\0"
                    q[10:12] = struct.pack(">H", E.in_cksum(bytes(q[:skip])))
            elif kind == "src":                            # immutable: must not verify
                q[9 if _af6(k) else 13] ^= 0x01
                if not _af6(k):
                    q[10:12] = b"\0\0"
                    q[10:12] = struct.pack(">H", E.in_cksum(bytes(q[:skip])))
            elif kind == "dup" and pkts:                   # a sequence number again inside the batch
                j = int(rng.integers(len(pkts)))
                q, kind = bytearray(pkts[j]), "dup" if kinds[j] == "good" else "other"
            elif kind == "old" and b == 1:                 # one from the previous batch
                j = int(rng.integers(len(batches[0][0])))
                q, kind = bytearray(batches[0][0][j]), "old" if batches[0][1][j] == "good" else "other"
            elif kind == "badopt":
                if _af6(k) or skip == 20:
                    kind = "good"
                else:
                    q[20:skip] = H.bad_options(rng, skip - 20, "len1")
                    q[10:12] = b"\0\0"
                    q[10:12] = struct.pack(">H", E.in_cksum(bytes(q[:skip])))
            elif kind in ("dup", "old"):
                kind = "good"
            pkts.append(bytes(q))
            kinds.append(kind)
        batches.append((pkts, np.array(kinds)))
    d_in = _up(torch, insa)
    res = []
    d_tab, d_words = _up(torch, tab), torch.zeros(WWORDS * (FREED + 1), dtype=torch.int32, device="cuda")
    for pkts, kinds in batches:
        arena, rec = H.layout(rng, pkts)
        want_st, want_pk = _expected(env, pkts, insa, model, modes, table_ref)
        st, d_ipkt, d_arena, desc, rst = _device_chain(env, arena, rec, d_sad, d_tab, d_words, d_in)
        res.append(dict(pkts=pkts, kinds=kinds, arena=arena, rec=rec, want_st=want_st, want_pk=want_pk, st=st,
                        d_ipkt=d_ipkt, d_arena=d_arena, desc=desc, rst=rst,
                        tab=d_tab.cpu().numpy().view(REPLAY_DTYPE), words=d_words.cpu().numpy().view(np.uint32),
                        last=[m.last for m in model], bitmaps=[m.bitmap.copy() for m in model]))
    # the control: the second batch through the windows as the first left them, without ESPGPU_REPLAY_AH
    ctl = res[0]["tab"].copy()
    ctl["flags"] &= 0xffffffff ^ L.REPLAY_AH
    d_ctab, d_cwords = _up(torch, ctl), torch.from_numpy(res[0]["words"].view(np.int32).copy()).cuda()
    d_cin = _up(torch, insa)
    c_st, _, _, _, c_rst = _device_chain(env, res[1]["arena"], res[1]["rec"], d_sad, d_ctab, d_cwords, d_cin)
    return dict(batches=res, control=(c_st, c_rst), insa=insa, d_in=d_in, d_sad=d_sad, table=table, modes=modes)


@pytest.mark.gpu
def test_whole_sequence_matches_the_restatement(env, chain):
    from espgpu.batch import INSA_DTYPE, PKT_DTYPE
    booked_p, booked_b = np.zeros(NCH, dtype=np.int64), np.zeros(NCH, dtype=np.int64)
    for b, r in enumerate(chain["batches"]):
        st, want, kinds = r["st"], r["want_st"], r["kinds"]
        bad = np.flatnonzero(st != want)
        assert bad.size == 0, (b, bad[:8], st[bad[:8]], want[bad[:8]], kinds[bad[:8]])
        # every class the test names is in the batch and ends as the reference would end it
        for kind, code in (("good", 0), ("ttl", 0), ("icv", EBADMSG), ("src", EBADMSG), ("dup", EACCES),
                           ("badopt", EINVAL)) + ((("old", EACCES),) if b == 1 else ()):
            m = kinds == kind
            assert m.sum() >= 3 and (st[m] == code).all(), (b, kind, m.sum(), st[m][:8])
        # windows: last and every bitmap word against the restated ipsec_updatereplay
        for k in range(NCH):
            assert int(r["tab"]["last"][k]) == r["last"][k], (b, k)
            assert np.array_equal(r["words"][WWORDS * k:WWORDS * (k + 1)], r["bitmaps"][k]), (b, k)
        assert not r["words"][WWORDS * NCH:].any()
        # resulting packets
        ipkt, arena = r["d_ipkt"].cpu().numpy().view(PKT_DTYPE), r["d_arena"].cpu().numpy()
        seen = set()
        for i in range(len(st)):
            if st[i]:
                assert ipkt["len"][i] == 0
                continue
            o = int(ipkt["off4"][i]) * 4
            got = arena[o:o + int(ipkt["len"][i])].tobytes()
            assert got == r["want_pk"][i], (b, i, kinds[i])
            k = int(r["desc"]["sa"][i])
            booked_p[k] += 1
            booked_b[k] += len(got)
            seen.add((env.sas[k].sha, env.sas[k].esn, _af6(k), got != r["pkts"][i][-len(got):]))
        assert len(seen) >= 12 if b == 0 else seen
    g_in = chain["d_in"].cpu().numpy().view(INSA_DTYPE)
    insa = chain["insa"]
    # (the control run has its own table)
    assert np.array_equal(g_in["packets"][:NCH] - insa["packets"][:NCH], booked_p)
    assert np.array_equal(g_in["bytes"][:NCH] - insa["bytes"][:NCH], booked_b)
    assert np.array_equal(g_in[NCH:], insa[NCH:])


@pytest.mark.gpu
def test_windows_without_the_flag_read_the_wrong_dword(env, chain):
    """The second batch through the windows the first one left, with and
    without ESPGPU_REPLAY_AH.  Without it the check reads byte 4 of the record,
    ip_id / ip_off or the IPv6 payload length and next header: a number far
    ahead of the window, so the packets replayed from the first batch pass
    the check, and the update then moves the window to wherever ip_id points
    and refuses fresh packets."""
    r = chain["batches"][1]
    c_st, c_rst = chain["control"]
    old, fresh = r["kinds"] == "old", r["kinds"] == "good"
    assert old.sum() >= 3 and (r["rst"][old] == EACCES).all() and not r["rst"][fresh].any()
    assert (c_rst[old] == 0).any()                         # the check decided a replayed record differently
    assert not r["st"][fresh].any() and (c_st[fresh] == EACCES).any()
    assert np.flatnonzero(c_st != r["st"]).size >= 1


@pytest.mark.gpu
def test_ah_transport_around_esp_goes_back_into_classification(env, chain):
    """d_ipkt of step 6 is the next round's d_pkt: the inner ESP packets get
    the descriptors the host gives for them."""
    torch = _torch()
    from espgpu.batch import PKT_DTYPE, esp_classify
    r = chain["batches"][0]
    n = len(r["st"])
    d_desc = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
    d_cst = torch.zeros(n, dtype=torch.uint8, device="cuda")
    esp_classify(env.drv, r["d_arena"], r["d_ipkt"], n, chain["d_sad"], d_desc, d_cst, flags=L.CLS_IPCSUM | L.CLS_AH)
    torch.cuda.synchronize()
    ipkt, arena = r["d_ipkt"].cpu().numpy().view(PKT_DTYPE), r["d_arena"].cpu().numpy()
    w_desc, w_cst = CH.host_classify_batch(chain["table"], arena, ipkt, L.CLS_IPCSUM | L.CLS_AH)
    g_desc, g_cst = d_desc.cpu().numpy().view(DESC), d_cst.cpu().numpy()
    assert np.array_equal(g_cst, w_cst) and np.array_equal(g_desc, w_desc)
    inner = np.flatnonzero(g_cst == 0)
    assert inner.size >= 50
    for i in inner:
        k = int(r["desc"]["sa"][i])
        assert chain["modes"][k] == E.IPSEC_MODE_TRANSPORT and not _af6(k) and r["st"][i] == 0
        want = r["want_pk"][i]
        st, d = E.ipsec_input_classify({int(e["spi"]): (int(e["sa"]), int(e["proto"]), int(e["af"]), bytes(e["dst"]),
                                                        int(e["salt"])) for e in chain["table"] if e["spi"]},
                                       want, int(ipkt["off4"][i]), True)
        assert st == 0 and tuple(g_desc[i]) == d and d[2] in (ESP0, ESP0 + 1)
    assert (g_cst[r["st"] != 0] == EINVAL).all()           # an empty d_ipkt entry: len 0
