"""Outbound AH on the device-resident batch path (ah_out.hip): every test
compares the device batch with the host rules (pinned against ah.py's
restatements of the reference in test_ah_out.py) applied in index order: the
whole arena with the random bytes in the headroom and between the packets,
d_hsave, every output array with guard entries past n, the SA tables, and the
inputs unchanged.  The whole sequence is also compared with the restatement
itself, HMAC by hashlib, sent through the inbound AH sequence, and run around
ESP as an SA bundle."""
import hmac as pyhmac
import struct

import numpy as np
import pytest

import ah_in_helpers as H
import ah_out_helpers as O
from ah_helpers import AhSA
from encap_helpers import addr
from helpers import DESC, GcmSA
from espgpu import _lib as L
from espgpu import ah as A
from espgpu import esp as E

EINVAL, EACCES, EBADMSG, EMSGSIZE, ENOTSUP, EAFNOSUPPORT, ENOBUFS = 22, 13, 74, 90, 95, 97, 105
SLOT = O.SLOT
GUARD = 5
NAH = 40                    # sessions 0 .. NAH - 1 are AH SAs: sha cycles 1, 256, 384, 512
ESP0, NESP = 40, 4          # then four ESP (GCM) sessions
FREED = 44                  # a slot freed again
NSES = 260                  # and AH SAs up to here, for the framing tables
WILD, LINKLOCAL, BADFLAGS, NATTFLAGS = 35, 36, 38, 39
SHAS = (1, 256, 384, 512)
EDGES = [1, 63, 64, 65, 255, 256, 257, 1025]
HEAD = 64                   # short of an IPv6 tunnel's ahsize + 40 unless the ICV has 12 bytes


def _torch():
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.fail("GPU test run without a visible HIP device")
    return torch


def _symbols():
    """The tests fail, not skip, on a build without the outbound AH block."""
    lib = L.lib()
    for name in ("espgpu_ah_encap_batch", "espgpu_ah_frame_batch", "espgpu_ah_sent_batch"):
        assert hasattr(lib, name), "libespgpu.so lacks " + name


def _up(torch, a):
    return torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).copy()).cuda()


class Env:
    def __init__(self):
        from espgpu.opencrypto import GpuCryptoDriver
        rng = np.random.default_rng(7201)
        self.drv = GpuCryptoDriver(max_sessions=NSES + 4, batch_records=1024, batch_bytes=1 << 20, nbatches=1)
        self.sas, self.mlens = [], []
        for k in range(NSES):
            if ESP0 <= k < ESP0 + NESP:
                sa = GcmSA(rng)
                csp, mlen = sa.esp_sa().csp(), None
            else:
                sa = AhSA(rng, SHAS[k % 4] if k < NAH else 256, esn=bool(k // 4 & 1))
                csp, mlen = sa.csp(), sa.mlen
            rc, sid = self.drv.newsession(csp)
            assert rc == 0 and sid == k, (rc, sid, k)
            self.sas.append(sa)
            self.mlens.append(mlen)
        self.drv.freesession(FREED)
        self.mlens[FREED] = None
        self.digest = [m is not None for m in self.mlens]
        assert sorted(set(m for m in self.mlens if m)) == [12, 16, 24, 32]


@pytest.fixture(scope="module")
def env():
    _torch()
    _symbols()
    e = Env()
    yield e
    e.drv.close()
    import gc
    gc.collect()


def _af6(k):
    return k % 5 in (1, 3)


def _enc_table(rng, nenc=FREED + 3):
    """AH SAs of every policy, mode and family; four unusable ones."""
    from espgpu.batch import ENCSA_DTYPE
    t = np.zeros(nenc, dtype=ENCSA_DTYPE)
    t["bytes"] = rng.integers(0, 2**40, nenc)
    t["packets"] = rng.integers(0, 2**20, nenc)
    t["ttl"] = rng.integers(1, 256, nenc)
    t["pad_"] = 0xa7
    for k in range(nenc):
        af6 = _af6(k)
        t["flags"][k] = O.ah_enc_flags(keeptos=k % 7 == 0, tunnel=bool(k & 2), af6=af6, dfbit=int(rng.integers(3)),
                                       ecn=int(rng.integers(-1, 2)), rfc6864=bool(k & 4))
        for f in ("src", "dst"):
            a = addr(rng, af6)
            t[f][k, :len(a)] = np.frombuffer(a, dtype=np.uint8)
    if nenc > NATTFLAGS:
        assert not _af6(WILD) and _af6(LINKLOCAL)
        t["dst"][WILD] = 0                                   # AF_INET wildcard: transport
        t["flags"][WILD] &= ~np.uint32(L.ENC_TUNNEL)
        t["dst"][LINKLOCAL, :2] = [0xfe, 0x80]
        t["flags"][BADFLAGS] &= ~np.uint32(L.ENC_AH)
        t["flags"][NATTFLAGS] |= L.ENC_NATT
    return t


KINDS = ("ok", "ok", "ok", "ok", "ok", "badopt", "shortsr", "sr", "badver", "short", "badihl", "wild", "linklocal",
         "badflags", "natflags", "esp", "nosess", "bigsa")


def _packet(rng, e, opts_ok=True, force_transport=False, kind="ok", min_ihl=5, consistent=True, plen=None,
            sr_ok=True):
    """A cleartext packet for the SA row e.  sr_ok False: no source-route
    option (a receiver could not verify the packet where it was sent from)."""
    saf6 = bool(e["flags"] & L.ENC_AF6)
    v6 = saf6 if force_transport or rng.random() < 0.75 else not saf6
    dst = None
    if force_transport or rng.random() < 0.7:
        dst = e["dst"][:16 if saf6 else 4].tobytes() if v6 == saf6 and e["dst"].any() else None
    plen = int(rng.choice([0, 1, 2, 3, 40, int(rng.integers(0, 200))])) if plen is None else plen
    if v6:
        src = bytes([0xfe, 0x80, 1, 2]) + addr(rng, True)[4:] if rng.random() < 0.2 else None
        return O.clear6(rng, plen, dst=dst, src=src, consistent=consistent)
    ihl = int(rng.integers(min_ihl, 16)) if opts_ok else 5
    room = ihl * 4 - 20
    if kind == "badopt":
        opts = H.bad_options(rng, room, str(rng.choice(["lone", "len0", "len1", "past"])))
    elif kind == "shortsr":
        ln = int(rng.choice([2, 3]))
        opts = bytes([1]) * (room - 4) + O.sr_option(rng, int(rng.choice([0x83, 0x89])), ln) + bytes([1]) * (4 - ln)
    elif kind == "sr":
        ln = int(rng.choice([x for x in (4, 7, 11) if x <= room]))
        opts = bytes([1]) * int(rng.integers(0, room - ln + 1)) + O.sr_option(rng, int(rng.choice([0x83, 0x89])), ln)
        opts += bytes([1]) * (room - len(opts))
    else:
        opts = O.good_options(rng, room, sr_ok)
    return O.clear4(rng, ihl, opts, plen, dst=dst, df=bool(rng.integers(2)), consistent=consistent)


def _pool(rng, env, n, enc, sas=None, kinds=KINDS, opts="all"):
    """n packets: (arena, PKT_DTYPE rec, sa ids, kinds).  opts: "all" any ip_hl,
    "none" no IPv4 options anywhere, "one" only lane 17 of every wave has
    options."""
    good = [k for k in range(NAH) if k not in (WILD, LINKLOCAL, BADFLAGS, NATTFLAGS)]
    v4tr = [k for k in good if not _af6(k) and not k & 2]              # AF_INET transport SAs
    pkts, ids, names = [], [], []
    for i in range(n):
        kind = kinds[int(rng.integers(len(kinds)))]
        sa = int(rng.choice(good if sas is None else sas))
        opts_ok = opts == "all" or (opts == "one" and i % 64 == 17)
        force = False
        if opts == "one" and i % 64 == 17:
            kind, force = ("ok", "badopt", "sr", "shortsr")[(i // 64) % 4], True
            sa = int(rng.choice(v4tr))
        if kind in ("badopt", "shortsr", "sr"):
            if not opts_ok:
                kind = "ok"
            else:
                sa, force = int(rng.choice(v4tr)), True
        if kind in ("wild", "linklocal", "badflags", "natflags") and sas is None:
            sa = {"wild": WILD, "linklocal": LINKLOCAL, "badflags": BADFLAGS, "natflags": NATTFLAGS}[kind]
            force = force or kind == "wild"
        if sas is None and opts == "all" and i % 257 == 100:
            kind, sa, force = "toobig", int(rng.choice(good)), False     # (a few: each is 64 KiB of arena)
        p = _packet(rng, enc[sa], opts_ok, force, kind, min_ihl=6 if force and kind != "wild" else 5,
                    plen=65500 if kind == "toobig" else None, consistent=kind != "toobig")
        if kind == "badver":
            p = bytes([int(rng.choice([0, 5, 7])) << 4 | 5]) + p[1:]
        elif kind == "short":
            p = p[:int(rng.integers(0, 20))]
        elif kind == "badihl":
            p = (bytes([0x44]) + p[1:]) if p[0] >> 4 == 4 and rng.random() < 0.5 else p[:(4 * (p[0] & 0xf) if p[0] >> 4 == 4 else 40) - 1]
        ids.append({"esp": ESP0 + int(rng.integers(NESP)), "nosess": FREED,
                    "bigsa": len(enc) + int(rng.integers(0, 3))}.get(kind, sa) if sas is None else sa)
        pkts.append(p)
        names.append(kind)
    arena, rec = O.layout(rng, pkts, HEAD)
    return arena, rec, np.array(ids, dtype=np.uint16), np.array(names)


def _run_encap(env, arena, rec, sa, enc, nenc=None, headroom=HEAD, id0=0xfff0):
    """Upload, ah_encap, download, compare everything with the host rule.
    Returns (arena, desc, opkt, estatus, hsave) as the device left them."""
    torch = _torch()
    from espgpu.batch import ENCSA_DTYPE, PKT_DTYPE, ah_encap
    n = len(rec)
    nenc = len(enc) if nenc is None else nenc
    rng = np.random.default_rng(n)
    hs0 = rng.integers(0, 256, (n + GUARD) * SLOT, dtype=np.uint8)
    d_arena, d_rec, d_enc, d_hs = _up(torch, arena), _up(torch, rec), _up(torch, enc), _up(torch, hs0)
    d_sa = torch.from_numpy(sa.view(np.int16).copy()).cuda()
    d_desc = torch.full(((n + GUARD) * 16,), 0xC3, dtype=torch.uint8, device="cuda")
    d_opkt = torch.full(((n + GUARD) * 8,), 0xC3, dtype=torch.uint8, device="cuda")
    d_est = torch.full((n + GUARD,), 0x77, dtype=torch.uint8, device="cuda")
    ah_encap(env.drv, d_arena, d_rec, d_sa, n, d_enc[:nenc * ENCSA_DTYPE.itemsize], headroom, id0, d_hs, d_desc,
             d_opkt, d_est)
    torch.cuda.synchronize()
    w_arena, w_desc, w_opkt, w_est, w_hs = O.host_encap_batch(arena, rec, sa, enc[:nenc], env.mlens, headroom, id0, hs0)
    g_est, g_desc = d_est.cpu().numpy(), d_desc.cpu().numpy()
    g_opkt = d_opkt.cpu().numpy()
    bad = np.flatnonzero(g_est[:n] != w_est)
    assert bad.size == 0, ("estatus", bad[:8], g_est[bad[:8]], w_est[bad[:8]], sa[bad[:8]])
    assert (g_est[n:] == 0x77).all() and (g_desc[n * 16:] == 0xC3).all() and (g_opkt[n * 8:] == 0xC3).all(), "past n"
    g_desc, g_opkt = g_desc[:n * 16].view(DESC), g_opkt[:n * 8].view(PKT_DTYPE)
    bad = np.flatnonzero(g_desc != w_desc)
    assert bad.size == 0, ("desc", bad[:8], g_desc[bad[:8]], w_desc[bad[:8]])
    assert np.array_equal(g_opkt, w_opkt)
    g_arena, g_hs = d_arena.cpu().numpy(), d_hs.cpu().numpy()
    bad = np.flatnonzero(g_arena != w_arena)
    assert bad.size == 0, ("arena", bad[:16], g_arena[bad[:16]], w_arena[bad[:16]])
    bad = np.flatnonzero(g_hs != w_hs)
    assert bad.size == 0, ("hsave", bad[:16] // SLOT, bad[:16] % SLOT)
    assert np.array_equal(d_enc.cpu().numpy(), enc.view(np.uint8)), "the SA table was written"
    assert np.array_equal(d_rec.cpu().numpy(), rec.view(np.uint8)) and np.array_equal(d_sa.cpu().numpy(), sa.view(np.int16))
    return g_arena, g_desc, g_opkt, g_est[:n], g_hs[:n * SLOT]


def _run_sent(env, arena, opkt, desc, status, enc, hsave, nenc=None):
    """Upload, ah_sent, download, compare everything with the host rule.
    Returns (arena, enc table, sstatus)."""
    torch = _torch()
    from espgpu.batch import ENCSA_DTYPE, ah_sent
    n = len(desc)
    nenc = len(enc) if nenc is None else nenc
    eguard = np.zeros(3, dtype=ENCSA_DTYPE)
    eguard.view(np.uint8)[:] = 0xC3
    d_arena, d_opkt, d_desc, d_st = _up(torch, arena), _up(torch, opkt), _up(torch, desc), _up(torch, status)
    d_enc, d_hs = _up(torch, np.concatenate([enc[:nenc], eguard])), _up(torch, hsave)
    d_sst = torch.full((n + GUARD,), 0x77, dtype=torch.uint8, device="cuda")
    ah_sent(env.drv, d_arena, d_opkt, d_desc, d_st, n, d_enc[:nenc * ENCSA_DTYPE.itemsize], d_hs, d_sst)
    torch.cuda.synchronize()
    w_arena, w_enc, w_sst = O.host_sent_batch(arena, opkt, desc, status, enc[:nenc], env.digest, hsave)
    g_sst, g_enc = d_sst.cpu().numpy(), d_enc.cpu().numpy().view(ENCSA_DTYPE)
    bad = np.flatnonzero(g_sst[:n] != w_sst)
    assert bad.size == 0, ("sstatus", bad[:8], g_sst[bad[:8]], w_sst[bad[:8]])
    assert (g_sst[n:] == 0x77).all(), "wrote past n"
    for fld in ("bytes", "packets", "flags", "ttl"):
        bad = np.flatnonzero(g_enc[fld][:nenc] != w_enc[fld])
        assert bad.size == 0, ("encsa." + fld, bad[:8], g_enc[fld][bad[:8]], w_enc[fld][bad[:8]])
    assert np.array_equal(g_enc[:nenc].view(np.uint8), w_enc.view(np.uint8))
    assert np.array_equal(g_enc[nenc:].view(np.uint8), eguard.view(np.uint8)), "encsa guard entries written"
    g_arena = d_arena.cpu().numpy()
    bad = np.flatnonzero(g_arena != w_arena)
    assert bad.size == 0, ("arena", bad[:16], g_arena[bad[:16]], w_arena[bad[:16]])
    assert np.array_equal(d_hs.cpu().numpy(), hsave) and np.array_equal(d_desc.cpu().numpy(), desc.view(np.uint8))
    assert np.array_equal(d_st.cpu().numpy(), status) and np.array_equal(d_opkt.cpu().numpy(), opkt.view(np.uint8))
    return g_arena, g_enc[:nenc], g_sst[:n]


# ---- (a) espgpu_ah_encap_batch and espgpu_ah_sent_batch --------------------------
@pytest.fixture(scope="module")
def mixed(env):
    rng = np.random.default_rng(7203)
    enc = _enc_table(rng)
    arena, rec, sa, kinds = _pool(rng, env, 1400, enc)
    return arena, rec, sa, kinds, enc


@pytest.mark.gpu
def test_encap_mixed_batch(env, mixed):
    arena, rec, sa, kinds, enc = mixed
    g_arena, desc, opkt, est, hs = _run_encap(env, arena, rec, sa, enc)
    assert {int(x) for x in np.unique(est)} == {0, EINVAL, ENOTSUP, EAFNOSUPPORT, ENOBUFS, EMSGSIZE}
    assert (kinds == "toobig").sum() >= 4 and (est[kinds == "toobig"] == EMSGSIZE).all()
    for kind, st in (("badopt", EINVAL), ("shortsr", EINVAL), ("badver", EAFNOSUPPORT), ("short", EINVAL),
                     ("badihl", EINVAL), ("linklocal", ENOTSUP), ("badflags", EINVAL), ("natflags", EINVAL),
                     ("esp", EINVAL), ("nosess", EINVAL), ("bigsa", EINVAL)):
        m = kinds == kind
        assert m.sum() > 5 and (est[m] == st).all(), (kind, est[m][:8])
    for kind in ("ok", "sr", "wild"):
        m = kinds == kind
        assert m.sum() > 5 and np.isin(est[m], [0, ENOBUFS]).all() and (est[m] == 0).sum() > 5, kind
    assert (est == ENOBUFS).sum() > 20
    ok = est == 0
    assert (desc["len"][~ok] == 0).all() and (desc["sa"][~ok] == 0xffff).all() and (opkt["len"][~ok] == 0).all()
    assert np.array_equal(desc["off4"][ok], opkt["off4"][ok]) and np.array_equal(desc["len"][ok], opkt["len"][ok])
    assert set((desc["salt"][ok] - 12).tolist()) == set(range(20, 64, 4))      # every ip_hl, and IPv6's 40
    front = (rec["off4"][ok].astype(np.int64) - opkt["off4"][ok]) * 4
    assert len(set(front.tolist())) >= 6                      # every ahsize, with and without an outer header
    assert set((opkt["len"][ok] - rec["len"][ok]).tolist()) == set(front.tolist())


@pytest.mark.gpu
@pytest.mark.parametrize("n", EDGES)
def test_encap_launch_edges(env, mixed, n):
    arena, rec, sa, kinds, enc = mixed
    sl = slice(7, 7 + n)
    _run_encap(env, arena, rec[sl], sa[sl], enc, nenc=len(enc) if n & 1 else NAH - 4, id0=0xffff0000 + n)


@pytest.mark.gpu
@pytest.mark.parametrize("opts", ["none", "one"])
def test_encap_waves_without_options_and_with_one_lane_of_them(env, opts):
    """none: no wave runs the option loop.  one: in every wave only lane 17
    has IPv4 options (good ones, refused ones, a source route, a short source
    route, wave after wave) and the other 63 lanes go through the loop's
    instantiation too."""
    rng = np.random.default_rng(7204 + len(opts))
    enc = _enc_table(rng)
    arena, rec, sa, kinds = _pool(rng, env, 700, enc, opts=opts)
    _, desc, opkt, est, _ = _run_encap(env, arena, rec, sa, enc)
    long_hdr = np.array([arena[int(o) * 4] >> 4 == 4 and arena[int(o) * 4] & 0xf > 5 for o in rec["off4"]])
    lane17 = np.arange(len(rec)) % 64 == 17
    if opts == "none":
        assert not (long_hdr & (kinds != "badihl")).any() and (est == 0).sum() > 100
    else:
        assert long_hdr[lane17].all() and not (long_hdr & ~lane17 & (kinds != "badihl")).any()
        for kind, st in (("ok", 0), ("sr", 0), ("badopt", EINVAL), ("shortsr", EINVAL)):
            m = lane17 & (kinds == kind)
            assert m.sum() >= 2 and (est[m] == st).all(), (kind, est[m])


def _after_encap(env, arena, rec, sa, enc, rng, fail=0.1, badslot=0.03):
    """The batch as the host rule's ah_encap leaves it, and a status array as
    the merges would: ah_encap's refusals, a few failures of the later stages,
    zeros; a few slots of accepted records spoilt."""
    n = len(rec)
    hs0 = rng.integers(0, 256, n * SLOT, dtype=np.uint8)
    a2, desc, opkt, est, hs = O.host_encap_batch(arena, rec, sa, enc, env.mlens, HEAD, 5, hs0)
    status = est.copy()
    bad = (rng.random(n) < fail) & (status == 0)
    status[bad] = rng.choice([EACCES, EBADMSG, EINVAL], int(bad.sum()))
    hs = hs.copy()
    for i in np.flatnonzero((rng.random(n) < badslot) & (status == 0)):
        hs[i * SLOT] ^= 0x20                                 # the other version
    return a2, desc, opkt, status, hs


@pytest.fixture(scope="module")
def sent_pool(env, mixed):
    arena, rec, sa, kinds, enc = mixed
    return _after_encap(env, arena, rec, sa, enc, np.random.default_rng(7205)) + (kinds, enc)


@pytest.mark.gpu
def test_sent_many_sas_interleaved(env, sent_pool):
    """Every wave holds records of many SAs: the per-wave loop books them."""
    arena, desc, opkt, status, hs, kinds, enc = sent_pool
    g_arena, g_enc, sst = _run_sent(env, arena, opkt, desc, status, enc, hs)
    assert {int(x) for x in np.unique(sst)} == {0, EINVAL} and 5 < (sst == EINVAL).sum() < 100
    ok = (status == 0) & (sst == 0)
    assert 200 < ok.sum() < (status == 0).sum()
    assert int((g_enc["packets"] - enc["packets"]).sum()) == int(ok.sum())
    assert int((g_enc["bytes"] - enc["bytes"]).sum()) == int(opkt["len"][ok].sum())
    assert len(np.flatnonzero(g_enc["packets"] != enc["packets"])) >= 20
    assert (g_arena != arena).sum() > 1000                   # headers were restored
    # an entry without ESPGPU_ENC_AH books nothing even where the status is 0
    e2 = enc.copy()
    e2["flags"][:8] &= ~np.uint32(L.ENC_AH)
    _, g2, s2 = _run_sent(env, arena, opkt, desc, status, e2, hs)
    assert np.array_equal(g2["packets"][:8], enc["packets"][:8]) and not s2[np.isin(desc["sa"], list(range(8)))].any()


@pytest.mark.gpu
@pytest.mark.parametrize("n", EDGES)
def test_sent_launch_edges(env, sent_pool, n):
    arena, desc, opkt, status, hs, kinds, enc = sent_pool
    sl = slice(7, 7 + n)
    _run_sent(env, arena, opkt[sl], desc[sl], status[sl], enc, hs[7 * SLOT:(7 + n) * SLOT],
              nenc=len(enc) if n & 1 else NAH - 4)


@pytest.mark.gpu
@pytest.mark.parametrize("sa,n", [(0, 1025), (1, 700)], ids=["inet-transport", "inet6-transport"])
def test_sent_one_sa_for_the_whole_batch(env, sa, n):
    """Every record of one SA: whole workgroups add once (the workgroup sum),
    and bytes crosses 2^32."""
    rng = np.random.default_rng(7206 + sa)
    enc = _enc_table(rng)
    enc["bytes"][sa], enc["packets"][sa] = 2**32 - 1000, 2**32 - 3
    arena, rec, ids, kinds = _pool(rng, env, n, enc, sas=[sa], kinds=("ok",))
    a2, desc, opkt, status, hs = _after_encap(env, arena, rec, ids, enc, rng, fail=0.03, badslot=0.01)
    _, g_enc, sst = _run_sent(env, a2, opkt, desc, status, enc, hs)
    ok = (status == 0) & (sst == 0)
    assert ok.sum() > n // 3
    assert int(g_enc["packets"][sa]) == 2**32 - 3 + int(ok.sum()) and g_enc["bytes"][sa] > 2**32
    others = np.arange(len(enc)) != sa
    assert np.array_equal(g_enc["packets"][others], enc["packets"][others])


@pytest.mark.gpu
def test_zero_packets_and_arguments(env, mixed):
    torch = _torch()
    arena, rec, sa, kinds, enc = mixed
    lib, ctx = env.drv.lib, env.drv.ctx
    d_arena, d_rec, d_enc = _up(torch, arena[:8192]), _up(torch, rec[:4]), _up(torch, enc)
    d_sa = torch.zeros(4, dtype=torch.int16, device="cuda")
    d_hs = torch.zeros(4 * SLOT + 4, dtype=torch.uint8, device="cuda")
    d_desc = torch.zeros(64, dtype=torch.uint8, device="cuda")
    d_opkt = torch.zeros(32, dtype=torch.uint8, device="cuda")
    d_st = torch.full((4,), 1, dtype=torch.uint8, device="cuda")
    d_out = torch.zeros(4, dtype=torch.uint8, device="cuda")
    d_osa = torch.zeros(32 * 4, dtype=torch.uint8, device="cuda")
    assert lib.espgpu_ah_encap_batch(ctx, None, None, None, 0, None, 0, 0, 0, None, None, None, None, None) == 0
    assert lib.espgpu_ah_frame_batch(ctx, None, None, 0, None, 0, None, None) == 0
    assert lib.espgpu_ah_sent_batch(ctx, None, None, None, None, 0, None, 0, None, None, None) == 0
    eargs = [d_arena.data_ptr(), d_rec.data_ptr(), d_sa.data_ptr(), 4, d_enc.data_ptr(), len(enc), HEAD, 0,
             d_hs.data_ptr(), d_desc.data_ptr(), d_opkt.data_ptr(), d_out.data_ptr(), None]
    fargs = [d_arena.data_ptr(), d_desc.data_ptr(), 4, d_osa.data_ptr(), 4, d_out.data_ptr(), None]
    sargs = [d_arena.data_ptr(), d_opkt.data_ptr(), d_desc.data_ptr(), d_st.data_ptr(), 4, d_enc.data_ptr(), len(enc),
             d_hs.data_ptr(), d_out.data_ptr(), None]
    assert lib.espgpu_ah_encap_batch(None, *eargs) == EINVAL and lib.espgpu_ah_frame_batch(None, *fargs) == EINVAL
    assert lib.espgpu_ah_sent_batch(None, *sargs) == EINVAL
    for k, v in ((0, None), (1, None), (2, None), (4, None), (8, None), (9, None), (10, None), (11, None),
                 (0, d_arena.data_ptr() + 2), (8, d_hs.data_ptr() + 1)):
        a = list(eargs)
        a[k] = v
        assert lib.espgpu_ah_encap_batch(ctx, *a) == EINVAL, (k, v)
    for k, v in ((0, None), (1, None), (3, None), (5, None), (0, d_arena.data_ptr() + 1)):
        a = list(fargs)
        a[k] = v
        assert lib.espgpu_ah_frame_batch(ctx, *a) == EINVAL, (k, v)
    for k, v in ((0, None), (1, None), (2, None), (3, None), (5, None), (7, None), (8, None),
                 (0, d_arena.data_ptr() + 1), (7, d_hs.data_ptr() + 2)):
        a = list(sargs)
        a[k] = v
        assert lib.espgpu_ah_sent_batch(ctx, *a) == EINVAL, (k, v)
    torch.cuda.synchronize()
    assert np.array_equal(d_arena.cpu().numpy(), arena[:8192]) and not d_hs.cpu().numpy().any()
    assert lib.espgpu_health(ctx) == 0


# ---- (b) espgpu_ah_frame_batch ----------------------------------------------------
def _frame_table(rng, env, nout):
    """outsa[nout]: spis, counters of every size, ESN and CYCSEQ here and there,
    and three SAs near the end of their number space."""
    from espgpu.batch import OUTSA_DTYPE
    t = np.zeros(nout, dtype=OUTSA_DTYPE)
    t["count"] = rng.integers(0, 2**31, nout)
    t["cntr"] = rng.integers(0, 2**63, nout)
    t["spi"] = rng.integers(256, 2**32, nout)
    t["salt"] = rng.integers(0, 2**32, nout)
    t["pad_"] = 0x0badf00d
    for k in range(nout):
        t["flags"][k] = (L.OUT_ESN if k % 3 == 0 else 0) | (L.OUT_WRAPCHECK if k % 4 == 0 else 0) | \
            (L.OUT_PAD_SEQ | L.OUT_CTRCOMPAT if k % 5 == 0 else 0)
        if k % 3 == 0:
            t["count"][k] += np.uint64(int(rng.integers(0, 5)) << 32)
    t["count"][2], t["flags"][2] = 2**32 - 1 - 9, 0                   # ends inside the batch: 9 numbers left
    t["count"][3], t["flags"][3] = 2**32 - 5, L.OUT_ESN               # ESN: goes through 2^32
    t["count"][4], t["flags"][4] = 2**32 - 3, L.OUT_CYCSEQ            # CYCSEQ: cycles
    t["count"][5], t["flags"][5] = 2**64 - 4, L.OUT_ESN               # 3 numbers left
    return t


def _frame_pool(rng, env, n, nout, hot=(2, 3, 4, 5)):
    """n descriptors over one arena: taking-part records of SAs below nout with
    non-taking ones interleaved.  Returns (arena, desc, kinds)."""
    kinds = np.array(rng.choice(["ok"] * 12 + ["len0", "bigsa", "esp", "nosess", "salt2", "salt8", "saltbig", "nosa"], n))
    desc = np.zeros(n, dtype=DESC)
    lens = rng.integers(44, 120, n) & ~3
    offs = np.concatenate([[0], np.cumsum((lens + 4 * rng.integers(0, 3, n))[:-1])]) + 8
    digests = np.array([k for k in range(min(nout, NSES)) if env.digest[k]])
    sa = digests[rng.integers(0, len(digests), n)]
    hotm = rng.random(n) < 0.12
    sa[hotm] = rng.choice(hot, int(hotm.sum()))
    tops = rng.random(n) < 0.1                               # the table's last entries: the highest radix digit
    sa[tops] = digests[-1 - rng.integers(0, 3, int(tops.sum()))]
    salt = (12 + 4 * rng.integers(0, 8, n)).astype(np.int64)
    edge = rng.random(n) < 0.1
    salt[edge] = lens[edge]                                  # the ICV field's offset at the very end
    ln = lens.copy()
    for kind, f in (("len0", lambda m: ln.__setitem__(m, 0)), ("bigsa", lambda m: sa.__setitem__(m, nout)),
                    ("esp", lambda m: sa.__setitem__(m, ESP0 + 1)), ("nosess", lambda m: sa.__setitem__(m, FREED)),
                    ("salt2", lambda m: salt.__setitem__(m, salt[m] + 2)), ("salt8", lambda m: salt.__setitem__(m, 8)),
                    ("saltbig", lambda m: salt.__setitem__(m, ln[m] + 4)), ("nosa", lambda m: sa.__setitem__(m, 0xffff))):
        f(kinds == kind)
    desc["off4"], desc["len"], desc["sa"], desc["esn_hi"], desc["salt"] = offs // 4, ln, sa, 0x5a5a5a5a, salt
    arena = rng.integers(0, 256, int(offs[-1] + lens[-1] + 64), dtype=np.uint8)
    return arena, desc, kinds


def _run_frame(env, arena, desc, outsa, nout=None, calls=None, drv=None):
    """Upload, ah_frame (once, or per (start, count) of `calls` back to back
    without a synchronisation), download, compare everything with the host
    rule.  Returns (desc, fstatus, outsa)."""
    torch = _torch()
    from espgpu.batch import OUTSA_DTYPE, ah_frame
    n = len(desc)
    nout = len(outsa) if nout is None else nout
    oguard = np.zeros(3, dtype=OUTSA_DTYPE)
    oguard.view(np.uint8)[:] = 0xC3
    dguard = np.zeros(GUARD, dtype=DESC)
    dguard.view(np.uint8)[:] = 0xC3
    d_arena, d_desc = _up(torch, arena), _up(torch, np.concatenate([desc, dguard]))
    d_out = _up(torch, np.concatenate([outsa[:nout], oguard]))
    d_fst = torch.full((n + GUARD,), 0x77, dtype=torch.uint8, device="cuda")
    for s, c in calls or [(0, n)]:
        ah_frame(drv or env.drv, d_arena, d_desc[s * 16:], c, d_out[:nout * OUTSA_DTYPE.itemsize], d_fst[s:])
    torch.cuda.synchronize()
    w_arena, w_desc, w_fst, w_out = O.host_frame_batch(arena, desc, outsa[:nout], env.digest)
    g_fst, g_desc = d_fst.cpu().numpy(), d_desc.cpu().numpy().view(DESC)
    g_out = d_out.cpu().numpy().view(OUTSA_DTYPE)
    bad = np.flatnonzero(g_fst[:n] != w_fst)
    assert bad.size == 0, ("fstatus", bad[:8], g_fst[bad[:8]], w_fst[bad[:8]], desc[bad[:8]])
    assert (g_fst[n:] == 0x77).all() and np.array_equal(g_desc[n:], dguard), "wrote past n"
    bad = np.flatnonzero(g_desc[:n] != w_desc)
    assert bad.size == 0, ("desc", bad[:8], g_desc[bad[:8]], w_desc[bad[:8]])
    for fld in ("count", "cntr", "spi", "salt", "flags", "pad_"):
        bad = np.flatnonzero(g_out[fld][:nout] != w_out[fld])
        assert bad.size == 0, ("outsa." + fld, bad[:8], g_out[fld][bad[:8]], w_out[fld][bad[:8]])
    assert np.array_equal(g_out[nout:].view(np.uint8), oguard.view(np.uint8)), "outsa guard entries written"
    g_arena = d_arena.cpu().numpy()
    bad = np.flatnonzero(g_arena != w_arena)
    assert bad.size == 0, ("arena", bad[:16], g_arena[bad[:16]], w_arena[bad[:16]])
    return g_desc[:n], g_fst[:n], g_out[:nout]


@pytest.mark.gpu
@pytest.mark.parametrize("n,nout", [(2047, 255), (2048, 256), (2049, 257), (4100, 257)])
def test_frame_sort_tiles_radix_passes_and_the_wrap(env, n, nout):
    rng = np.random.default_rng(7210 + n)
    outsa = _frame_table(rng, env, nout)
    arena, desc, kinds = _frame_pool(rng, env, n, nout)
    g_desc, fst, g_out = _run_frame(env, arena, desc, outsa)
    assert {int(x) for x in np.unique(fst)} == {0, EINVAL, EACCES}
    for kind in ("len0", "bigsa", "esp", "nosess", "salt2", "salt8", "saltbig", "nosa"):
        m = kinds == kind
        assert m.sum() > 10 and (fst[m] == EINVAL).all() and (g_desc["len"][m] == 0).all(), kind
    ok = kinds == "ok"
    # SA 2: nine numbers, then EACCES for the rest of its batch, the counter left at the limit
    m2 = ok & (desc["sa"] == 2)
    assert m2.sum() > 15 and not fst[m2][:9].any() and (fst[m2][9:] == EACCES).all() and int(g_out["count"][2]) == 2**32 - 1
    assert (g_desc["len"][m2][9:] == 0).all() and np.array_equal(g_desc["len"][m2][:9], desc["len"][m2][:9])
    m5 = ok & (desc["sa"] == 5)
    assert m5.sum() > 5 and not fst[m5][:3].any() and (fst[m5][3:] == EACCES).all() and int(g_out["count"][5]) == 2**64 - 1
    assert (g_desc["esn_hi"][m5][:3] == 2**32 - 1).all()
    for k in (3, 4):                                         # ESN and CYCSEQ go through 2^32
        mk = ok & (desc["sa"] == k)
        assert mk.sum() > 8 and not fst[mk].any() and int(g_out["count"][k]) == int(outsa["count"][k]) + int(mk.sum()) > 2**32
    assert set(g_desc["esn_hi"][ok & (desc["sa"] == 3)].tolist()) == {0, 1}
    assert set(g_desc["esn_hi"][ok & (desc["sa"] == 4)].tolist()) == {0}
    rest = ok & ~np.isin(desc["sa"], (2, 5))
    assert not fst[rest].any() and np.array_equal(g_desc["salt"][rest], desc["salt"][rest])
    assert int((fst[ok] == 0).sum()) == sum(int(a) - int(b) for a, b in zip(g_out["count"], outsa["count"]))
    top = sorted(set(desc["sa"][ok].tolist()))[-1]
    assert top == nout - 1 and g_out["count"][top] > outsa["count"][top]
    untouched = np.setdiff1d(np.arange(nout), desc["sa"][ok & (fst == 0)])
    assert untouched.size > 0 and np.array_equal(g_out[untouched], outsa[untouched])


@pytest.mark.gpu
def test_frame_two_calls_without_a_sync(env):
    rng = np.random.default_rng(7215)
    outsa = _frame_table(rng, env, 64)
    arena, desc, kinds = _frame_pool(rng, env, 3000, 64)
    _run_frame(env, arena, desc, outsa, calls=[(0, 1700), (1700, 1300)])


@pytest.mark.gpu
def test_frame_workspace_growth_on_a_fresh_driver():
    _torch()
    _symbols()
    from espgpu.opencrypto import GpuCryptoDriver

    class Small:
        digest = [True] * 6
    rng = np.random.default_rng(7216)
    drv = GpuCryptoDriver(max_sessions=8, batch_records=1024, batch_bytes=1 << 20, nbatches=1)
    try:
        for k in range(6):
            rc, sid = drv.newsession(AhSA(rng, 256).csp())
            assert rc == 0 and sid == k
        env = Small()
        for n in (100, 5000, 300):
            outsa = _frame_table(rng, env, 6)
            arena, desc, kinds = _frame_pool(rng, env, n, 6, hot=(2, 5))
            desc["sa"][np.isin(kinds, ["esp", "nosess"])] = 7           # no session there
            _run_frame(env, arena, desc, outsa, drv=drv)
    finally:
        drv.close()


# ---- (c), (d) the whole sequence ---------------------------------------------------
NCH = 10                    # AH SAs of the chain: SHA-1 / SHA2-256 / -384 / -512, ESN and not, both families
WSIZE, WWORDS = 64, 32
CHEAD = 88                  # an IPv6 tunnel with a 32-byte ICV


def _chain_tables(env, rng, count0):
    from espgpu.batch import OUTSA_DTYPE
    enc = _enc_table(rng)
    assert {(SHAS[k % 4], bool(k // 4 & 1)) for k in range(NCH)} == {(s, e) for s in SHAS for e in (False, True)}
    assert {(bool(k & 2), _af6(k)) for k in range(NCH)} == {(t, a) for t in (False, True) for a in (False, True)}
    outsa = np.zeros(FREED + 3, dtype=OUTSA_DTYPE)
    for k in range(NCH):
        outsa[k] = (count0(k), 0x1111 * k, env.sas[k].sa.spi, 0xdead0000 + k, L.OUT_ESN if env.sas[k].esn else 0, 7)
    return enc, outsa


def _device_out(env, arena, rec, sa, d_enc, d_outsa, head=CHEAD):
    """Steps 1-5 on one stream, no synchronisation in between."""
    torch = _torch()
    from espgpu.batch import ah_encap, ah_frame, ah_sent, encrypt_batch, replay_merge
    n, drv = len(rec), env.drv
    mk = lambda: torch.zeros(n, dtype=torch.uint8, device="cuda")        # noqa: E731
    est, fst, st, sst = mk(), mk(), torch.full((n,), 0x55, dtype=torch.uint8, device="cuda"), mk()
    d_arena, d_rec = _up(torch, arena), _up(torch, rec)
    d_sa = torch.from_numpy(sa.view(np.int16).copy()).cuda()
    d_desc = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
    d_opkt = torch.zeros(n * 8, dtype=torch.uint8, device="cuda")
    d_hs = torch.zeros(n * SLOT, dtype=torch.uint8, device="cuda")
    ah_encap(drv, d_arena, d_rec, d_sa, n, d_enc, head, 0x4000, d_hs, d_desc, d_opkt, est)
    ah_frame(drv, d_arena, d_desc, n, d_outsa, fst)
    encrypt_batch(drv, d_arena, d_desc, n, st)
    replay_merge(drv, st, fst, n)
    replay_merge(drv, st, est, n)
    ah_sent(drv, d_arena, d_opkt, d_desc, st, n, d_enc, d_hs, sst)
    torch.cuda.synchronize()
    assert not sst.cpu().numpy().any()
    return d_arena, d_opkt, st.cpu().numpy(), d_desc.cpu().numpy().view(DESC)


def _chain_packets(rng, enc, n, loop):
    """Cleartext packets for SAs 0 .. NCH - 1 with consistent lengths and valid
    checksums.  loop: packets a receiver can verify (no source routes, no
    fragments' bits) whose transport destination is the SA's."""
    sa = rng.integers(0, NCH, n).astype(np.uint16)
    pkts, kinds = [], []
    for i, k in enumerate(sa):
        e = enc[int(k)]
        tunnel, saf6 = bool(e["flags"] & L.ENC_TUNNEL), bool(e["flags"] & L.ENC_AF6)
        kind = "ok"
        if not loop and not tunnel and not saf6 and rng.random() < 0.3:
            kind = str(rng.choice(["sr", "badopt"]))
        p = _packet(rng, e, True, not tunnel, kind, min_ihl=6 if kind != "ok" else 5,
                    plen=int(rng.integers(0, 200)) if not tunnel else None, sr_ok=not loop)
        pkts.append(p)
        kinds.append(kind)
    return sa, pkts, np.array(kinds)


@pytest.mark.gpu
def test_whole_sequence_matches_the_restatement(env):
    """Encap, frame, digest, merges, sent against ipsec_output_encap_ah,
    ah_output_seq, ah_output, hashlib's HMAC over the massaged packet with the
    ICV field zero (and the high sequence word for ESN), ah_output_cb."""
    torch = _torch()
    from espgpu.batch import ENCSA_DTYPE, OUTSA_DTYPE, PKT_DTYPE
    rng = np.random.default_rng(7220)
    enc, outsa = _chain_tables(env, rng, lambda k: (5 << 32 | 1000 + k) if env.sas[k].esn else 1000 + k)
    n = 400
    sa, pkts, kinds = _chain_packets(rng, enc, n, loop=False)
    arena, rec = O.layout(rng, pkts, CHEAD)
    d_enc, d_outsa = _up(torch, enc), _up(torch, outsa)
    d_arena, d_opkt, st, desc = _device_out(env, arena, rec, sa, d_enc, d_outsa)
    wire, opkt = d_arena.cpu().numpy(), d_opkt.cpu().numpy().view(PKT_DTYPE)
    state = [E.OutState(int(outsa["count"][k]), 0, int(outsa["flags"][k])) for k in range(NCH)]
    booked_p, booked_b = np.zeros(NCH, dtype=np.int64), np.zeros(NCH, dtype=np.int64)
    seen = set()
    for i, p in enumerate(pkts):
        k = int(sa[i])
        s, e = env.sas[k], O.encsa_of(enc[k])
        wst, front, hashed, saved, hs, nxt = O.reference(e, s.mlen, p, CHEAD, 0x4000 + i)
        assert st[i] == wst, (i, kinds[i], st[i], wst)
        if wst:
            assert opkt["len"][i] == 0
            continue
        rc, hashed, esn_hi, state[k] = A.ah_output_seq(state[k], s.sa.spi, hashed, hs + 12)
        assert rc == 0
        m = bytearray(0 if b is None else b for b in hashed)                 # the ICV field hashed as zeros
        msg = bytes(m) + (struct.pack(">I", esn_hi) if s.esn else b"")
        m[hs + 12:hs + 12 + s.mlen] = pyhmac.new(s.key, msg, H.HASH[s.sha]).digest()[:s.mlen]
        want = bytes(A.ah_output_cb(list(m), saved))
        o = int(opkt["off4"][i]) * 4
        assert o == int(rec["off4"][i]) * 4 - front and int(opkt["len"][i]) == len(want)
        got = wire[o:o + len(want)].tobytes()
        assert got == want, (i, k, kinds[i], [j for j in range(len(want)) if got[j] != want[j]][:8])
        assert desc["esn_hi"][i] == esn_hi and desc["salt"][i] == hs + 12
        booked_p[k] += 1
        booked_b[k] += len(want)
        seen.add((s.sha, s.esn, bool(enc["flags"][k] & L.ENC_AF6), front > A.ah_hdrsiz(s.mlen, _af6(k)), kinds[i]))
    assert (st[kinds == "badopt"] == EINVAL).all() and (kinds == "badopt").sum() > 3
    assert not st[kinds == "sr"].any() and (kinds == "sr").sum() > 3
    assert len(seen) >= 12
    g_enc, g_out = d_enc.cpu().numpy().view(ENCSA_DTYPE), d_outsa.cpu().numpy().view(OUTSA_DTYPE)
    assert np.array_equal(g_enc["packets"][:NCH] - enc["packets"][:NCH], booked_p)
    assert np.array_equal(g_enc["bytes"][:NCH] - enc["bytes"][:NCH], booked_b)
    assert np.array_equal(g_enc[NCH:], enc[NCH:])
    assert [int(c) for c in g_out["count"][:NCH]] == [s.count for s in state]
    for fld in ("cntr", "spi", "salt", "flags", "pad_"):
        assert np.array_equal(g_out[fld], outsa[fld]), fld


def _insa_for(enc, nin):
    from espgpu.batch import INSA_DTYPE
    insa = np.zeros(nin, dtype=INSA_DTYPE)
    for k in range(min(nin, NAH)):
        f = int(enc["flags"][k])
        insa["flags"][k] = H.ah_flags(E.IPSEC_MODE_TUNNEL if f & L.ENC_TUNNEL else E.IPSEC_MODE_TRANSPORT,
                                      bool(f & L.ENC_AF6), bool(f & L.ENC_AH_KEEPTOS))
    return insa


def _device_in(env, d_arena, d_pkt, n, d_sad, d_tab, d_words, d_in):
    """The inbound AH sequence, steps 0-7, on one stream."""
    torch = _torch()
    from espgpu.batch import ah_decap, ah_input, decrypt_batch, esp_classify, replay_check, replay_merge, replay_update
    drv = env.drv
    mk = lambda: torch.zeros(n, dtype=torch.uint8, device="cuda")        # noqa: E731
    cst, ast, rst, ust, st, dst = mk(), mk(), mk(), mk(), mk(), mk()
    tr = torch.zeros(n, dtype=torch.int32, device="cuda")
    d_desc = torch.zeros(n * 16, dtype=torch.uint8, device="cuda")
    d_ipkt = torch.zeros(n * 8, dtype=torch.uint8, device="cuda")
    d_hs = torch.zeros(n * SLOT, dtype=torch.uint8, device="cuda")
    esp_classify(drv, d_arena, d_pkt, n, d_sad, d_desc, cst, flags=L.CLS_IPCSUM | L.CLS_AH)
    ah_input(drv, d_arena, d_desc, n, d_in, d_hs, ast)
    replay_check(drv, d_arena, d_desc, n, d_tab, d_words, rst)
    decrypt_batch(drv, d_arena, d_desc, n, st, trailer=tr)
    replay_update(drv, d_arena, d_desc, n, st, d_tab, d_words, ust)
    for r in (ast, rst, ust, cst):
        replay_merge(drv, st, r, n)
    ah_decap(drv, d_arena, d_desc, st, n, d_in, d_hs, d_ipkt, dst)
    replay_merge(drv, st, dst, n)
    torch.cuda.synchronize()
    return st.cpu().numpy(), d_ipkt


def _sad_and_windows(env, enc, extra=()):
    from espgpu.batch import REPLAY_DTYPE, SAD_DTYPE, sad_build
    ent = np.zeros(NCH + len(extra), dtype=SAD_DTYPE)
    for k in range(NCH):
        ent[k] = (env.sas[k].sa.spi, k, 51, 6 if _af6(k) else 4, 0x77777777, 0, list(enc["dst"][k]))
    for j, row in enumerate(extra):
        ent[NCH + j] = row
    tab = np.zeros(FREED + 1, dtype=REPLAY_DTYPE)
    for k in range(NCH):
        tab[k] = (0, WSIZE, WWORDS, WWORDS * k, (L.REPLAY_ESN if env.sas[k].esn else 0) | L.REPLAY_AH)
    return sad_build(ent, 64), tab


@pytest.mark.gpu
def test_outbound_then_inbound_gives_the_packets_back_and_refuses_a_replay(env):
    torch = _torch()
    from espgpu.batch import PKT_DTYPE
    rng = np.random.default_rng(7221)
    enc, outsa = _chain_tables(env, rng, lambda k: 0)
    n = 500
    sa, pkts, kinds = _chain_packets(rng, enc, n, loop=True)
    arena, rec = O.layout(rng, pkts, CHEAD)
    d_enc, d_outsa = _up(torch, enc), _up(torch, outsa)
    d_arena, d_opkt, st, desc = _device_out(env, arena, rec, sa, d_enc, d_outsa)
    assert not st.any()
    wire = d_arena.clone()
    table, tab = _sad_and_windows(env, enc)
    d_sad, d_tab = _up(torch, table), _up(torch, tab)
    d_words = torch.zeros(WWORDS * (FREED + 1), dtype=torch.int32, device="cuda")
    d_in = _up(torch, _insa_for(enc, FREED + 1))
    ist, d_ipkt = _device_in(env, d_arena, d_opkt, n, d_sad, d_tab, d_words, d_in)
    assert not ist.any(), (np.flatnonzero(ist)[:8], ist[ist != 0][:8])
    out, ipkt = d_arena.cpu().numpy(), d_ipkt.cpu().numpy().view(PKT_DTYPE)
    seen = set()
    for i, p in enumerate(pkts):
        o = int(ipkt["off4"][i]) * 4
        assert o == int(rec["off4"][i]) * 4 and int(ipkt["len"][i]) == len(p), i
        got = out[o:o + len(p)].tobytes()
        assert got == p, (i, int(sa[i]), [j for j in range(len(p)) if got[j] != p[j]][:8])
        seen.add((int(sa[i]), p[0] >> 4))
    assert len(seen) >= NCH + 2                              # every SA, and tunnels with both inner families
    # the same wire packets again: replayed
    ist2, d_ipkt2 = _device_in(env, wire, d_opkt, n, d_sad, d_tab, d_words, d_in)
    assert (ist2 == EACCES).all() and not d_ipkt2.cpu().numpy().view(PKT_DTYPE)["len"].any()


# ---- (e) an SA bundle: ESP inside, AH outside ----------------------------------------
@pytest.mark.gpu
def test_esp_then_ah_bundle_out_and_back_in(env):
    """ESP transport out, its d_opkt as the AH step's d_pkt, AH transport out;
    then AH in, its d_ipkt back into classification, ESP in: the cleartext."""
    torch = _torch()
    from espgpu.batch import (INSA_DTYPE, PKT_DTYPE, decrypt_batch, encrypt_batch,
                              esp_classify, esp_decap, esp_encap, esp_frame, esp_sent, replay_merge)
    rng = np.random.default_rng(7222)
    drv = env.drv
    enc, outsa = _chain_tables(env, rng, lambda k: 0)
    ahs = [k for k in range(NCH) if not k & 2 and not _af6(k)]          # AF_INET transport AH SAs
    assert len(ahs) >= 2
    for j in range(NESP):                                    # the ESP SAs: transport, the AH SA's destination
        k = ESP0 + j
        enc["flags"][k] = 0
        enc["dst"][k] = enc["dst"][ahs[j % len(ahs)]]
        s = env.sas[k]
        outsa[k] = (50 * j, 900 * j, s.spi, int.from_bytes(s.salt, "little"), L.OUT_PAD_SEQ, 0)
    n = 300
    esa = (ESP0 + rng.integers(0, NESP, n)).astype(np.uint16)
    asa = np.array([ahs[(int(k) - ESP0) % len(ahs)] for k in esa], dtype=np.uint16)
    pkts = []
    for k in asa:
        ihl = int(rng.integers(5, 16))
        pkts.append(O.clear4(rng, ihl, O.good_options(rng, ihl * 4 - 20, sr_ok=False),
                             int(rng.integers(0, 200)), dst=enc["dst"][int(k), :4].tobytes(), df=True,
                             proto=int(rng.choice([6, 17]))))
    ehead, tail, ahead = 16, 32, 44
    from encap_helpers import layout as elayout
    arena, rec = elayout(rng, pkts, ehead + ahead, tail)
    d_arena, d_rec = _up(torch, arena), _up(torch, rec)
    d_enc, d_outsa = _up(torch, enc), _up(torch, outsa)
    d_esa = torch.from_numpy(esa.view(np.int16).copy()).cuda()
    d_asa = torch.from_numpy(asa.view(np.int16).copy()).cuda()
    mk = lambda: torch.zeros(n, dtype=torch.uint8, device="cuda")        # noqa: E731
    z16 = lambda: torch.zeros(n * 16, dtype=torch.uint8, device="cuda")  # noqa: E731
    z8 = lambda: torch.zeros(n * 8, dtype=torch.uint8, device="cuda")    # noqa: E731
    est, fst, st = mk(), mk(), mk()
    d_desc, d_frame, d_eopkt = z16(), torch.zeros(n, dtype=torch.int32, device="cuda"), z8()
    esp_encap(drv, d_arena, d_rec, d_esa, n, d_enc, d_outsa, ehead, tail, 9, d_desc, d_frame, d_eopkt, est)
    esp_frame(drv, d_arena, d_desc, d_frame, n, d_outsa, fst)
    encrypt_batch(drv, d_arena, d_desc, n, st)
    replay_merge(drv, st, fst, n)
    replay_merge(drv, st, est, n)
    esp_sent(drv, d_eopkt, d_desc, st, n, d_enc)
    # the AH SA around it: step 1's d_pkt is ESP's d_opkt
    from espgpu.batch import ah_encap, ah_frame, ah_sent
    aest, afst, ast, sst = mk(), mk(), mk(), mk()
    d_adesc, d_aopkt = z16(), z8()
    d_hs = torch.zeros(n * SLOT, dtype=torch.uint8, device="cuda")
    ah_encap(drv, d_arena, d_eopkt, d_asa, n, d_enc, ahead, 77, d_hs, d_adesc, d_aopkt, aest)
    ah_frame(drv, d_arena, d_adesc, n, d_outsa, afst)
    encrypt_batch(drv, d_arena, d_adesc, n, ast)
    replay_merge(drv, ast, afst, n)
    replay_merge(drv, ast, aest, n)
    ah_sent(drv, d_arena, d_aopkt, d_adesc, ast, n, d_enc, d_hs, sst)
    torch.cuda.synchronize()
    assert not st.cpu().numpy().any() and not ast.cpu().numpy().any() and not sst.cpu().numpy().any()
    aopkt = d_aopkt.cpu().numpy().view(PKT_DTYPE)
    wire = d_arena.cpu().numpy()
    for i in range(0, n, 17):                                # IP | AH | ESP on the wire
        o = int(aopkt["off4"][i]) * 4
        hl = (int(wire[o]) & 0xf) * 4
        assert wire[o + 9] == 51 and wire[o + hl] == 50 and E.in_cksum(wire[o:o + hl].tobytes()) == 0
        assert struct.unpack(">H", wire[o + 2:o + 4].tobytes())[0] == aopkt["len"][i]
    # inbound: AH first
    extra = [(env.sas[ESP0 + j].spi, ESP0 + j, 50, 4, int.from_bytes(env.sas[ESP0 + j].salt, "little"), 0,
              list(enc["dst"][ESP0 + j])) for j in range(NESP)]
    table, tab = _sad_and_windows(env, enc, extra)
    d_sad, d_tab = _up(torch, table), _up(torch, tab)
    d_words = torch.zeros(WWORDS * (FREED + 1), dtype=torch.int32, device="cuda")
    insa = _insa_for(enc, FREED + 1)
    insa["flags"][ESP0:ESP0 + NESP] = L.IN_TRANSPORT
    d_in = _up(torch, insa)
    ist, d_ipkt = _device_in(env, d_arena, d_aopkt, n, d_sad, d_tab, d_words, d_in)
    assert not ist.any(), (np.flatnonzero(ist)[:8], ist[ist != 0][:8])
    # then ESP: d_ipkt goes straight back into classification
    cst, est2, dst = mk(), mk(), mk()
    tr = torch.zeros(n, dtype=torch.int32, device="cuda")
    d_idesc, d_fpkt = z16(), z8()
    esp_classify(drv, d_arena, d_ipkt, n, d_sad, d_idesc, cst, flags=L.CLS_IPCSUM | L.CLS_AH)
    decrypt_batch(drv, d_arena, d_idesc, n, est2, trailer=tr)
    replay_merge(drv, est2, cst, n)
    esp_decap(drv, d_arena, d_arena, d_ipkt, d_idesc, tr, est2, n, d_in, d_fpkt, dst)
    replay_merge(drv, est2, dst, n)
    torch.cuda.synchronize()
    assert not est2.cpu().numpy().any(), (cst.cpu().numpy()[:16], est2.cpu().numpy()[:16], dst.cpu().numpy()[:16])
    idesc = d_idesc.cpu().numpy().view(DESC)
    assert np.array_equal(idesc["sa"], esa)
    out, fpkt = d_arena.cpu().numpy(), d_fpkt.cpu().numpy().view(PKT_DTYPE)
    for i, p in enumerate(pkts):
        o = int(fpkt["off4"][i]) * 4
        assert int(fpkt["len"][i]) == len(p) and out[o:o + len(p)].tobytes() == p, i
    g_in = d_in.cpu().numpy().view(INSA_DTYPE)
    assert int(g_in["packets"][:NCH].sum()) == n and int(g_in["packets"][ESP0:ESP0 + NESP].sum()) == n
