"""Records at byte offsets of 2^31 and 2^32 and beyond (high_offset_helpers.py):
the GCM, ETA and AH digest kernels over the existing mixed layouts, packed
output into an `out` longer than 4 GiB, and the whole outbound and inbound
stage loop with NAT-T.

espgpu_desc.off4 and espgpu_pkt.off4 count 4-byte units, so a batch addresses
16 GiB.  Every case places a layout of 0.4 to 1.5 MB so that about half of its
records lie below the boundary ("sign": 2^31, where a byte offset cast to int
turns negative; "wrap": 2^32, where one held in 32 bits starts again at 0),
about half above, and one long record across it.  The comparisons are the
existing ones (sweep_helpers.check, ah_sweep_helpers.check,
test_esp_natt_gpu.end_to_end) on the window that holds the layout; after each
case every byte of both 6 GiB allocations outside the window must still hold
the fill pattern.  By the placement's safety condition (asserted on the CPU in
test_high_offsets.py) a kernel that drops or mis-extends an offset's high bits
lands in those allocations: the case fails, nothing faults."""
import numpy as np
import pytest

import ah_sweep_helpers as A
import high_offset_helpers as P
import oracle as O
import sweep_helpers as S
import test_esp_natt_gpu as N
from helpers import GcmSA, build_records, oracle_decrypt
from high_offset_helpers import AH_LAYOUTS, ETA_LAYOUTS, GCM_LAYOUTS

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

BOUNDARY = pytest.mark.parametrize("boundary", list(P.BOUNDARIES))
MODES = ["outofplace", "inplace", "encrypt"]


@pytest.fixture(scope="module")
def arenas():
    """Two allocations of 6.01 GiB, filled once.  Failing to get them fails
    the test: nothing here is skipped."""
    if not torch.cuda.is_available():
        pytest.fail("GPU test run without a visible HIP device")
    torch.cuda.empty_cache()
    try:
        a = P.Arenas()
    except AssertionError as e:
        pytest.fail(str(e))
    yield a
    a.release()


@pytest.fixture(scope="module")
def drv():
    from espgpu.opencrypto import GpuCryptoDriver
    if not torch.cuda.is_available():
        pytest.fail("GPU test run without a visible HIP device")
    d = GpuCryptoDriver(max_sessions=64)
    yield d
    d.close()


def _run(drv, arenas, b, boundary, mode, grouped=True):
    place = P.Placed(arenas, P.place_for_batch(b, boundary))
    sids = []
    try:
        for s in b.sas:
            rc, sid = drv.newsession(s.esp_sa().csp())
            assert rc == 0, drv.last_error()
            sids.append(sid)
        return S.check(drv, b, sids, mode, grouped=grouped, place=place)
    finally:
        for s in sids:
            drv.freesession(s)


# ---- GCM ---------------------------------------------------------------------

@BOUNDARY
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(GCM_LAYOUTS))
def test_gcm(drv, arenas, gcm_lanes, name, mode, boundary):
    _run(drv, arenas, GCM_LAYOUTS[name](), boundary, mode)


# ---- ETA ---------------------------------------------------------------------

@BOUNDARY
@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("name", list(ETA_LAYOUTS))
def test_eta(drv, arenas, name, mode, boundary):
    _run(drv, arenas, ETA_LAYOUTS[name](), boundary, mode)


@pytest.mark.parametrize("name", list(ETA_LAYOUTS))
def test_eta_through_the_planner(drv, arenas, name):
    _run(drv, arenas, ETA_LAYOUTS[name](), "wrap", "outofplace", grouped=False)


# ---- AH ----------------------------------------------------------------------

@BOUNDARY
@pytest.mark.parametrize("grouped", [True, False], ids=["grouped", "planner"])
@pytest.mark.parametrize("mode", A.MODES)
@pytest.mark.parametrize("name", list(AH_LAYOUTS))
def test_ah(drv, arenas, name, mode, grouped, boundary):
    lay = AH_LAYOUTS[name]()
    place = P.Placed(arenas, P.place_for_layout(lay, boundary))
    sids = []
    try:
        for s in lay.sas:
            rc, sid = drv.newsession(s.csp())
            assert rc == 0, drv.last_error()
            sids.append(sid)
        for k in lay.freed_sas:
            drv.freesession(sids[k])
        A.check(drv, lay, sids, mode, grouped=grouped, place=place)
    finally:
        for k, s in enumerate(sids):
            if k not in lay.freed_sas:
                drv.freesession(s)


# ---- packed output -------------------------------------------------------------

def test_packed_output_past_4_gib(drv, arenas):
    """espgpu_decrypt_batch_packed with a stride of 65536 and 65536 + 300 GCM
    records of 12 payload bytes: slot i lies at i * 65536 of `out` (the second
    allocation from its start), the last 300 slots at 2^32 and beyond.  The
    oracle decides every status and every slot's payload; the rest of every
    slot and everything behind the last one still hold the pattern, compared
    on the device (the first 64 bytes of each slot are downloaded through a
    strided view, nothing else of `out` is)."""
    from espgpu.batch import decrypt_batch_packed
    n, stride, c = P.PACKED_N, P.PACKED_STRIDE, P.PACKED_PAYLOAD
    rng = np.random.default_rng(9900)
    sa = GcmSA(rng)
    plain, ct, descs, eh = build_records(rng, [sa], np.zeros(n, dtype=np.int64), np.full(n, c))
    bad = ct.copy()
    flip = rng.random(n) < 0.02
    flip[[0, 65535, 65536, n - 1]] = [False, True, True, False]      # both kinds on both sides of 2^32
    for i in np.flatnonzero(flip):
        bad[int(descs["off4"][i]) * 4 + int(descs["len"][i]) - 1] ^= 0x10
    _, want_st = oracle_decrypt([sa], bad, descs, eh)
    assert ((want_st == O.EBADMSG) == flip).all() and (want_st[~flip] == 0).all()
    rc, sid = drv.newsession(sa.esp_sa().csp())
    assert rc == 0, drv.last_error()
    out = arenas.out_from_start()
    slots = out[:n * stride].view(n, stride)
    try:
        dd = descs.copy()
        dd["sa"] = sid
        arena = torch.from_numpy(bad).cuda()
        d_desc = torch.from_numpy(np.ascontiguousarray(dd).view(np.uint8).copy()).cuda()
        st = torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda")
        decrypt_batch_packed(drv, arena, d_desc, n, st, out, stride, grouped=True)
        torch.cuda.synchronize()
        got = st.cpu().numpy()
        wrong = np.flatnonzero(got != want_st)
        assert not len(wrong), "%d statuses differ, first: record %d got %d, the oracle %d" % (
            len(wrong), wrong[0], got[wrong[0]], want_st[wrong[0]])
        heads = slots[:, :64].cpu().numpy()
        # only the ICV was flipped: a failed record's unverified plaintext is the true one
        want = np.full((n, 64), P.PATTERN, dtype=np.uint8)
        o = descs["off4"].astype(np.int64) * 4
        want[:, :c] = plain[(o + 16)[:, None] + np.arange(c)[None, :]]
        diff = np.flatnonzero((heads != want).any(axis=1))
        assert not len(diff), "%d slots differ in their first 64 bytes, first: slot %d at byte %#x of out" % (
            len(diff), diff[0], int(diff[0]) * stride)
        assert not (torch.from_numpy(bad).cuda() != arena).any(), "the arena changed"
    finally:
        drv.freesession(sid)
        slots[:, :64].fill_(P.PATTERN)
        stray = [arenas.first_stray(t) for t in arenas.bufs]
    assert stray[1] is None, "out was written outside the slots' first 64 bytes: first at byte %#x (slot %d + %d)" % (
        stray[1], stray[1] // stride, stray[1] % stride)
    assert stray[0] is None, "the other allocation was written at byte %#x" % stray[0]


# ---- the stage kernels -----------------------------------------------------------

@BOUNDARY
@pytest.mark.parametrize("policy", [0, 1], ids=["auto", "recompute"])
def test_stage_loop_end_to_end(arenas, policy, boundary):
    """encap -> frame -> encrypt -> merges -> sent -> classify -> replay check
    -> decrypt with trailer -> window update -> decap -> NAT-T checksum
    (test_esp_natt_gpu.end_to_end) with the packets 72 + 49 bytes apart around
    the boundary: wire packets, ESP records and moved headers across it and
    beside it.  Only the cleartext packet list is relocated here."""
    N.end_to_end(policy, lambda arena, rec: P.Placed(arenas, P.place_for_packets(arena, rec, boundary)))

