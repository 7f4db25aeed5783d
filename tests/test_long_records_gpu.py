"""GPU parity for records from jumbo size to the largest a descriptor carries
(len is 16 bits: 65532 bytes), the long length sets and layouts of
sweep_helpers.py; their coverage is asserted on the CPU in
test_length_sweep.py.  Above test_length_sweep_gpu.py's lengths (GCM up to
8224 bytes, ETA up to 1088) the kernels run the same generic code, and this
module pins it where it had been run at a handful of lengths, decrypting, at
most:

  * GCM, every design: the counter cache (esp_gcm.hip ctr_cache_build, keyed
    on ctr >> 8) at keys 3, 4, 7, 8 and 15, records that end just before, at
    and just after a key change at every last-block size, the largest payloads
    each ICV length allows (the 8-byte ICV's reaches key 16), whole waves of
    one long length, and waves of 16 different lengths up to 64 KiB in which
    every lane changes its key at steps of its own;
  * ETA: the verified decrypt's equal-length path (j = f * ceil(2^32 / nbu)
    >> 32) at nbu up to 4092 blocks and its shuffle search over units of long
    records of different lengths; the wave-wide HMAC loops at every residue of
    the hashed length around 9 KB and at the limit; the CBC chain and CBC-MAC
    quads, AES-CTR and ESP-NULL at 64 KiB;
  * encryption of all of them, and the trailer words of long records.

Caller-grouped, out of place, in place and encrypting; the mixed layouts once
more through the planner.  Every case is decided by the oracle byte for byte
(sweep_helpers.check).  The GCM cases stand first and in functions of their
own, so that a fault in an ETA kernel cannot be taken
for one of theirs.  One long layout is kept at a time: a layout's three modes
follow each other, and a uniform GCM layout (built and run through the oracle
in about 1.5 s) is made once per design."""
import pytest

import sweep_helpers as H

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

MODES = ["outofplace", "inplace", "encrypt"]


@pytest.fixture(scope="module")
def drv():
    from espgpu.opencrypto import GpuCryptoDriver
    if not torch.cuda.is_available():
        pytest.fail("GPU test run without a visible HIP device")
    d = GpuCryptoDriver(max_sessions=64)
    yield d
    d.close()


def _run(drv, b, mode, grouped=True):
    sids = []
    try:
        for s in b.sas:
            rc, sid = drv.newsession(s.esp_sa().csp())
            assert rc == 0, drv.last_error()
            sids.append(sid)
        return H.check(drv, b, sids, mode, grouped=grouped)
    finally:
        for s in sids:
            drv.freesession(s)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("si", range(len(H.GCM_SESSIONS)), ids=H.GCM_SESSION_IDS)
def test_gcm_long_uniform(drv, gcm_lanes, si, mode):
    """GCM_LONG_LENS (85 lengths: 13 around each of five counter-key changes,
    the jumbo window, the 13 largest), 16 consecutive records each: 1360
    records in 44.0 MiB.  Two records tampered in every second run."""
    _run(drv, H.gcm_long_uniform(si), mode)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("si", range(len(H.GCM_SESSIONS)), ids=H.GCM_SESSION_IDS)
def test_gcm_long_aligned_waves(drv, gcm_lanes, si, mode):
    """GCM_LONG_ALIGNED, 16 records each: whole waves on the 4-lane kernel's
    aligned schedule, whose J0 slot takes a lane's counter back from keys 3, 4,
    7, 8 and 15 to key 0 (sweep_helpers.gcm_j0_back_key)."""
    _run(drv, H.gcm_long_aligned(si), mode)


@pytest.mark.parametrize("mode", MODES)
def test_gcm_long_mixed(drv, gcm_lanes, mode):
    """517 records, log-uniform lengths from 4 bytes to the largest, one above
    32 KiB and one below 64 bytes in every wave; two sessions, malformed
    lengths, the other session's id, 5 % tampered, a partial last wave."""
    _run(drv, H.gcm_long_mixed(), mode)


def test_gcm_long_mixed_through_the_planner(drv, gcm_lanes):
    """The same records with every descriptor naming its own session (through
    the planner another session's id is no error), out of place."""
    _run(drv, H.gcm_long_mixed(foreign=False), "outofplace", grouped=False)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kind", H.MIXED_KINDS)
def test_eta_long_uniform(drv, kind, mode):
    """The kind's 18 long lengths, 64 consecutive records each: 1152 records
    in 39.4 MiB.  Even units intact (the equal-length path of the verified
    decrypt), three records tampered in every odd one."""
    _run(drv, H.eta_long_uniform(kind), mode)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kind", H.MIXED_KINDS)
def test_eta_long_mixed(drv, kind, mode):
    """485 records, log-uniform lengths up to the kind's largest and one
    record of the largest in every unit; tampered, empty, orphan and (CBC)
    shortened records, a partial last unit."""
    _run(drv, H.eta_long_mixed(kind), mode)


@pytest.mark.parametrize("kind", H.MIXED_KINDS)
def test_eta_long_mixed_through_the_planner(drv, kind):
    _run(drv, H.eta_long_mixed(kind), "outofplace", grouped=False)
