"""GPU parity over dense payload-length sweeps and prescribed wave
compositions (sweep_helpers.py): the GCM kernels (4-lane, 8-lane, burst) and
the ETA kernels (AES-CBC / AES-CTR / ESP-NULL with every HMAC, and AES-CBC
alone), caller-grouped, out of place, in place and encrypting.

Uniform: every length of the set fills a wave of its own (16 GCM records, 64
ETA records), so each length meets every schedule on its own terms.  Mixed:
the lengths inside a wave differ as each family prescribes (see the layout
functions).  Every case is decided by the oracle, byte for byte over the
whole arena, the prefilled `out`, the statuses and the trailer words
(sweep_helpers.check); a failure names the first differing record, its run
or unit and its payload length.

These sets end at 8224 bytes (GCM) and 1088 bytes (ETA).  Records from jumbo
size to the 65532 bytes a descriptor carries are swept the same way in
test_long_records_gpu.py."""
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
def test_gcm_uniform_waves(drv, gcm_lanes, si, mode):
    """GCM_LENS (every multiple of 4 up to 2112 bytes and around the lengths
    at which the counter's second byte changes), 16 consecutive records each.
    Length 0 is EINVAL with the record untouched (a wave of such records
    leaves at once); in every second run two records are tampered."""
    _run(drv, H.gcm_uniform(si), mode)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("kind", list(H.ETA_KINDS))
def test_eta_uniform_units(drv, kind, mode):
    """The kind's length set (CBC: 0..68 blocks; CTR and NULL: every multiple
    of 4 up to 1088 bytes), 64 consecutive records each; even units intact,
    three records tampered in every odd one."""
    _run(drv, H.eta_uniform(kind), mode)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("family", H.GCM_FAMILIES)
def test_gcm_mixed_waves(drv, gcm_lanes, family, mode):
    _run(drv, H.gcm_mixed(family), mode)


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("family", H.ETA_FAMILIES)
@pytest.mark.parametrize("kind", H.MIXED_KINDS)
def test_eta_mixed_units(drv, kind, family, mode):
    _run(drv, H.eta_mixed(family, kind), mode)


@pytest.mark.parametrize("mode", MODES)
def test_eta_sessions_interleaved_in_a_unit(drv, mode):
    _run(drv, H.eta_interleaved(), mode)


@pytest.mark.parametrize("kind", H.MIXED_KINDS)
def test_eta_random_through_the_planner(drv, kind):
    _run(drv, H.eta_mixed("h-random", kind), "outofplace", grouped=False)


def test_eta_sessions_interleaved_through_the_planner(drv):
    _run(drv, H.eta_interleaved(), "outofplace", grouped=False)
