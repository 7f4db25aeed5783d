"""The staging copies of the driver path (espgpu_process / flush / poll) over
record length, start alignment and threads per record, every result decided
by the oracle (staging_helpers.py; the layouts' coverage is asserted on the
CPU by test_staging_sweep.py):

  a. the xfer kernel, ESP: every session kind x record length mod 16 x start
     residue 0..15, staged records among them;
  b. ESP records that span several xfer pieces (4092 .. 65532 bytes), as
     small batches and as one large batch;
  c. the xfer kernel, AH: every byte length x start residue, COMPUTE and
     VERIFY;
  d. the self-staging GCM kernels on one workgroup, where a chunk holds up to
     256 records and stage_in gives a record 64 down to 2 threads;
  e. the same behind a live doorbell kernel, which takes its workgroups from
     the launched kernels' grid.

Every case checks every crp_etype, every byte of every packet buffer, the
whole registered buffer (the bytes between the packets stay zero) and the
zero-copy count."""
import pytest

import staging_helpers as S

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

REG_BYTES = 3 << 20


class _Env:
    def __init__(self, **kw):
        from espgpu.opencrypto import CryptoFramework, GpuCryptoDriver
        if not torch.cuda.is_available():
            pytest.fail("GPU test run without a visible HIP device")
        self.drv = GpuCryptoDriver(**kw)
        self.fw = CryptoFramework(self.drv)
        self.reg = S.aligned_zeros(REG_BYTES)
        self.drv.register_host(self.reg)
        self._ses = {}

    def tune(self, **kw):
        for k, v in kw.items():
            assert self.drv.set_tuning(k, v) == 0, k

    def sessions(self, lay):
        """A crypto_session per SA of the layout, opened once."""
        if id(lay) not in self._ses:
            out = []
            for sa in lay.sas:
                err, cs = self.fw.crypto_newsession(sa.esp_sa().csp())
                assert err == 0
                out.append(cs)
            self._ses[id(lay)] = (lay, out)
        return self._ses[id(lay)][1]

    def both_ways(self, lay, path):
        ses = self.sessions(lay)
        S.run_esp(self.fw, self.drv, self.reg, ses, lay, path, True)
        S.run_esp(self.fw, self.drv, self.reg, ses, lay, path, False)

    def close(self):
        try:
            self.drv.unregister_host(self.reg)
        finally:
            self.drv.close()


@pytest.fixture(scope="module", autouse=True)
def ah_offered():
    """The AH sessions of case c go through the probe: the bid for them on
    (set_tuning "ah_offer", process-wide), and back to the default afterwards."""
    from espgpu import _lib as L
    assert L.lib().espgpu_set_tuning(None, b"ah_offer", 1) == 0
    yield
    L.lib().espgpu_set_tuning(None, b"ah_offer", -1)


@pytest.fixture(scope="module")
def env():
    e = _Env(max_sessions=32)
    yield e
    e.close()


XFER = pytest.mark.parametrize("xfer", [1, 0], ids=["xfer-kernel", "memcpy"])


@XFER
def test_a_xfer_kernel_every_length_class_at_every_residue(env, xfer):
    """stage_fused 0: nothing bypasses the xfer kernel.  xfer 1: the staging
    region moves by it too; xfer 0: the zero-copy records alone."""
    env.tune(xfer=xfer, stage_fused=0)
    env.both_ways(S.esp_residues(), "xfer %d, stage_fused 0" % xfer)


@XFER
def test_b_records_of_several_pieces_small_batches(env, xfer):
    env.tune(xfer=xfer, stage_fused=0)
    env.both_ways(S.esp_pieces(False), "xfer %d, stage_fused 0, small batches" % xfer)


def test_b_records_of_several_pieces_large_batch(env):
    """One slot of 1.2 MB: the three streams, the zero-copy records moved on
    the compute stream."""
    env.tune(xfer=1, stage_fused=0)
    env.both_ways(S.esp_pieces(True), "large batch")


@XFER
@pytest.mark.parametrize("sha,esn", S.AH_SESSIONS, ids=S.AH_IDS)
def test_c_ah_every_byte_length_at_every_residue(env, sha, esn, xfer):
    """COMPUTE writes the mlen digest bytes, at a multiple of 4 from a start
    at any residue, and nothing else; VERIFY writes nothing."""
    env.tune(xfer=xfer, stage_fused=0)
    lay = S.ah_layout(sha, esn)
    err, ses = env.fw.crypto_newsession(lay.sa.csp())
    assert err == 0
    try:
        path = "xfer %d" % xfer
        S.run_ah(env.fw, env.drv, env.reg, ses, lay, path, S.COMPUTE)
        S.run_ah(env.fw, env.drv, env.reg, ses, lay, path, S.VERIFY)
    finally:
        env.fw.crypto_freesession(ses)


@pytest.fixture(scope="module")
def env1():
    """One workgroup for the launched GCM kernels."""
    e = _Env(max_sessions=32)
    e.tune(grid=1)
    yield e
    e.close()


@pytest.mark.parametrize("fused", [1, 0], ids=["self-staging", "xfer-control"])
@pytest.mark.parametrize("kernel", ["fused", "burst"])
@pytest.mark.parametrize("kind", S.STAGE_SESSIONS)
def test_d_self_staging_threads_per_record(env1, kind, kernel, fused):
    """grid 1: the chunk grows to 256 records and stage_in gives each record
    64 down to 4 (fused small-batch kernel) or 2 (burst kernel) threads; the
    same layouts through the xfer kernel (stage_fused 0) as the control."""
    env1.tune(stage_fused=fused, gcm_burst=4096 if kernel == "burst" else 0, xfer=1)
    for n in S.STAGE_N[kernel]:
        tprs = sorted(set(S.record_tpr(n, 1, kernel)))
        env1.both_ways(S.esp_stage(kind, n), "stage_fused %d, %s kernel, grid 1, n %d, threads per record %s" % (
            fused, kernel, n, tprs))


def test_e_grid_reduced_by_a_live_door():
    """door 64, grid 65, gcm_burst 32: a burst of 32 records goes through the
    doorbell kernel; the batch of 100 records behind it is launched (fused
    small-batch kernel) on the 65 - 64 = 1 workgroup the live door kernel
    leaves, one chunk of 128 records at 8 threads per record.  (Should the
    door kernel have honoured the retire request before the launch reads its
    state, the batch runs on 65 workgroups; the results are the same.)"""
    e = _Env(max_sessions=8)
    try:
        e.tune(door=64, grid=65, gcm_burst=32, stage_fused=1)
        kind = S.STAGE_SESSIONS[0]
        first, second = S.esp_stage(kind, 32), S.esp_stage(kind, 100)
        ses = e.sessions(first)
        d0 = e.drv.stats()["door"]
        S.run_esp(e.fw, e.drv, e.reg, ses, first, "door 64", True)
        assert e.drv.stats()["door"] - d0 == 1
        ses2 = e.sessions(second)
        S.run_esp(e.fw, e.drv, e.reg, ses2, second, "launched beside door 64, grid 65", True)
        assert e.drv.stats()["door"] - d0 == 1
        S.run_esp(e.fw, e.drv, e.reg, ses, first, "door 64", False)
        assert e.drv.stats()["door"] - d0 == 2
        S.run_esp(e.fw, e.drv, e.reg, ses2, second, "launched beside door 64, grid 65", False)
        assert e.drv.stats()["door"] - d0 == 2
    finally:
        e.close()
