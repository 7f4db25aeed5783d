"""GPU parity for the interior pair step of the fused GCM kernel (esp_gcm.hip
do_group: the step that runs whole under the record's exec mask, with the
grouped GHASH table reads and two rounds per round-key fetch), at the sizes
where its paths part: both schedules of the 4-lane kernel (aligned: the
payload's block count nct = 3 mod 4, as for 1448 and for 1452 bytes, both 91
blocks; position: any other, here 1464 bytes, 92 blocks with a partial last
one), every key length on that path, waves with absent and with invalid
lanes beside whole ones, forged records in place, and records whose counter's
second byte changes mid-record in some lanes of a wave only.

Every case is decided by the oracle, byte for byte over the whole arena:
  * decrypt in place: the arena equals the oracle's in-place result (a failed
    or invalid record untouched);
  * decrypt out of place: the arena is unchanged and `out` (zero before) holds
    the oracle's plaintext for every verified record and nothing else; the
    payload span of a record that failed its tag is unspecified there;
  * encrypt: the arena equals the oracle's ciphertext.
A record that carries another session's id inside a caller-grouped chunk is
the engine's own rule (EINVAL, untouched: the chunk is one session), which
the oracle has no notion of: the oracle runs over the other records, so such
a record is untouched in its arena too.

Through the `gcm_lanes` fixture each case runs the 4-lane kernel at these
sizes (and the 8-lane and burst designs, which share the code)."""
import functools

import numpy as np
import pytest

import oracle as O
from helpers import GcmSA, build_records
from sweep_helpers import _oracle, _payload_mask

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

WAVE = 16                       # records per wave of the 4-lane kernel
# payload bytes -> the 4-lane kernel's schedule for a batch of that size only
SIZES = [1448, 1452, 1464]
SIZE_IDS = ["aligned-1448", "aligned-1452", "position-1464"]
CHUNK = 256                     # records per caller-grouped chunk


@pytest.fixture(scope="module")
def drv():
    from espgpu.opencrypto import GpuCryptoDriver
    if not torch.cuda.is_available():
        pytest.fail("GPU test run without a visible HIP device")
    d = GpuCryptoDriver(max_sessions=64)
    yield d
    d.close()


def _dev(a):
    return torch.from_numpy(np.array(a)).cuda()           # a copy: the shared batches are read-only


def _descs_dev(descs):
    return torch.from_numpy(np.ascontiguousarray(descs).view(np.uint8).copy()).cuda()


def _sessions(drv, sas):
    sids = []
    for s in sas:
        rc, sid = drv.newsession(s.esp_sa().csp())
        assert rc == 0, drv.last_error()
        sids.append(sid)
    return sids


def _check(drv, sas, sids, mode, src, descs, eh, foreign=None):
    """Run one batch (caller-grouped: implicit chunks of one session) and
    compare it with the oracle as the module docstring says.  descs["sa"]
    indexes sas; foreign: records carrying another session's id."""
    from espgpu.batch import decrypt_batch, encrypt_batch
    n = len(descs)
    foreign = np.zeros(n, dtype=bool) if foreign is None else foreign
    ref, ref_st = _oracle(sas, src, descs, eh, ~foreign, encrypt=mode == "encrypt")
    d = descs.copy()
    d["sa"] = [sids[s] for s in descs["sa"]]
    arena = _dev(src)
    st = torch.full((n,), 0xEE, dtype=torch.uint8, device="cuda")
    if mode == "encrypt":
        encrypt_batch(drv, arena, _descs_dev(d), n, st, grouped=True)
    elif mode == "inplace":
        decrypt_batch(drv, arena, _descs_dev(d), n, st, out=None, grouped=True)
    else:
        out = torch.zeros_like(arena)
        decrypt_batch(drv, arena, _descs_dev(d), n, st, out=out, grouped=True)
    torch.cuda.synchronize()
    got = st.cpu().numpy()
    assert (got == ref_st).all(), "statuses differ at %s" % np.nonzero(got != ref_st)[0][:10]
    res = arena.cpu().numpy()
    if mode == "outofplace":
        assert (res == src).all(), "out of place: the arena changed at byte %d" % int(np.argmax(res != src))
        want = np.zeros_like(src)
        okm = _payload_mask(descs, ref_st == 0, len(src), sas)
        want[okm] = ref[okm]
        care = ~_payload_mask(descs, ref_st == O.EBADMSG, len(src), sas)
        o = out.cpu().numpy()
        diff = (o != want) & care
        assert not diff.any(), "first differing byte of out: %d" % int(np.argmax(diff))
    else:
        assert (res == ref).all(), "first differing byte %d" % int(np.argmax(res != ref))
    return ref_st


@functools.lru_cache(maxsize=None)
def _batch(klen, ct_len, n, seed):
    """One session's records of one payload size, built (and encrypted by the
    oracle) once and shared by the modes; never written to."""
    rng = np.random.default_rng(seed)
    sas = [GcmSA(rng, klen, esn=bool(klen & 8))]
    eh = rng.integers(0, 2**32, n, dtype=np.uint32)
    plain, ct, descs, eh = build_records(rng, sas, np.zeros(n, dtype=np.int64), np.full(n, ct_len), esn_hi=eh)
    for a in (plain, ct):
        a.setflags(write=False)
    return sas, plain, ct, descs, eh


@pytest.mark.parametrize("ct_len", SIZES, ids=SIZE_IDS)
@pytest.mark.parametrize("mode", ["outofplace", "encrypt", "inplace"])
@pytest.mark.parametrize("klen", [16, 24, 32])
def test_key_lengths_on_the_interior_path(drv, gcm_lanes, klen, mode, ct_len):
    """AES-128/192/256 (10, 12, 14 rounds: 4, 5 and 6 round pairs of the pair
    step's key fetch) in MODE 0, 1 and 3, on batches that take the interior
    path of one schedule only (SIZES); n = 16 k + 5 over two chunks, so the last wave
    has absent lanes."""
    n = WAVE * 20 + 5
    sas, plain, ct, descs, eh = _batch(klen, ct_len, n, 7000 + klen)
    sids = _sessions(drv, sas)
    try:
        st = _check(drv, sas, sids, mode, plain if mode == "encrypt" else ct, descs, eh)
        assert (st == 0).all()
    finally:
        for s in sids:
            drv.freesession(s)


@pytest.mark.parametrize("ct_len", SIZES, ids=SIZE_IDS)
@pytest.mark.parametrize("mode", ["outofplace", "encrypt", "inplace"])
def test_invalid_descriptors_beside_whole_waves(drv, gcm_lanes, mode, ct_len):
    """len & 3, payload length <= 0 and another session's id, placed so that
    in each aligned run of 256 records some waves have every lane valid (0, 2,
    4, ...), some have invalid records among valid ones (1, 3, 5) and one is
    invalid throughout (7); at this batch size the 4-lane kernel's chunks are
    four waves, so waves 0-3 and 4-7 each share a workgroup's chunk.  n =
    16 k + 5 ends in a wave with absent lanes and an invalid record."""
    n = CHUNK * 2 + WAVE * 2 + 5
    rng = np.random.default_rng(7100 + ct_len)
    sas = [GcmSA(rng, 16), GcmSA(rng, 16)]
    eh = rng.integers(0, 2**32, n, dtype=np.uint32)
    plain, ct, descs, eh = build_records(rng, sas, np.zeros(n, dtype=np.int64), np.full(n, ct_len),
                                         esn_hi=eh, stride_pad=8)
    foreign = np.zeros(n, dtype=bool)
    for base in range(0, n, CHUNK):
        def at(w, k):
            return base + WAVE * w + k
        picks = [(at(1, 1), "len3"), (at(1, 4), "nopay"), (at(1, 11), "sa"), (at(3, 1), "sa"),
                 (at(3, 15), "len3"), (at(5, 7), "nopay0")] + [(at(7, k), ("len3", "sa", "nopay", "sa")[k % 4])
                                                                for k in range(WAVE)]
        for i, kind in picks:
            if i >= n:
                continue
            if kind == "len3":
                descs["len"][i] += 2                     # len & 3 (the bytes lie in the stride's slack)
            elif kind == "nopay":
                descs["len"][i] = 28                     # payload length -4
            elif kind == "nopay0":
                descs["len"][i] = 32                     # payload length 0
            else:
                descs["sa"][i] = 1
                foreign[i] = True
    descs["len"][n - 2] += 2                             # in the last, partly absent wave
    # a chunk's first record names its session, and a batch this small runs in
    # chunks of as few as four records (launch_gcm)
    assert not foreign[::4].any()
    sids = _sessions(drv, sas)
    try:
        st = _check(drv, sas, sids, mode, plain if mode == "encrypt" else ct, descs, eh, foreign)
        # 22 per whole chunk, wave 1's three of the last chunk, and record n - 2
        assert (st == O.EINVAL).sum() == 22 + 22 + 3 + 1 and ((st == 0) | (st == O.EINVAL)).all()
    finally:
        for s in sids:
            drv.freesession(s)


@pytest.mark.parametrize("ct_len", SIZES, ids=SIZE_IDS)
def test_inplace_forged_records(drv, gcm_lanes, ct_len):
    """In place with forgeries in the AAD, the first, a middle and the last
    ciphertext block and the ICV: one whole wave of 16 failures and single
    failures in otherwise valid waves.  Failed records unchanged, good ones
    decrypted (the oracle's arena)."""
    n = WAVE * 20 + 5
    sas, plain, ct, descs, eh = _batch(16, ct_len, n, 7016)
    bad = ct.copy()
    flip = np.zeros(n, dtype=bool)
    flip[4 * WAVE:5 * WAVE] = True                       # a whole wave
    flip[[1, WAVE + 15, 2 * WAVE + 8, 7 * WAVE, 9 * WAVE + 3, CHUNK + 2, CHUNK + WAVE + 9, n - 1]] = True
    for k, i in enumerate(np.nonzero(flip)[0]):
        o, L = int(descs["off4"][i]) * 4, int(descs["len"][i])
        # (ct_len - 1: in the last block, which is partial for 1452 and 1464)
        pos = [o + 5, o + 16, o + 16 + 16 * 45 + 7, o + 16 + ct_len - 1, o + L - 1][k % 5]
        bad[pos] ^= 1 << (k % 8)
    sids = _sessions(drv, sas)
    try:
        st = _check(drv, sas, sids, "inplace", bad, descs, eh)
        assert (st[flip] == O.EBADMSG).all() and (st[~flip] == 0).all()
    finally:
        for s in sids:
            drv.freesession(s)


@pytest.mark.parametrize("mode", ["outofplace", "encrypt", "inplace"])
def test_counter_second_byte_changes_in_some_lanes(drv, gcm_lanes, mode):
    """8948-byte payloads (560 blocks: the counter's second byte changes
    twice) beside 1448-byte ones in the same wave, so the counter cache is
    rebuilt mid-record in some lanes only while the others have finished or
    run on.  (560 blocks are not 3 mod 4: these waves run the position
    schedule.)"""
    n = WAVE * 4 + 5
    rng = np.random.default_rng(7200)
    sas = [GcmSA(rng, 16)]
    cts = np.where(np.isin(np.arange(n) % WAVE, (0, 3, 7, 8, 15)), 8948, 1448)
    cts[2 * WAVE:3 * WAVE] = 8948                        # and one wave of long records only
    eh = rng.integers(0, 2**32, n, dtype=np.uint32)
    plain, ct, descs, eh = build_records(rng, sas, np.zeros(n, dtype=np.int64), cts, esn_hi=eh)
    bad = ct.copy()
    if mode != "encrypt":                                # a forgery past the counter's byte change
        o = int(descs["off4"][3]) * 4
        bad[o + 16 + 16 * 300] ^= 0x20
    sids = _sessions(drv, sas)
    try:
        st = _check(drv, sas, sids, mode, plain if mode == "encrypt" else bad, descs, eh)
        assert list(np.nonzero(st)[0]) == ([] if mode == "encrypt" else [3])
        assert mode == "encrypt" or st[3] == O.EBADMSG
    finally:
        for s in sids:
            drv.freesession(s)
