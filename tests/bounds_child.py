"""The sweeps under the bounds-checked library (`make -C f-stack_amd checked`,
csrc/bounds_chk.h).  A plain script, not collected by pytest; no GPU work at
import.  test_bounds_gpu.py starts it as a fresh child with ESPGPU_LIB naming
libespgpu_chk.so:

    python tests/bounds_child.py FAMILY [--mode MODE] [--match TEXT]

FAMILY: gcm, ah, short-extent or pad; MODE keeps the runs of
one mode (outofplace / inplace / encrypt; AH: outofplace / inplace / sign),
TEXT those whose label contains it.
It opens one GpuCryptoDriver, runs the family's layouts through the `check`
functions of sweep_helpers and ah_sweep_helpers (so the oracle still decides
every byte in the checked build), arms the context before every launch and
prints one JSON report as its last line.  The ETA kernels (esp_cbc.hip) are
not instrumented and no family launches them.

The armed extent is the header's contract (include/espgpu.h, d_arena): the
largest off4 * 4 + len over ALL descriptors of the batch, malformed ones
included, reads allowed 16 bytes past it.  The tensor's own size is not used.

Loaded with the default library (no espgpu_chk_* symbols) nothing is armed
and the report carries the times alone: the same layouts' wall time beside
the checked build's."""
import ctypes as C
import functools
import json
import os
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (os.path.join(ROOT, "f-stack_amd"), os.path.join(ROOT, "oracle"), HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

PAD = 16                      # include/espgpu.h: d_arena needs 16 spare bytes at its end
SHORT = 32                    # short-extent: the arena armed this far short of the last record's end
KEEP = 64                     # bounds_chk.h kChkKeep
NO_MARK = -2**63              # bounds_chk.h kChkNoMark
FILE_TAGS = {1: "esp_gcm.hip", 3: "esp_ah.hip"}
KINDS = ["read", "write", "desc", "status", "trailer", "order", "chunks", "sas"]
LOAD_HELPERS = ("ld16(", "esp_ld4(", "esp_ld4w(")
GCM_DESIGNS = [("lanes4", 4, 0), ("lanes8", 8, 0), ("burst", 8, 1 << 30)]    # as conftest.py's gcm_lanes
FAMILIES = ("gcm", "ah", "short-extent", "pad")


def armed_extent(descs):
    """The bytes of the arena the header's contract covers: the largest
    off4 * 4 + len over every descriptor (numpy records with off4 and len)."""
    return int((descs["off4"].astype(np.int64) * 4 + descs["len"].astype(np.int64)).max())


class Violation(C.Structure):
    _fields_ = [("site", C.c_uint32), ("kind", C.c_uint32), ("buf", C.c_uint32), ("bytes", C.c_uint32),
                ("at", C.c_int64), ("bound", C.c_uint64), ("block", C.c_uint32), ("lane", C.c_uint32)]


class Report(C.Structure):
    _fields_ = [("nviol", C.c_uint32), ("pad_", C.c_uint32), ("nchecked", C.c_uint64), ("hw", C.c_int64 * 2),
                ("v", Violation * KEEP)]


def site_name(site):
    return "%s:%d" % (FILE_TAGS.get(site >> 16, "file%d" % (site >> 16)), site & 0xffff)


def site_line(site, csrc=os.path.join(ROOT, "f-stack_amd", "csrc")):
    """The source line a site id names ("" if there is none)."""
    try:
        with open(os.path.join(csrc, FILE_TAGS[site >> 16])) as f:
            return f.read().splitlines()[(site & 0xffff) - 1]
    except (KeyError, IndexError, OSError):
        return ""


def is_record_load_site(site):
    return any(h in site_line(site) for h in LOAD_HELPERS)


# ---------------------------------------------------------------------------
# the runs of a family: (label, "S" or "A", layout thunk, mode, grouped, design)

def gcm_runs():
    import sweep_helpers as S
    modes = ["outofplace", "inplace", "encrypt"]
    runs = []
    for design in GCM_DESIGNS:
        for si, sid in enumerate(S.GCM_SESSION_IDS):
            runs += [("gcm_uniform[%s] %s" % (sid, design[0]), "S", lambda i=si: S.gcm_uniform(i), m, True, design)
                     for m in modes]
        for fam in S.GCM_FAMILIES:
            runs += [("gcm_mixed[%s] %s" % (fam, design[0]), "S", lambda f=fam: S.gcm_mixed(f), m, True, design)
                     for m in modes]
        # records up to 65532 bytes, every lane of a wave at a length of its own (about 5 MB; the
        # uniform long layouts, 44 MiB each, stay with the default library)
        runs += [("gcm_long_mixed %s" % design[0], "S", S.gcm_long_mixed, m, True, design) for m in modes]
    return runs


def ah_runs():
    import ah_sweep_helpers as A
    runs = []
    for name, fn in (("uniform", A.uniform), ("quads", A.quads), ("one_long", A.one_long)):
        for (sha, esn), hid in zip(A.HASH_ESN, A.HASH_ESN_IDS):
            runs += [("ah_%s[%s]" % (name, hid), "A", lambda f=fn, s=sha, e=esn: f(s, e), m, True, None)
                     for m in A.MODES]
    runs += [("ah_hashes", "A", A.hashes, m, True, None) for m in A.MODES]
    for grouped in (True, False):
        runs += [("ah_random_mix %s" % ("grouped" if grouped else "planner"), "A", A.random_mix, m, grouped, None)
                 for m in A.MODES]
    runs.append(("ah_hashes planner", "A", A.hashes, "outofplace", False, None))
    runs += [("ah_key_lengths", "A", A.key_lengths, m, True, None) for m in A.MODES]
    return runs


@functools.lru_cache(maxsize=None)
def tail_layout(si, rem):
    """One wave of GCM records (session si of GCM_SESSIONS) of one payload
    length whose last block holds rem bytes (4, 8, 12 or 16), the second
    record's ICV tampered.  A mark is taken against the end of the arena's
    LAST record, so the uniform layouts (which end on their longest length,
    a whole last block) measure that one record's tail alone; these end on
    every tail the kernels tell apart."""
    import sweep_helpers as S
    rng = np.random.default_rng(8600 + 4 * si + rem // 4)
    n = S.GCM_RUN
    return S.make_batch(rng, [S._gcm_sa(rng, si)], np.zeros(n, dtype=np.int64), np.full(n, 32 + rem), [(1, "icv")])


def pad_runs():
    """The GCM uniform layouts, every session (so every ICV length), in the
    three modes and designs; then tail_layout for every session and every
    last-block length."""
    import sweep_helpers as S
    modes = ["outofplace", "inplace", "encrypt"]
    runs = [r for r in gcm_runs() if r[0].startswith("gcm_uniform")]
    for design in GCM_DESIGNS:
        for si, sid in enumerate(S.GCM_SESSION_IDS):
            for rem in (4, 8, 12, 16):
                runs += [("gcm_tail[%s,rem%d] %s" % (sid, rem, design[0]), "S", lambda i=si, r=rem: tail_layout(i, r),
                          m, True, design) for m in modes]
    return runs


def short_runs():
    import sweep_helpers as S
    return [("gcm_uniform[aes192-icv8] short", "S", lambda: S.gcm_uniform(2), "outofplace", True, None)]


def runs_of(family, mode=None):
    runs = {"gcm": gcm_runs, "ah": ah_runs, "pad": pad_runs,
            "short-extent": short_runs}[family]()
    return [r for r in runs if mode is None or r[3] == mode]


def layout_descs(lay):
    return lay.descs


def layout_arena_bytes(lay, which):
    """The bytes of the arena tensor check() builds for the layout."""
    return len(lay.plain) if which == "S" else len(lay.arena)


# ---------------------------------------------------------------------------
# the driver handed to check(): arms the context before every launch

class _ArmingLib:
    def __init__(self, lib, arena_bytes, out_bytes):
        self._lib, self._ab, self._ob = lib, arena_bytes, out_bytes
        self.launches = 0

    def _arm(self, ctx, arena, out):
        self.launches += 1
        if hasattr(self._lib, "espgpu_chk_arm"):
            rc = self._lib.espgpu_chk_arm(ctx, arena, self._ab, out, self._ob, PAD)
            assert rc == 0, "espgpu_chk_arm: %d" % rc

    def espgpu_decrypt_batch_trailer(self, ctx, arena, desc, n, st, out, trl, flags, stream):
        self._arm(ctx, arena, out)
        return self._lib.espgpu_decrypt_batch_trailer(ctx, arena, desc, n, st, out, trl, flags, stream)

    def espgpu_decrypt_batch(self, ctx, arena, desc, n, st, out, flags, stream):
        self._arm(ctx, arena, out)
        return self._lib.espgpu_decrypt_batch(ctx, arena, desc, n, st, out, flags, stream)

    def espgpu_encrypt_batch(self, ctx, arena, desc, n, st, flags, stream):
        self._arm(ctx, arena, None)
        return self._lib.espgpu_encrypt_batch(ctx, arena, desc, n, st, flags, stream)


class ArmingDriver:
    """What check() sees of a driver (lib, ctx, last_error), the batch calls
    armed with the given extents first."""

    def __init__(self, drv, arena_bytes, out_bytes):
        self._drv, self.ctx = drv, drv.ctx
        self.lib = _ArmingLib(drv.lib, arena_bytes, out_bytes)

    def last_error(self):
        return self._drv.last_error()


class Checker:
    def __init__(self, drv):
        self.drv, self.lib = drv, drv.lib
        self.live = hasattr(self.lib, "espgpu_chk_arm")
        if self.live:
            vp = C.c_void_p
            self.lib.espgpu_chk_arm.argtypes = [vp, vp, C.c_uint64, vp, C.c_uint64, C.c_uint32]
            self.lib.espgpu_chk_report.argtypes = [vp, vp, C.c_uint32]
            self.lib.espgpu_chk_reset.argtypes = [vp]

    def reset(self):
        if self.live:
            assert self.lib.espgpu_chk_reset(self.drv.ctx) == 0, self.drv.last_error()

    def report(self):
        """-> dict(violations, checked, marks [arena, out] (None: no access seen), first: the kept violations)"""
        if not self.live:
            return dict(violations=0, checked=0, marks=[None, None], first=[])
        r = Report()
        got = self.lib.espgpu_chk_report(self.drv.ctx, C.byref(r), C.sizeof(r))
        assert got == C.sizeof(r), "espgpu_chk_report: %d" % got
        first = []
        for k in range(min(r.nviol, KEEP)):
            v = r.v[k]
            first.append(dict(site=v.site, name=site_name(v.site), kind=KINDS[v.kind] if v.kind < len(KINDS) else v.kind,
                              buf=v.buf, bytes=v.bytes, at=v.at, bound=v.bound, block=v.block, lane=v.lane))
        return dict(violations=r.nviol, checked=r.nchecked, marks=[None if m == NO_MARK else m for m in r.hw],
                    first=first)


def _open_sessions(drv, lay, which):
    sids = []
    for s in lay.sas:
        rc, sid = drv.newsession(s.esp_sa().csp() if which == "S" else s.csp())
        assert rc == 0, drv.last_error()
        sids.append(sid)
    freed = getattr(lay, "freed_sas", ())
    for k in freed:
        drv.freesession(sids[k])
    return sids, freed


def _close_sessions(drv, sids, freed):
    for k, s in enumerate(sids):
        if k not in freed:
            drv.freesession(s)


def _set_design(drv, design):
    lanes, burst = (design[1], design[2]) if design else (0, 4096)
    assert drv.lib.espgpu_set_tuning(drv.ctx, b"gcm_lanes", lanes) == 0
    assert drv.lib.espgpu_set_tuning(drv.ctx, b"gcm_burst", burst) == 0


def run_checked(drv, chk, run):
    """One layout in one mode through its helper's check(), armed with the
    header's extent.  -> the run's entry of the report."""
    import torch
    label, which, thunk, mode, grouped, design = run
    lay = thunk()
    ext = armed_extent(layout_descs(lay))
    assert ext + PAD <= layout_arena_bytes(lay, which), "%s: the armed extent + pad leaves the arena tensor" % label
    if which == "S":
        import sweep_helpers as H
        H.expected(lay, mode == "encrypt")          # (the oracle's side outside the timed span)
    else:
        import ah_sweep_helpers as H
        H.reference(lay)
    _set_design(drv, design)
    sids, freed = _open_sessions(drv, lay, which)
    try:
        chk.reset()
        armed = ArmingDriver(drv, ext, ext)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        H.check(armed, lay, sids, mode, grouped=grouped)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        assert armed.lib.launches == 1
        rep = chk.report()
    finally:
        _close_sessions(drv, sids, freed)
        _set_design(drv, None)
    rep.update(label=label, mode=mode, extent=ext, seconds=round(dt, 4), mlen=sorted({int(s.mlen) for s in lay.sas}),
               kernel="gcm" if label.startswith("gcm") else "ah")
    return rep


def run_short(drv, chk, run):
    """The control: the layout out of place with the ARENA armed SHORT bytes
    short of its last record's end (`out` armed in full, so no store is
    concerned).  The bytes exist; the checker merely was told less.  The last
    record's loads past the armed end + pad are refused and read as zeros, so
    its verification fails; every other record must match the oracle."""
    import torch
    import oracle as O
    import sweep_helpers as H
    from espgpu.batch import decrypt_batch
    label, which, thunk, mode, grouped, design = run
    b = thunk()
    ends = b.descs["off4"].astype(np.int64) * 4 + b.descs["len"].astype(np.int64)
    last = int(np.argmax(ends))
    ext = int(ends[last])
    assert int(np.sort(ends)[-2]) <= ext - SHORT, "the record before the last ends inside the cut"
    ref, ref_st, ref_trl = H.expected(b, False)
    sids, freed = _open_sessions(drv, b, which)
    try:
        chk.reset()
        armed = ArmingDriver(drv, ext - SHORT, ext)
        d = b.descs.copy()
        d["sa"] = [sids[s] for s in b.descs["sa"]]
        d["sa"][b.orphan] = 0xFFFF
        arena = torch.from_numpy(np.array(b.bad)).cuda()
        descs = torch.from_numpy(np.ascontiguousarray(d).view(np.uint8).copy()).cuda()
        st = torch.full((b.n,), 0xEE, dtype=torch.uint8, device="cuda")
        trl = torch.from_numpy(np.full(b.n, H.TRL_FILL, dtype=np.uint32).view(np.int32)).cuda()
        out = torch.full_like(arena, H.OUT_FILL)
        t0 = time.perf_counter()
        decrypt_batch(armed, arena, descs, b.n, st, out=out, grouped=True, trailer=trl)
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        rep = chk.report()
    finally:
        _close_sessions(drv, sids, freed)
    others = np.arange(b.n) != last
    got = st.cpu().numpy()
    wrong = np.nonzero((got != ref_st) & others)[0]
    assert not len(wrong), "short extent: status %d, the oracle %d at %s" % (got[wrong[0]], ref_st[wrong[0]],
                                                                              b.where(wrong[0]))
    assert (arena.cpu().numpy() == b.bad).all(), "short extent: the arena changed"
    want = np.full_like(b.bad, H.OUT_FILL)
    okm = H._payload_mask(b.descs, (ref_st == 0) & others, len(b.bad), b.sas)
    want[okm] = ref[okm]
    care = ~H._payload_mask(b.descs, (ref_st == O.EBADMSG) | ~others, len(b.bad), b.sas)
    diff = (out.cpu().numpy() != want) & care
    assert not diff.any(), "short extent: out differs at " + b.where_byte(int(np.argmax(diff)))
    gt = trl.cpu().numpy().view(np.uint32)
    wrong = np.nonzero((gt != ref_trl) & others)[0]
    assert not len(wrong), "short extent: trailer word differs at " + b.where(wrong[0])
    rep.update(label=label, mode=mode, extent=ext - SHORT, last_end=ext, seconds=round(dt, 4),
               last_status=int(got[last]), oracle_last_status=int(ref_st[last]),
               load_sites=[bool(is_record_load_site(v["site"])) for v in rep["first"]])
    return rep


def main(argv):
    import argparse
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("family", choices=FAMILIES)
    ap.add_argument("--mode", default=None)
    ap.add_argument("--match", default="")
    a = ap.parse_args(argv)
    import torch
    from espgpu.opencrypto import GpuCryptoDriver
    from espgpu import _lib as L
    if not torch.cuda.is_available():
        print("bounds_child: no visible HIP device", file=sys.stderr)
        return 2
    drv = GpuCryptoDriver(max_sessions=64)
    items = []
    t_all = time.perf_counter()
    try:
        chk = Checker(drv)
        if a.family == "ah":
            assert L.lib().espgpu_set_tuning(None, b"ah_offer", 1) == 0
        for run in [r for r in runs_of(a.family, a.mode) if a.match in r[0]]:
            items.append((run_short if a.family == "short-extent" else run_checked)(drv, chk, run))
    finally:
        drv.close()
    first = [v for it in items for v in it["first"]][:KEEP]
    marks = [max([it["marks"][k] for it in items if it["marks"][k] is not None], default=None) for k in (0, 1)]
    for it in items:
        del it["first"]
    print(json.dumps(dict(family=a.family, mode=a.mode, live=chk.live, library=os.path.basename(L.LIB_PATH),
                          violations=sum(it["violations"] for it in items),
                          checked=sum(it["checked"] for it in items), marks=marks, first=first,
                          gpu_seconds=round(sum(it["seconds"] for it in items), 3),
                          wall_seconds=round(time.perf_counter() - t_all, 3), runs=items)))
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
