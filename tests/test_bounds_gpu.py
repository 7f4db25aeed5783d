"""The length sweeps under the bounds-checked library (`make checked`,
csrc/bounds_chk.h): every record-derived global-memory access of esp_gcm.hip
and esp_ah.hip is checked against the extent the header promises
callers (include/espgpu.h: the largest record end, 16 spare bytes for reads)
and against its index bound; an access that leaves it is reported and not
made.  Output parity cannot see a stray read; this can.

One fresh child process per case (tests/bounds_child.py with ESPGPU_LIB =
libespgpu_chk.so), each under its own time limit; the child still compares
every byte with the oracle.  After a child that ended with any status but 0
(a GPU fault can surface as a HIP error in a process that goes on running and
exits 1) or ran into its limit, the module starts no further child.  The default library, conftest.py,
smoke() and bench.py never load the checked build.

short-extent is the control that the checker is live: the arena armed 32
bytes short of its last record's end.  The bytes exist; the checker merely
was told less.

The ETA kernels (esp_cbc.hip) are not instrumented and no case here launches
them: DESIGN.md, section 4."""
import json
import os
import subprocess
import sys

import pytest

import bounds_child as B

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "f-stack_amd")
CHILD = os.path.join(ROOT, "tests", "bounds_child.py")
LIMIT = 300                                   # seconds per child
_state = {"dead": None}


@pytest.fixture(scope="module")
def checked_lib():
    subprocess.run(["make", "-s", "-C", PKG, "-j8", "checked"], check=True, timeout=900, stdout=subprocess.DEVNULL)
    return os.path.join(PKG, "libespgpu_chk.so")


def _child(lib, family, mode=None):
    """-> the child's report.  Fails the test on a nonzero exit status or a
    child that ran into its limit; after either, no further start."""
    if _state["dead"]:
        pytest.fail("not started: %s" % _state["dead"])
    env = dict(os.environ, ESPGPU_LIB=lib)
    cmd = [sys.executable, CHILD, family] + (["--mode", mode] if mode else [])
    try:
        r = subprocess.run(cmd, env=env, cwd=ROOT, capture_output=True, text=True, timeout=LIMIT)
    except subprocess.TimeoutExpired:
        _state["dead"] = "the %s child did not finish in %d s" % (family, LIMIT)
        pytest.fail(_state["dead"])
    if r.returncode != 0:
        _state["dead"] = "the %s child ended with status %d" % (family, r.returncode)
    assert r.returncode == 0, "%s child: exit status %d\n%s" % (family, r.returncode, r.stderr[-4000:])
    rep = json.loads(r.stdout.strip().splitlines()[-1])
    assert rep["live"] and rep["library"] == "libespgpu_chk.so", "the child did not run the checked library"
    print("%s%s: %d runs, %d checked accesses, %d violations, marks %s, gpu-side %.1f s, child %.1f s" % (
        family, " " + mode if mode else "", len(rep["runs"]), rep["checked"], rep["violations"], rep["marks"],
        rep["gpu_seconds"], rep["wall_seconds"]))
    return rep


def _assert_clean(rep):
    assert rep["runs"], "the case ran nothing"
    assert rep["violations"] == 0, "violations: " + json.dumps(rep["first"][:8])
    for run in rep["runs"]:
        assert run["checked"] > 0, "no checked access in " + run["label"]
        for m in run["marks"]:
            assert m is None or m <= B.PAD, "%s %s: an access ends %d bytes past the armed extent" % (
                run["label"], run["mode"], m)
        assert run["marks"][0] is not None, "no arena access seen in " + run["label"]


@pytest.mark.parametrize("mode", ["outofplace", "inplace", "encrypt"])
def test_gcm(checked_lib, mode):
    """gcm_uniform for the three GCM_SESSIONS, gcm_mixed over GCM_FAMILIES
    and gcm_long_mixed (records up to 65532 bytes) in this mode, through each
    of the three designs (4 lanes, 8 lanes, burst; set_tuning inside the
    child)."""
    rep = _child(checked_lib, "gcm", mode)
    _assert_clean(rep)
    assert {r["label"].split(" ")[-1] for r in rep["runs"]} == {"lanes4", "lanes8", "burst"}


@pytest.mark.parametrize("mode", ["sign", "inplace", "outofplace"])
def test_ah(checked_lib, mode):
    """The ah_sweep_helpers layouts test_ah_sweep_gpu.py runs on the batch
    path: signing and both verifies."""
    _assert_clean(_child(checked_lib, "ah", mode))


def test_short_extent_is_reported_and_not_read(checked_lib):
    """A GCM icv8 uniform layout, the arena armed 32 bytes short: violations, all of them loads at record-load sites whose bytes lie
    between the armed end and the last record's end + 16; every record but
    the last still matches the oracle (the child asserts it) and the process
    exits normally."""
    rep = _child(checked_lib, "short-extent")
    assert len(rep["runs"]) == 1
    for run in rep["runs"]:
        assert run["violations"] > 0, "the checker saw nothing in " + run["label"]
        assert run["checked"] > 0
        assert all(run["load_sites"]), run["label"]
    for v in rep["first"]:
        assert v["kind"] == "read" and v["buf"] == 0, v
    for run in rep["runs"]:
        mine = [v for v in rep["first"] if v["bound"] == run["extent"]]
        assert mine
        for v in mine:
            assert run["extent"] + B.PAD - 16 <= v["at"] < run["last_end"] + B.PAD, (run["label"], v)
            assert v["at"] + v["bytes"] > run["extent"] + B.PAD, (run["label"], v)


def test_pad_marks_within_the_header_promise(checked_lib):
    """A measurement, recorded: the GCM uniform layouts and
    the tail layouts armed with pad 16; the high-water mark of access end -
    armed end per ICV length and mode.  A mark above 16 is a bug in
    the kernel or in the header."""
    rep = _child(checked_lib, "pad")
    _assert_clean(rep)
    table = {}
    for run in rep["runs"]:
        key = (run["kernel"], tuple(run["mlen"]), run["mode"])
        table[key] = max(table.get(key, -2**63), run["marks"][0])
    for (kernel, mlen, mode), mark in sorted(table.items()):
        print("pad: %s ICV %s %s: arena mark %d" % (kernel, list(mlen), mode, mark))
        assert mark <= B.PAD
