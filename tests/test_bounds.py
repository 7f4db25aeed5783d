"""The bounds-checked build (f-stack_amd `make checked`, csrc/bounds_chk.h)
as far as it can be pinned without a GPU: the extent bounds_child.py arms
with, the room every layout of the GPU cases leaves for it, the build itself,
the default library's symbols, and that no global-memory access of the two
instrumented kernel files goes round the accessor layer."""
import os
import re
import subprocess

import numpy as np
import pytest

import bounds_child as B
from helpers import DESC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "f-stack_amd")
CSRC = os.path.join(PKG, "csrc")


def _descs(rows):
    d = np.zeros(len(rows), dtype=DESC)
    for i, (off4, ln) in enumerate(rows):
        d[i]["off4"], d[i]["len"] = off4, ln
    return d


# ---- the armed extent ------------------------------------------------------------

def test_extent_is_the_largest_record_end():
    assert B.armed_extent(_descs([(0, 40), (10, 64), (26, 100)])) == 204


def test_extent_of_unsorted_offsets():
    """The last descriptor is not the last record."""
    assert B.armed_extent(_descs([(100, 48), (0, 48), (500, 16), (30, 1500)])) == 2016
    assert B.armed_extent(_descs([(30, 1500), (500, 16)])) == 2016


def test_extent_counts_a_malformed_longer_len():
    """A descriptor whose len says more than the record holds (len_delta +2 in
    the sweeps) is read by the kernels as it stands: the header's contract
    covers it, so the extent does."""
    rows = [(0, 40), (10, 64), (26, 100)]
    longer = [(0, 40), (10, 64 + 200), (26, 100)]
    assert B.armed_extent(_descs(longer)) == 40 + 264
    assert B.armed_extent(_descs(rows[:2] + [(26, 102)])) == 206


def test_extent_of_one_record_and_of_len_zero():
    assert B.armed_extent(_descs([(7, 36)])) == 64
    assert B.armed_extent(_descs([(7, 0)])) == 28
    assert B.armed_extent(_descs([(0, 65535)])) == 65535           # (len is 16 bits; off4 * 4 does not wrap)
    assert B.armed_extent(_descs([(0x3fffffff, 65535)])) == 0xfffffffc + 65535


def test_extent_of_ah_byte_lengths():
    """AH records have any byte length: the extent is not rounded to 4."""
    assert B.armed_extent(_descs([(4, 13), (9, 31)])) == 67
    assert B.armed_extent(_descs([(4, 13), (9, 1)])) == 37


# ---- a condition on the inputs of the GPU cases ----------------------------------

@pytest.mark.parametrize("family", list(B.FAMILIES))
def test_every_layout_leaves_room_for_extent_and_pad(family):
    """bounds_child.py arms extent + 16 for reads; check() builds the arena
    tensor from the layout's own array.  If a layout ever armed past its
    tensor, a read the checker allows could leave the allocation: pinned here
    for every layout of every case, so a later layout cannot do so quietly.
    (build_records and ah_sweep_helpers.Layout leave 64 bytes; a malformed
    len adds at most 2.)"""
    seen = set()
    for label, which, thunk, mode, grouped, design in B.runs_of(family):
        key = label.split(" ")[0]
        if key in seen:
            continue
        seen.add(key)
        lay = thunk()
        ext = B.armed_extent(B.layout_descs(lay))
        have = B.layout_arena_bytes(lay, which)
        assert ext + B.PAD <= have, "%s: extent %d + %d > arena %d" % (label, ext, B.PAD, have)
        assert ext > 0 and lay.n == len(B.layout_descs(lay))
    assert seen


def test_the_families_cover_their_layouts():
    import ah_sweep_helpers as A
    import sweep_helpers as S
    gcm = B.runs_of("gcm")
    assert len(gcm) == 3 * 3 * (len(S.GCM_SESSIONS) + len(S.GCM_FAMILIES) + 1)
    assert len([r for r in gcm if r[0].startswith("gcm_long_mixed ")]) == 3 * 3
    assert not any("long_uniform" in r[0] for fam in B.FAMILIES for r in B.runs_of(fam))
    assert {r[5][0] for r in gcm} == {"lanes4", "lanes8", "burst"}
    ah = B.runs_of("ah")
    assert len(ah) == 3 * 3 * len(A.HASH_ESN) + 3 + 6 + 1 + 3
    assert {r[3] for r in ah} == set(A.MODES)
    for fam, mode in (("gcm", "inplace"), ("gcm", "encrypt"), ("ah", "sign")):
        part = B.runs_of(fam, mode)
        assert part and all(r[3] == mode for r in part)
    assert sum(len(B.runs_of("gcm", m)) for m in ("outofplace", "inplace", "encrypt")) == len(gcm)
    pad = B.runs_of("pad")
    assert len([r for r in pad if r[0].startswith("gcm_tail")]) == 3 * 3 * len(S.GCM_SESSIONS) * 4
    # no family launches the ETA kernels (esp_cbc.hip is not instrumented)
    for fam in B.FAMILIES:
        for label, which, thunk, mode, grouped, design in B.runs_of(fam):
            assert label.startswith(("gcm_", "ah_")), label


# ---- the build and the default library -------------------------------------------

@pytest.fixture(scope="module")
def checked_lib():
    subprocess.run(["make", "-s", "-C", PKG, "-j8", "checked"], check=True, timeout=900, stdout=subprocess.DEVNULL)
    return os.path.join(PKG, "libespgpu_chk.so")


def _symbols(path):
    out = subprocess.run(["nm", "-D", "--defined-only", path], check=True, capture_output=True, text=True).stdout
    return {ln.split()[-1] for ln in out.splitlines() if ln.strip()}


def test_make_checked_builds_without_a_gpu(checked_lib):
    syms = _symbols(checked_lib)
    assert {"espgpu_chk_arm", "espgpu_chk_report", "espgpu_chk_reset"} <= syms
    assert "espgpu_decrypt_batch" in syms and "espgpu_abi_version" in syms


def test_default_library_exports_no_checker_symbol():
    syms = _symbols(os.path.join(PKG, "libespgpu.so"))
    assert "espgpu_decrypt_batch" in syms
    assert not [s for s in syms if "espgpu_chk_" in s]
    hdr = open(os.path.join(ROOT, "include", "espgpu.h")).read()
    assert "espgpu_chk_" not in hdr and "ESPGPU_BOUNDS" not in hdr


def test_report_layout_matches_the_header():
    """bounds_child.py reads the report with ctypes: the sizes bounds_chk.h implies."""
    import ctypes as C
    src = open(os.path.join(CSRC, "bounds_chk.h")).read()
    assert int(re.search(r"kChkKeep = (\d+);", src).group(1)) == B.KEEP
    assert C.sizeof(B.Violation) == 40 and C.sizeof(B.Report) == 32 + 40 * B.KEEP
    kinds = re.findall(r"^\s+CHK_([A-Z]+) = (\d+),", src, re.M)
    assert [k.lower() for k, _ in kinds] == B.KINDS and [int(v) for _, v in kinds] == list(range(len(B.KINDS)))
    for tag, name in B.FILE_TAGS.items():
        assert re.search(r"^#define ESPGPU_CHK_TAG %d\b" % tag, open(os.path.join(CSRC, name)).read(), re.M)


# ---- no access goes round the accessor layer -------------------------------------

KERNEL_FILES = ("esp_gcm.hip", "esp_ah.hip")

# reinterpret_casts that stay in the kernel files: (file, text the line contains, why it is not a
# record-derived global access)
ALLOWED_CASTS = [
    ("esp_gcm.hip", "(lds + a", "LDS: the T-table pair"),
    ("esp_gcm.hip", "(lds + LDS_GT + ea)", "LDS: the 8-bit GHASH table"),
    ("esp_gcm.hip", "(lds + LDS_TP + x * 256", "LDS: the T-table fill"),
    ("esp_gcm.hip", "(t + (2 * q", "the GHASH power table of the SA (gtab): a ctx table, not record-derived"),
    ("esp_gcm.hip", "(scratch)[i] = reinterpret_cast<const uint4 *>(t4)[i]", "gtab to LDS scratch: a ctx table"),
    ("esp_gcm.hip", "(scratch + (2 * q", "LDS scratch"),
    ("esp_gcm.hip", "(dst + (v * 16 + q) * 16)", "LDS: the expanded GHASH table"),
    ("esp_gcm.hip", "const uint32_t *q = reinterpret_cast<const uint32_t *>(rec + len - mlen);",
     "an address only: the ICV dwords are read through esp_ld4w(q, k)"),
    ("esp_gcm.hip", "(p.hdesc + start)", "stage_in: host memory, out of scope"),
    ("esp_gcm.hip", "(const_cast<espgpu_desc *>(p.desc) + start)", "stage_in: the staging copy, out of scope"),
    ("esp_gcm.hip", "(&a.ctl->", "the doorbell kernel: host memory, out of scope"),
    ("esp_gcm.hip", "p.desc = reinterpret_cast<const espgpu_desc *>(sl.arena + sl.desc_off);",
     "the doorbell kernel: an address only"),
    ("esp_gcm.hip", "p.hdesc = reinterpret_cast<const espgpu_desc *>(sl.hdesc);", "the doorbell kernel: an address only"),
    ("esp_gcm.hip", "reinterpret_cast<hipStream_t>(stream)", "host code: the stream handle"),
    ("esp_ah.hip", "reinterpret_cast<hipStream_t>(stream)", "host code: the stream handle"),
]

# a per-record array, the chunk list or the SA table indexed or offset directly; a record pointer, the
# arena, out or the E_K(J0) scratch indexed
RAW_INDEX = re.compile(r"\bp\.(desc|status|trailer|order|chunks|sas)\s*(\[|\+)|\b(rec|orec|dst|q)\s*\[|"
                       r"\bp\.(arena|out|icv_out|ej0)\s*\[")
ALLOWED_RAW = [
    ("esp_gcm.hip", "(const_cast<espgpu_desc *>(p.desc) + start)", "stage_in, as above"),
    ("esp_gcm.hip", "uint32_t o[4], q[4];", "a local array of the AES round (registers)"),
    ("esp_gcm.hip", "q[col] = xor3(", "the same local array"),
    ("esp_gcm.hip", "u0 = q[0], u1 = q[1], u2 = q[2], u3 = q[3];", "the same local array"),
    ("esp_gcm.hip", "kb = make_uint4(q[0], q[1], q[2], q[3]);", "the same local array"),
    ("esp_gcm.hip", "p.ej0[di]", "the burst kernel's E_K(J0) scratch: sized by run_batch for n, indexed by a checked "
                                 "descriptor index; not record-derived, out of scope"),
]


def _code_lines(name):
    for no, ln in enumerate(open(os.path.join(CSRC, name)).read().splitlines(), 1):
        code = ln.split("//")[0]
        if code.strip():
            yield no, code


def test_every_entry_of_the_allow_lists_has_a_reason_and_a_line():
    for f, text, why in ALLOWED_CASTS + ALLOWED_RAW:
        assert why.strip()
        assert any(text in code for _, code in _code_lines(f)), "stale allow-list entry: %s: %s" % (f, text)


@pytest.mark.parametrize("name", KERNEL_FILES)
def test_no_cast_of_a_global_pointer_outside_the_accessor_layer(name):
    bad = []
    for no, code in _code_lines(name):
        if "reinterpret_cast" in code and not any(f == name and t in code for f, t, _ in ALLOWED_CASTS):
            bad.append("%s:%d: %s" % (name, no, code.strip()))
        if RAW_INDEX.search(code) and not any(f == name and t in code for f, t, _ in ALLOWED_RAW):
            bad.append("%s:%d: %s" % (name, no, code.strip()))
    assert not bad, "global-memory accesses outside dev_prims.h's helpers (or add to the allow-list, with a reason):\n" + \
        "\n".join(bad)


def test_the_source_check_sees_a_raw_access():
    """The patterns above do flag what they are for."""
    for line in ("  v = bswap32(*reinterpret_cast<const uint32_t *>(rec + o));", "  p.status[di] = ESPGPU_EINVAL;",
                 "  const DevSA *s = p.sas + sa;", "  const uint4 dv = *reinterpret_cast<const uint4 *>(p.desc + di);",
                 "      if (mlen > 8) tag.z = q[2];", "  const uint8_t b = rec[o];", "  p.arena[off] = 0;",
                 "  dst[4 * k] = v;"):
        flagged = ("reinterpret_cast" in line and not any(t in line for _, t, _ in ALLOWED_CASTS)) or \
            (RAW_INDEX.search(line) and not any(t in line for _, t, _ in ALLOWED_RAW))
        assert flagged, line


def test_the_helpers_are_checked_in_the_checked_build():
    """dev_prims.h routes every helper to the checked accessors under ESPGPU_BOUNDS."""
    src = open(os.path.join(CSRC, "dev_prims.h")).read()
    chk = src.split("#else", 1)[1].split("#endif", 1)[0] + src.split("#define CHK_SITE", 1)[1]
    for h in ("ld16", "st16", "st8", "st_partial", "esp_ld4", "esp_st4", "esp_ld4w", "esp_at_ld", "esp_at_st",
              "esp_at_ptr", "esp_desc_ld16"):
        assert re.search(r"^#define %s\(.*\) chk_" % h, chk, re.M), h
