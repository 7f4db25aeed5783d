"""The placement of test_high_offsets_gpu.py (high_offset_helpers.py), checked
without a GPU for every layout and both boundaries: the safety condition (no
offset with dropped or mis-extended high bits leaves the allocation), a long
record across the boundary, a quarter of the records wholly on each side,
relocated off4 values that fit 32 bits and differ from the layout's by exactly
base / 4."""
import numpy as np
import pytest

import ah_sweep_helpers as A
import high_offset_helpers as P
import sweep_helpers as S
from high_offset_helpers import AH_LAYOUTS, ETA_LAYOUTS, GCM_LAYOUTS

BOUNDARY = pytest.mark.parametrize("boundary", list(P.BOUNDARIES))


def place_of(name, boundary):
    """-> (the layout, its Place)"""
    if name in AH_LAYOUTS:
        lay = AH_LAYOUTS[name]()
        return lay, P.place_for_layout(lay, boundary)
    b = {**GCM_LAYOUTS, **ETA_LAYOUTS}[name]()
    return b, P.place_for_batch(b, boundary)


def test_sizes():
    assert P.ALLOC == 2**31 + 2**32 + 2**23 and P.GUARD == 2**31
    assert P.BOUNDARIES == {"sign": 2**31, "wrap": 2**32}
    # what the safety condition rests on
    assert P.SPAN >= 2**32 and P.GUARD >= 2**31
    assert P.PATTERN not in (S.OUT_FILL, A.OUT_FILL, 0, 0xEE, 0xFF)


@BOUNDARY
@pytest.mark.parametrize("name", list(GCM_LAYOUTS) + list(ETA_LAYOUTS) + list(AH_LAYOUTS))
def test_placement_of_every_layout(name, boundary):
    lay, pl = place_of(name, boundary)
    # the sizes the cases were chosen by
    assert 1024 <= len(pl.offs) <= 2048 and pl.size <= 1.6e6
    pl.check_safe()
    below, across, above = pl.check_geometry()
    assert below + across + above == len(pl.offs)
    d = pl.relocate(lay.descs)
    assert d.dtype == lay.descs.dtype and d["off4"].dtype == np.uint32
    assert (d["off4"].astype(np.int64) * 4 == lay.descs["off4"].astype(np.int64) * 4 + pl.base).all()
    for f in lay.descs.dtype.names:
        if f != "off4":
            assert (d[f] == lay.descs[f]).all()
    assert (pl.back(d["off4"]) == lay.descs["off4"]).all()
    assert lay.descs["off4"].max() < 2**28            # the layout itself was not changed
    # the boundary lies inside the window, the window inside the allocation
    assert pl.base % 128 == 0 and pl.base < pl.B < pl.base + pl.size <= P.SPAN - P.REACH
    # at "wrap" the offsets of the upper records do not fit 32 bits as bytes: what the case is for
    hi = d["off4"].astype(np.int64) * 4 >= 2**32
    assert hi.any() == (boundary == "wrap")
    # at both, some byte offset has bit 31 set
    assert ((d["off4"].astype(np.int64) * 4) & 2**31).any()


@BOUNDARY
@pytest.mark.parametrize("policy", [0, 1], ids=["auto", "recompute"])
def test_placement_of_the_stage_loop(policy, boundary):
    """The cleartext packets of test_esp_natt_gpu.end_to_end with their head
    and tail room: what the stage kernels may write."""
    from test_esp_natt_gpu import end_to_end_packets
    *_, head, tail, arena, rec = end_to_end_packets(policy)
    assert (head, tail) == (72, 49) and len(rec) == 200
    pl = P.place_for_packets(arena, rec, boundary, head, tail)
    assert (pl.offs >= 0).all() and (pl.offs + pl.lens <= len(arena)).all()
    pl.check_safe()
    below, across, above = pl.check_geometry()
    assert across >= 1 and below + across + above == 200
    r = pl.relocate(rec)
    assert (r["off4"].astype(np.int64) * 4 == rec["off4"].astype(np.int64) * 4 + pl.base).all()
    assert (r["len"] == rec["len"]).all() and (pl.back(r["off4"]) == rec["off4"]).all()
    assert pl.base < pl.B < pl.base + pl.size <= P.SPAN - P.REACH


def test_an_unsafe_placement_is_noticed():
    """check_safe sees a record whose truncated or sign-extended offset would
    leave an allocation without the guard or the room behind 2^32."""
    pl = P.Place("wrap", 8192, range(0, 5120, 1024), [1024] * 5)
    pl.check_safe()
    pl.check_geometry(quarter=True)
    guard, alloc = P.GUARD, P.ALLOC
    try:
        P.GUARD, P.ALLOC = 0, alloc - guard
        with pytest.raises(AssertionError, match="sign-extended"):
            pl.check_safe()
    finally:
        P.GUARD, P.ALLOC = guard, alloc
    with pytest.raises(AssertionError, match="across the boundary"):
        P.Place("sign", 4096, [0, 1024, 2048], [1024, 1024, 1024], cut=1024).check_geometry()
    with pytest.raises(AssertionError, match="below"):
        P.Place("sign", 1 << 16, [0] + list(range(1024, 9 * 1024, 1024)), [1024] * 9, cut=512).check_geometry()


def test_packed_slots():
    """The packed case: slot i of `out` at i * PACKED_STRIDE from the second
    allocation's start, the last PACKED_HIGH slots at 2^32 and beyond, every
    slot inside the allocation."""
    n = P.PACKED_N
    ends = np.arange(n, dtype=np.int64) * P.PACKED_STRIDE + P.PACKED_STRIDE
    assert ends[-1] <= P.ALLOC
    assert (ends - P.PACKED_STRIDE >= 2**32).sum() == P.PACKED_HIGH == 300
    assert P.PACKED_STRIDE == 65536 and n == 65536 + 300
