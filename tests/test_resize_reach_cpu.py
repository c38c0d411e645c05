"""The claims of tests/resize_reach_cases.py, without a GPU: every case reaches the path it names (the launch arithmetic
restated in launch_shape, its spans held against the library's own contribution tables), the table as a whole covers the LDS
threshold from both sides at every pixel size, a second round of each of the three row loops and a side of 2^24, no vector of
tests/golden/resize_cases.json and no seeded random case of the GPU suite reaches any of that, and the recorded bytes are
those of the host-compiled kernel arithmetic and of the independent model."""
import hashlib

import numpy as np
import pytest

import emu_resize_lib as E
import resize_cases as RC
import resize_model as M
import resize_reach_cases as RR
from pixo_amd import resize

IDS = [c["name"] for c in RR.CASES]
LANCZOS = [c for c in RR.CASES if c["algorithm"] == RR.LANCZOS3]


@pytest.mark.parametrize("c", RR.CASES, ids=IDS)
def test_launch_shape_agrees_with_the_claim(c):
    s = RR.launch_shape(c)
    assert (s["staged_bytes"], s["use_lds"], s["h_tiles"]) == (c["staged_bytes"], c["use_lds"], c["h_tiles"]), c["name"]
    assert c["kernel"] in s["rounds"] and s["rounds"][c["kernel"]] == c["row_rounds"], (c["name"], s["rounds"])
    assert max(c["sw"], c["sh"], c["dw"], c["dh"]) <= RR.MAX_DIMENSION
    assert c["gen"] == "lcg" and len(RC.make_input(c)) == c["sw"] * c["sh"] * RR.bpp(c)


@pytest.mark.parametrize("c", LANCZOS, ids=[c["name"] for c in LANCZOS])
def test_spans_equal_those_of_the_library_tables(c):
    """launch_shape's taps are the ones the library builds its tables (and from them its span) with"""
    for src, dst in ((c["sw"], c["dw"]), (c["sh"], c["dh"])):
        starts, counts, _ = resize.contributions(src, dst)
        s, e = RR.taps(src, dst)
        assert np.array_equal(starts, s) and np.array_equal(counts, e - s), (c["name"], src, dst)


def test_row_rounds_at_the_cap():
    assert RR.row_rounds(262140, "point") == 1 and RR.row_rounds(262141, "point") == 2
    assert RR.row_rounds(65535, "lanczos_v") == 1 and RR.row_rounds(65536, "lanczos_v") == 2
    assert RR.row_rounds(1, "lanczos_h") == 1 and RR.row_rounds(RR.MAX_DIMENSION, "point") == 65


def test_the_table_covers_what_it_is_for():
    for ct, bpp in RC.BPP.items():
        of = [c for c in LANCZOS if c["color_type"] == ct]
        assert any(c["use_lds"] and c["staged_bytes"] == RR.SEG_BYTES for c in of), "no exactly full LDS case at %d bytes per pixel" % bpp
        assert any(not c["use_lds"] and RR.SEG_BYTES < c["staged_bytes"] <= RR.SEG_BYTES + 4 for c in of), \
            "no direct case just above the capacity at %d bytes per pixel" % bpp
    for kernel in RR.ROWS_PER_BLOCK:
        assert any(c["kernel"] == kernel and c["row_rounds"] >= 2 for c in RR.CASES), "no second round of the %s kernel" % kernel
    assert any(RR.MAX_DIMENSION in (c["sw"], c["sh"], c["dw"], c["dh"]) for c in RR.CASES)
    assert any(c["h_tiles"] == 2 and not c["use_lds"] and c["dw"] % RR.TILE for c in LANCZOS), "no direct case with a ragged second tile"
    assert len(set(IDS)) == len(IDS)


def _reaches(c):
    """The new paths a case takes: a list of words (empty: none of them)"""
    s = RR.launch_shape(c)
    out = [k + " round 2" for k, n in s["rounds"].items() if n >= 2]
    if s["use_lds"] is False:
        out.append("direct")
    if s["staged_bytes"] is not None and s["staged_bytes"] > RR.SEG_BYTES - 4:
        out.append("LDS full")
    if max(c["sw"], c["sh"], c["dw"], c["dh"]) > 1 << 23:
        out.append("side above 2^23")
    return out


def test_no_earlier_case_reaches_these_paths():
    """The proof of the gap: every golden vector and every seeded random case of tests/test_gpu_resize.py stays on LDS staging
    well below its capacity, within one round of every row loop, and below 2^23 on every side."""
    earlier = RC.ok_cases() + RC.random_cases(20261, 200)
    reached = {c["name"]: _reaches(c) for c in earlier}
    assert not {k: v for k, v in reached.items() if v}
    widest = max(RR.launch_shape(c)["staged_bytes"] or 0 for c in earlier)
    assert widest == 3396, widest  # (the largest staging any of them needs; the capacity is 8192)
    assert max(max(c["sw"], c["sh"], c["dw"], c["dh"]) for c in earlier) == 4096
    for c in RR.CASES:  # (group D only completes the call sequences of the GPU module)
        assert bool(_reaches(c)) == (c["group"] != "D"), c["name"]


def test_the_record_is_complete():
    g = RR.load_golden()
    assert sorted(g) == sorted(IDS)
    for c in RR.CASES:
        row = g[c["name"]]
        assert row["len"] == c["dw"] * c["dh"] * RR.bpp(c)
        assert ("hex" in row) == (row["len"] <= 64)
        if "hex" in row:
            assert hashlib.sha256(bytes.fromhex(row["hex"])).hexdigest() == row["sha256"]
    # a cap, not a tolerance: at most the one named case may go without the live model check below
    assert [n for n, row in g.items() if "model_checked_by" in row] == [RR.MAKER_ONLY]
    assert g[RR.MAKER_ONLY]["model_checked_by"] == "maker"


@pytest.mark.parametrize("c", RR.CASES, ids=IDS)
def test_host_compiled_kernel_arithmetic_gives_the_recorded_bytes(c):
    got = E.resize(RC.make_input(c), c["sw"], c["sh"], c["dw"], c["dh"], RR.bpp(c), c["algorithm"])
    row = RR.golden(c)
    assert len(got) == row["len"] and hashlib.sha256(got).hexdigest() == row["sha256"], c["name"]
    if "hex" in row:
        assert RC.first_difference(got, bytes.fromhex(row["hex"])) is None


MODELLED = [c for c in RR.CASES if c["name"] != RR.MAKER_ONLY]


@pytest.mark.parametrize("c", MODELLED, ids=[c["name"] for c in MODELLED])
def test_model_gives_the_recorded_bytes(c):
    assert len(MODELLED) == len(RR.CASES) - 1
    got = M.resize(RC.make_input(c), c["sw"], c["sh"], c["dw"], c["dh"], RR.bpp(c), c["algorithm"])
    row = RR.golden(c)
    assert len(got) == row["len"] and hashlib.sha256(got).hexdigest() == row["sha256"], c["name"]
