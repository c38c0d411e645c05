"""Resize cases chosen for the branches of pixo_amd/csrc/resize.hip that no golden vector and no seeded random case reaches:
the horizontal Lanczos3 pass without LDS staging (and the staging at exactly its capacity), a second round of each kernel's
row-stride loop, and sides at the documented maximum of 2^24.  Each case carries the path it claims and the quantities that
make the claim checkable; launch_shape() restates the launch arithmetic from its contract (a horizontal tile is 64 output
columns, grid.y is capped at 65535) and tests/test_resize_reach_cpu.py holds every claim against it without a GPU.  The
expected bytes (tests/golden/resize_reach_cases.json, made by tests/golden/make_golden_resize_reach.py) are recorded output of
the numpy model, confirmed by the host-compiled kernel arithmetic.  Test harness only."""
import hashlib
import json
import os

import numpy as np

import resize_cases as RC

F = np.float32
CASES_JSON = os.path.join(RC.GOLDEN, "resize_reach_cases.json")
TILE = 64            # output columns of one wavefront of the horizontal pass
SEG_BYTES = 8192     # LDS bytes of one staged source row segment
GRID_Y_CAP = 65535   # rows beyond grid.y * rows-per-block are reached by striding
ROWS_PER_BLOCK = {"point": 4, "lanczos_h": 4, "lanczos_v": 1}
MAX_DIMENSION = 1 << 24
NEAREST, BILINEAR, LANCZOS3 = 0, 1, 2


def _case(sw, sh, dw, dh, ct, algo, seed, kernel, path, staged_bytes=None, use_lds=None, row_rounds=1, h_tiles=None, group="A"):
    return dict(name="%s_%dx%d_to_%dx%d_c%d" % (RC.ALGO_NAMES[algo], sw, sh, dw, dh, ct), sw=sw, sh=sh, dw=dw, dh=dh, color_type=ct,
                algorithm=algo, gen="lcg", seed=seed, group=group, kernel=kernel, path=path, staged_bytes=staged_bytes,
                use_lds=use_lds, row_rounds=row_rounds, h_tiles=h_tiles)


def _threshold_pair(full_w, sh, dh, ct, seed):
    """dst_w = 1: the one tile spans the whole source row, so the staged size is sw * bpp + 8 exactly"""
    bpp = RC.BPP[ct]
    return [
        _case(full_w, sh, 1, dh, ct, LANCZOS3, seed, "lanczos_h", "LDS staging exactly full (a source offset of 3 fills the last dword)",
              staged_bytes=full_w * bpp + 8, use_lds=True, h_tiles=1),
        _case(full_w + 1, sh, 1, dh, ct, LANCZOS3, seed + 1, "lanczos_h", "direct loads, one pixel past the LDS capacity",
              staged_bytes=(full_w + 1) * bpp + 8, use_lds=False, h_tiles=1),
    ]


# ---- A. the LDS threshold and the direct path of resize_lanczos_h_kernel ---------------------------------------------------------
A_CASES = _threshold_pair(2046, 5, 3, 3, 3001) + _threshold_pair(2728, 5, 3, 2, 3003) + _threshold_pair(4092, 6, 2, 1, 3005) + \
    _threshold_pair(8184, 3, 2, 0, 3007) + [
    _case(20000, 6, 100, 5, 2, LANCZOS3, 3009, "lanczos_h", "direct loads, two tiles (the second ragged: 36 columns), src_h % 4 != 0",
          staged_bytes=39911, use_lds=False, h_tiles=2),
    _case(9000, 5, 70, 3, 3, LANCZOS3, 3010, "lanczos_h", "direct loads, two tiles (the second ragged: 6 columns)",
          staged_bytes=34212, use_lds=False, h_tiles=2),
    _case(300001, 2, 37, 2, 0, LANCZOS3, 3011, "lanczos_h", "direct loads, about 48,000 taps per output",
          staged_bytes=300009, use_lds=False, h_tiles=1),
    # the direct Rgba threshold case 2047x5 -> 1x3 with one dimension changed (2046x5 -> 1x3 above is the fourth)
    _case(2047, 5, 2, 3, 3, LANCZOS3, 3012, "lanczos_h", "direct loads, two outputs that each span the whole row",
          staged_bytes=8196, use_lds=False, h_tiles=1),
    _case(2047, 6, 1, 3, 3, LANCZOS3, 3013, "lanczos_h", "direct loads, a second workgroup of rows with 2 live rows of 4",
          staged_bytes=8196, use_lds=False, h_tiles=1),
    _case(2047, 5, 1, 2, 3, LANCZOS3, 3014, "lanczos_h", "direct loads, one output row fewer",
          staged_bytes=8196, use_lds=False, h_tiles=1),
]

# ---- B. a second round of each row-stride loop -------------------------------------------------------------------------------------
B_CASES = [
    _case(2, 3, 3, 262145, 2, NEAREST, 3020, "point", "point kernel, the second round holds one row", row_rounds=2, group="B"),
    _case(5, 7, 3, 262147, 0, BILINEAR, 3021, "point", "point kernel, the second round holds 7 rows", row_rounds=2, group="B"),
    _case(2, 262150, 5, 262149, 3, BILINEAR, 3022, "point", "point kernel, the second round holds 9 rows; source rows beyond 2^18", row_rounds=2,
          group="B"),
    _case(2, 262147, 3, 4, 1, LANCZOS3, 3023, "lanczos_h", "horizontal kernel, second round: the last workgroup has 3 live rows of 4 at its barriers",
          staged_bytes=12, use_lds=True, row_rounds=2, h_tiles=1, group="B"),
    # (each output of the case above averages some 390,000 rows, so its bytes hardly depend on the few rows of the second
    # round; here the last output row is made of the 67 rows of the second round and little else)
    _case(2, 262207, 3, 4096, 1, LANCZOS3, 3025, "lanczos_h", "horizontal kernel, second round of 67 rows (3 live rows of 4 in the last workgroup), "
          "384 vertical taps per output", staged_bytes=12, use_lds=True, row_rounds=2, h_tiles=1, group="B"),
    _case(5, 9, 3, 65541, 2, LANCZOS3, 3024, "lanczos_v", "vertical kernel, the second round holds 6 rows",
          staged_bytes=23, use_lds=True, row_rounds=2, h_tiles=1, group="B"),
]

# ---- C. sides at the documented maximum (gray, one row or one column) ------------------------------------------------------------------
C_CASES = [
    _case(MAX_DIMENSION, 1, MAX_DIMENSION - 1, 1, 0, NEAREST, 3030, "point", "2^24 source columns: d + 0.5 rounds to even above 2^23", group="C"),
    _case(MAX_DIMENSION - 1, 1, MAX_DIMENSION, 1, 0, BILINEAR, 3031, "point", "2^24 output columns", group="C"),
    _case(1, MAX_DIMENSION, 1, 9000001, 0, NEAREST, 3032, "point", "2^24 source rows, 35 rounds of the row loop", row_rounds=35, group="C"),
]

# ---- D. the other members of the call sequences on one shape (tests/test_gpu_resize_reach.py); none of them is a new path by itself ----
D_CASES = [
    _case(2047, 5, 1, 3, 0, LANCZOS3, 3040, "lanczos_h", "LDS staging; the shape of the direct Rgba case at 1 byte per pixel",
          staged_bytes=2055, use_lds=True, h_tiles=1, group="D"),
    _case(2047, 5, 1, 3, 2, LANCZOS3, 3041, "lanczos_h", "LDS staging; the shape of the direct Rgba case at 3 bytes per pixel",
          staged_bytes=6149, use_lds=True, h_tiles=1, group="D"),
    _case(2047, 5, 1, 3, 3, NEAREST, 3042, "point", "the shape of the direct Rgba case without tables", group="D"),
    _case(5, 2047, 3, 1, 3, LANCZOS3, 3043, "lanczos_h", "the direct Rgba case with its axes swapped: LDS staging, 2047 vertical taps",
          staged_bytes=28, use_lds=True, h_tiles=1, group="D"),
]

CASES = A_CASES + B_CASES + C_CASES + D_CASES
MAKER_ONLY = "lanczos3_5x9_to_3x65541_c2"  # the model needs about half a minute for it: the maker runs it, the suite does not


def by_name(name):
    return next(c for c in CASES if c["name"] == name)


# ---- the launch arithmetic, restated ----------------------------------------------------------------------------------------------------
def taps(src, dst):
    """(start, end) of every destination index of one Lanczos3 axis, f32 operation for operation (as
    resize_model.contributions; an empty range is end = start)"""
    scale = F(src) / F(dst)
    fs = max(scale, F(1))
    support = F(3) * fs
    d = np.arange(dst, dtype=np.int64)
    center = (d.astype(F) + F(0.5)) * scale - F(0.5)
    start = np.maximum(np.floor(center - support).astype(np.int64), 0)
    end = np.minimum(np.maximum(np.ceil(center + support).astype(np.int64), 0) + 1, src)
    return start, np.maximum(end, start)


def max_span(start, end):
    """The widest source span of one tile: from the start of the tile's first column to the furthest end seen in the tile"""
    span = 0
    for lo in range(0, len(start), TILE):
        span = max(span, int((end[lo:lo + TILE] - start[lo]).max()))
    return span


def row_rounds(rows, kernel):
    per = ROWS_PER_BLOCK[kernel]
    grid_y = min(-(-rows // per), GRID_Y_CAP)
    return -(-rows // (grid_y * per))


def launch_shape(c):
    """What the launches of this case look like: `rounds` per kernel launched, and for Lanczos3 the staged size of the widest
    tile (max_span * bpp + 8: up to 3 bytes of alignment in front, stored in whole dwords), whether it fits the LDS segment,
    and the number of horizontal tiles"""
    if c["algorithm"] != LANCZOS3:
        return dict(staged_bytes=None, use_lds=None, h_tiles=None, rounds={"point": row_rounds(c["dh"], "point")})
    staged = max_span(*taps(c["sw"], c["dw"])) * RC.BPP[c["color_type"]] + 8
    return dict(staged_bytes=staged, use_lds=staged <= SEG_BYTES, h_tiles=-(-c["dw"] // TILE),
                rounds={"lanczos_h": row_rounds(c["sh"], "lanczos_h"), "lanczos_v": row_rounds(c["dh"], "lanczos_v")})


# ---- expected bytes ------------------------------------------------------------------------------------------------------------------------
def load_golden():
    with open(CASES_JSON) as f:
        return {g["name"]: g for g in json.load(f)}


_GOLDEN = None


def golden(c):
    global _GOLDEN
    if _GOLDEN is None:
        _GOLDEN = load_golden()
    return _GOLDEN[c["name"]]


def bpp(c):
    return RC.BPP[c["color_type"]]


def check(c, got, what="") -> None:
    """Asserts that `got` is the case's recorded output.  The message names the case and the first differing index: short
    outputs are stored, for the others the host-compiled arithmetic (which the CPU suite holds to the same hash) is run on a
    mismatch to say where."""
    got = bytes(got)
    g = golden(c)
    label = c["name"] + (" " + what if what else "")
    assert len(got) == g["len"], "%s: length %d != %d" % (label, len(got), g["len"])
    if "hex" in g:
        diff = RC.first_difference(got, bytes.fromhex(g["hex"]))
        assert diff is None, "%s: %s" % (label, diff)
    if hashlib.sha256(got).hexdigest() != g["sha256"]:
        import emu_resize_lib as E
        want = E.resize(RC.make_input(c), c["sw"], c["sh"], c["dw"], c["dh"], bpp(c), c["algorithm"])
        where = RC.first_difference(got, want) if hashlib.sha256(want).hexdigest() == g["sha256"] else "the host arithmetic differs from the record too"
        raise AssertionError("%s: sha256 differs (%s)" % (label, where))
