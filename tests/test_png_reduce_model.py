"""tests/png_reduce_model.py (numpy restatement of the reference's PNG reductions, filters through the PNG oracle) against
the vectors the REFERENCE's own wasm build made (tests/golden/make_golden_png_reduce.py): IHDR depth / colour type, PLTE and
tRNS bytes, filter byte of every row, the prepared stream and its Adler-32.  Pins the model, which then stands in where the
wasm export cannot go (reduce_palette off, single switches)."""
import numpy as np
import pytest

import oracle_lib as O
import png_reduce_cases as PC
import png_reduce_model as M

SMALL, BIG = PC.small(), [c for c in PC.CASES if c not in PC.small()]


def run(c):
    # the wasm build has no `parallel` feature: its preset 0 is the stateful AdaptiveFast
    stream, layout, adler = M.prepare(PC.make_input(c), c["w"], c["h"], c["color_type"], M.Opts.preset(c["preset"], M.NO_RAYON))
    PC.check(c, stream, layout, adler)


@pytest.mark.parametrize("c", SMALL, ids=[c["name"] for c in SMALL])
def test_model_reproduces_reference_vector(c):
    run(c)


@pytest.mark.parametrize("c", BIG, ids=[c["name"] for c in BIG])
def test_model_reproduces_reference_vector_4096(c):
    run(c)


def test_vectors_cover_the_branches_they_claim():
    names = {c["name"] for c in PC.CASES}
    assert len(names) == len(PC.CASES) >= 70
    assert {c["popular"] for c in PC.CASES} >= {"skip", "front", "back"}
    assert {(c["expect"]["ctype"], c["expect"]["depth"]) for c in PC.CASES} >= {(3, 1), (3, 2), (3, 4), (3, 8), (2, 8), (4, 8), (6, 8), (0, 8)}
    assert {c["expect"]["plte"] for c in PC.CASES} >= {1, 2, 3, 4, 5, 16, 17, 200, 256}
    assert any(c["w"] * c["h"] >= 4096 * 4096 for c in PC.CASES) and any((c["w"], c["h"]) == (1920, 1080) for c in PC.CASES)
    two = {(c["w"], c["h"]): c["filters"] for c in PC.CASES if c.get("n") == 2 and c["h"] == 64}
    assert set(two[(64, 64)]) == {"1"} and len(set(two[(128, 64)])) > 1 and len(two[(128, 64)]) == 64  # the area rule counts pixels


@pytest.mark.parametrize("bits,top", [(1, 1), (2, 3), (4, 15), (8, 200)])
@pytest.mark.parametrize("ct", [2, 3])
def test_gray_bit_depths_with_reduce_palette_off(ct, bits, top):
    """RGB / RGBA -> Gray at 1, 2, 4, 8 bits is reachable only with reduce_palette off (the wasm export cannot say that):
    checked against the definitions."""
    rng = np.random.RandomState(bits * 10 + ct)
    w, h = 37, 90
    g = rng.randint(0, top + 1, (h, w)).astype(np.uint8)
    g[0, 0] = top
    img = np.stack([g, g, g] + ([np.full_like(g, 255)] if ct == 3 else []), axis=2)
    res = M.reduce(img.reshape(-1), w, h, ct, M.Opts(O.S_NONE, True, True, False))
    assert (res["color_type_byte"], res["bit_depth"], res["bytes_per_pixel"]) == (0, bits, 1)
    rows = res["rows"]
    assert rows.shape == (h, (w * bits + 7) // 8)
    unpacked = np.unpackbits(rows, axis=1)[:, :w * bits].reshape(h, w, bits)
    assert np.array_equal(unpacked.dot(1 << np.arange(bits)[::-1]).astype(np.uint8), g)


def test_single_switches():
    rng = np.random.RandomState(5)
    w, h = 40, 30
    img = rng.randint(0, 256, (h, w, 4)).astype(np.uint8)
    img[:, :, 3][rng.rand(h, w) < 0.3] = 0
    px = img.reshape(-1)
    keep = M.reduce(px, w, h, 3, M.Opts())
    assert np.array_equal(keep["rows"].reshape(-1), px) and keep["color_type_byte"] == 6
    only_alpha = M.Opts(O.S_NONE, True, False, False)
    res = M.reduce(px, w, h, 3, only_alpha)
    M.optimize_alpha(res, only_alpha)
    out = res["rows"].reshape(h, w, 4)
    assert (out[img[:, :, 3] == 0][:, :3] == 0).all() and np.array_equal(out[img[:, :, 3] != 0], img[img[:, :, 3] != 0])
    few = img.copy()
    few[:, :, :] = few[0, :3, :][rng.randint(0, 3, (h, w))]
    res = M.reduce(few.reshape(-1), w, h, 3, M.Opts(O.S_NONE, True, False, True))  # palette first, never alpha-optimised
    assert res["color_type_byte"] == 3 and sorted(res["palette"]) == sorted({tuple(int(v) for v in p) for p in few.reshape(-1, 4)})
