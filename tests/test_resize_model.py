"""The independent numpy model of resize (tests/resize_model.py) pinned to every vector made by the reference's own wasm
build — no mismatch allowed — and, where node and the staged wasm are present, to the live wasm on seeded random shapes."""
import numpy as np
import pytest

import resize_cases as RC
import resize_model as M

OK = RC.ok_cases()


@pytest.mark.parametrize("c", OK, ids=[c["name"] for c in OK])
def test_model_reproduces_golden(c):
    RC.check(c, M.resize(RC.make_input(c), c["sw"], c["sh"], c["dw"], c["dh"], RC.BPP[c["color_type"]], c["algorithm"]))


def test_golden_list_covers_what_it_must():
    assert len(RC.load_cases()) >= 150
    assert {(c["algorithm"], c["color_type"]) for c in OK} == {(a, ct) for a in range(3) for ct in range(4)}
    for a in range(3):
        mine = [c for c in OK if c["algorithm"] == a]
        assert any((c["sw"], c["sh"]) == (1, 1) and c["dw"] * c["dh"] > 1 for c in mine)
        assert any((c["dw"], c["dh"]) == (1, 1) and c["sw"] * c["sh"] > 1 for c in mine)
        assert any((c["sw"], c["sh"]) == (c["dw"], c["dh"]) for c in mine)
        assert any(c["sw"] == c["dw"] and c["sh"] != c["dh"] for c in mine)
        assert any(c["sw"] > 8 * c["dw"] and c["sh"] > 8 * c["dh"] for c in mine)
        assert any(c["dw"] > 6 * c["sw"] and c["dh"] > 6 * c["sh"] for c in mine)
        assert any((c["sw"], c["sh"], c["dw"], c["dh"]) == (1920, 1080, 640, 360) for c in mine)
        assert any((c["sw"], c["sh"], c["dw"], c["dh"], c["color_type"]) == (4096, 4096, 1024, 1024, 2) for c in mine)


def test_sinf_is_the_f64_polynomial_form():
    # values where one rounding of an f64 result decides: sin is odd, exact at 0, and close to libm everywhere in range
    x = np.linspace(-9.5, 9.5, 20001).astype(np.float32)
    s = M.sinf(x)
    assert np.array_equal(s, -M.sinf(-x))
    assert M.sinf(np.float32([0.0]))[0] == 0.0
    assert np.max(np.abs(s.astype(np.float64) - np.sin(x.astype(np.float64)))) < 6e-8  # half an ulp of values below 1


@pytest.mark.skipif(not RC.have_live_wasm(), reason="needs node and oracle/_ref/pixo_bg.wasm")
def test_model_against_the_live_wasm():
    cases = RC.random_cases(777, 60, max_side=512, max_pixels=512 * 512)
    inputs = [RC.make_input(c) for c in cases]
    bad = []
    for c, px, (want, err, _) in zip(cases, inputs, RC.run_wasm(cases, inputs)):
        assert err is None, (c["name"], err)
        diff = RC.first_difference(M.resize(px, c["sw"], c["sh"], c["dw"], c["dh"], RC.BPP[c["color_type"]], c["algorithm"]), want)
        if diff:
            bad.append("%s: %s" % (c["name"], diff))
    assert not bad, "\n".join(bad)
