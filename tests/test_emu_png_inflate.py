"""The device inflate's walk (pixo_amd/csrc/png_inflate_math.h) on the host, no GPU: every case of tests/inflate_cases.py
against `zlib.decompress` and the host inflate (`decode.inflate_zlib`) for bytes, verdicts and Adler-32; the table build and the
decode against a canonical code worked out here; one step replayed lane by lane against a sequential copy loop; and the
stand-alone fuzz program (its own process, the host compiler's sanitizers where installed) over the cases and seeded corruptions."""
import subprocess
import zlib

import pytest

import emu_png_inflate_lib as E
import inflate_cases as IC
from pixo_amd import decode, error

K = E.constants()
CASES = IC.cases(**K)


def test_the_constants_are_the_librarys():
    assert K == dict(step_tokens=decode.inflate_step_tokens(), window_bytes=decode.inflate_window_bytes(),
                     far_distance=decode.inflate_far_distance(), stored_chunk=decode.inflate_stored_chunk())
    assert K["window_bytes"] == 32768 and K["far_distance"] == K["window_bytes"] - 258 * K["step_tokens"]


def test_the_cases_are_what_they_claim():
    """zlib and the host inflate on every case: the references agree with each other before the walk is held against them"""
    kinds = {c["kind"] for c in CASES}
    assert kinds == {"ok", "bad", "needs_host", "header"}
    for c in CASES:
        if c["kind"] == "ok":
            assert len(c["data"]) == c["expected"], c["name"]
            assert zlib.decompressobj(-15).decompress(c["z"][2:]) == c["data"] if c["zlib_refuses"] else zlib.decompress(c["z"]) == c["data"], c["name"]
            assert decode.inflate_zlib(c["z"], c["expected"]) == c["data"], c["name"]
        elif c["kind"] == "needs_host":
            with pytest.raises(zlib.error):
                zlib.decompress(c["z"])
            assert decode.inflate_zlib(c["z"], c["expected"]) == c["data"], c["name"]
        else:
            with pytest.raises(error.Error):
                decode.inflate_zlib(c["z"], c["expected"])


@pytest.mark.parametrize("c", [c for c in CASES if c["kind"] != "header"], ids=lambda c: c["name"])
def test_the_walk_on_every_case(c):
    r = E.inflate(c["z"], c["expected"])
    assert r["turns"] <= r["bound"], "more loop turns than the header's bound"
    assert r["produced"] <= c["expected"]
    assert r["adler"] == zlib.adler32(r["out"][:r["produced"]])  # the Adler-32 is that of the bytes produced, whatever the verdict
    assert r["out"][r["produced"]:] == b"\xa5" * (c["expected"] - r["produced"])  # nothing is written behind them
    if c["kind"] == "ok":
        assert r["verdict"] == E.OK and r["produced"] == c["expected"] and r["out"] == c["data"]
        assert r["adler"] == zlib.adler32(c["data"]) == int.from_bytes(c["z"][-4:], "big")
    elif c["kind"] == "needs_host":
        assert r["verdict"] == E.NEEDS_HOST and r["produced"] == 0
    else:
        assert r["verdict"] == E.FAILED


def test_a_wrong_size_keeps_the_bytes_that_fit():
    c = next(c for c in CASES if c["name"] == "expected_one_short")
    whole = zlib.decompress(c["z"])
    r = E.inflate(c["z"], c["expected"])
    assert r["verdict"] == E.FAILED and whole.startswith(r["out"][:r["produced"]])
    r = E.inflate(c["z"], len(whole) + 1)
    assert r["verdict"] == E.FAILED and r["produced"] == len(whole) and r["out"][:-1] == whole  # the final block ended one byte early


def canonical_lookup(lengths, bits, max_len=15):
    """RFC 1951 3.2.2 restated: the (symbol, length) whose code the bits start with, first code bit lowest"""
    codes = IC.canonical({s: n for s, n in enumerate(lengths) if n})
    for s, (code, n) in codes.items():
        if n <= max_len and all(((bits >> i) & 1) == ((code >> (n - 1 - i)) & 1) for i in range(n)):
            return s, n
    return None


def test_table_build_and_decode():
    fixed = [8] * 144 + [9] * 112 + [7] * 24 + [8] * 8
    skew = [n + 1 for n in range(12)] + [13, 14, 15, 15]  # complete, up to 15 bits
    incomplete = [0, 2, 0, 3, 3, 0, 11, 15]
    one = [0, 0, 1]
    for lengths in (fixed, skew, incomplete, one, [5] * 32):
        lut = E.build(lengths)
        assert lut is not None
        for j in list(range(0, 1024, 7)) + [1023]:
            want = canonical_lookup(lengths, j, 10)
            assert lut[j] == (want[0] | want[1] << 12 if want else 0), (lengths[:4], j)
        for bits in list(range(0, 32768, 251)) + [32767, 0x5555, 0x2AAA]:
            assert E.decode(lengths, bits) == canonical_lookup(lengths, bits), (lengths[:4], bits)
    # Kraft sums above 1 are the host's; exactly 1 and below are decoded
    assert E.build([1, 1, 1]) is None and E.build([1, 2, 2, 15]) is None and E.build([2, 2, 2, 2, 1]) is None
    assert E.build([1, 2, 2]) is not None and E.build([0] * 30) is not None and E.decode([0] * 30, 0) is None
    L = E.lib()
    import ctypes as C
    e = C.c_uint32()
    assert [(L.emu_pngi_length_base(c, C.byref(e)), e.value) for c in range(29)] == list(zip(IC.LENGTH_BASE, IC.LENGTH_EXTRA))
    assert [(L.emu_pngi_distance_base(d, C.byref(e)), e.value) for d in range(30)] == list(zip(IC.DIST_BASE, IC.DIST_EXTRA))
    assert [L.emu_pngi_code_length_order(i) for i in range(19)] == IC.CL_ORDER


def test_a_step_lane_by_lane_equals_a_sequential_copy():
    W, far, step = K["window_bytes"], K["far_distance"], K["step_tokens"]
    for d in (1, 2, 3, 63, 64, 65, 300):
        assert [E.lib().emu_pngi_match_source(i, d) for i in range(258)] == [i % d if d < 64 else i for i in range(258)]
    prefix = IC.lcg(W + 1000, 41)
    steps = [
        [1, 2, 3, (3, 3), (4, 2), (258, 1), (258, 7), 9, (17, 1), (64, 64), (65, 64), (130, 63), (100, 300)],
        list(IC.lcg(step, 42)),
        [(258, W)] * step,                                   # the most a step produces, from exactly a window back
        [(258, far)] + [200] * (step - 1),                    # the farthest match that may have literals behind it in its step
        [7] * (step - 1) + [(258, W - 3)],                   # ... a farther one is the last of its step
        [(3, 1), (3, 2), (3, 3), (4, 3), (5, 4), (258, 255), (258, 256), (258, 257), (258, 258), (258, 259)],
        [(200, 5000), 1, (200, 199), 2, (200, 200), 3, (200, 201), (258, 128), (258, 65)],
    ]
    for cut in (len(prefix), W, W - 1, 777, 5):  # how much output lies in front of the step (and where in the ring it starts)
        for tokens in steps:
            if any(not isinstance(t, int) and t[1] > cut for t in tokens):
                continue
            assert E.step(prefix[:cut], tokens) == IC.run_tokens(tokens, prefix[:cut]), (cut, tokens[:3])


def test_the_fuzz_program(tmp_path):
    E.lib()  # (builds it)
    corpus = tmp_path / "corpus.bin"
    E.write_corpus(corpus, [(c["z"], c["expected"]) for c in CASES])
    r = subprocess.run([E.FUZZ, str(corpus), "40"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "fuzz_main ok" in r.stdout
    print(r.stdout.strip())
