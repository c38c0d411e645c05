"""The resize golden cases (tests/golden/resize_cases.json, made by tests/golden/make_golden_resize.py with the reference's
own wasm build): their inputs by generator name and seed, their expected bytes, and the live-wasm runner.  Test harness only."""
import hashlib
import json
import os
import shutil
import subprocess
import tempfile

import numpy as np

import synth

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
GOLDEN = os.path.join(HERE, "golden")
CASES_JSON = os.path.join(GOLDEN, "resize_cases.json")
WASM = os.path.join(ROOT, "oracle", "_ref", "pixo_bg.wasm")
LOADER = os.path.join(HERE, "ref_resize_wasm.js")
BPP = {0: 1, 1: 2, 2: 3, 3: 4}
ALGO_NAMES = {0: "nearest", 1: "bilinear", 2: "lanczos3"}


def make_input(c) -> np.ndarray:
    """The case's source pixels: `gen` names a tests/synth.py generator (seeded)."""
    w, h, ct, gen, seed = c["sw"], c["sh"], c["color_type"], c["gen"], c.get("seed", 42)
    if gen == "bytes":  # error cases: `data_len` arbitrary bytes
        return synth.lcg_bytes(c["data_len"], seed)
    n = w * h * BPP[ct]
    if gen == "lcg":  # every colour type
        return synth.lcg_bytes(n, seed)
    if gen == "noise" and ct == 2:
        return synth.noise(w, h, seed)
    if gen == "noise" and ct == 0:
        return synth.noise_gray(w, h, seed)
    if gen == "photo" and ct == 2:
        return synth.photo(w, h, seed)
    if gen == "gradient" and ct == 2:
        return synth.gradient_rgb(w, h)
    if gen == "checkerboard" and ct == 2:
        return synth.checkerboard(w, h)
    if gen == "rgba_noise" and ct == 3:
        return synth.rgba_noise_alpha1(w, h, seed)
    raise ValueError("no generator %r for colour type %d" % (gen, ct))


def load_cases():
    with open(CASES_JSON) as f:
        return json.load(f)


def ok_cases():
    return [c for c in load_cases() if "error" not in c]


def error_cases():
    return [c for c in load_cases() if "error" in c]


def expected_bytes(c):
    """The stored output of a small case, or None (large cases carry sha256 + len only)."""
    if not c.get("file"):
        return None
    with open(os.path.join(GOLDEN, c["file"]), "rb") as f:
        return f.read()


def first_difference(got: bytes, want: bytes):
    a, b = np.frombuffer(got, np.uint8), np.frombuffer(want, np.uint8)
    if a.size != b.size:
        return "length %d != %d" % (a.size, b.size)
    d = np.flatnonzero(a != b)
    return None if d.size == 0 else "%d byte(s) differ, first at index %d: got %d, want %d" % (d.size, d[0], a[d[0]], b[d[0]])


def check(c, got) -> None:
    """Asserts that `got` is the case's golden output; the message names the case and the first differing index."""
    got = bytes(got)
    want = expected_bytes(c)
    if want is not None:
        diff = first_difference(got, want)
        assert diff is None, "%s: %s" % (c["name"], diff)
    assert len(got) == c["len"], "%s: length %d != %d" % (c["name"], len(got), c["len"])
    assert hashlib.sha256(got).hexdigest() == c["sha256"], "%s: sha256 differs (%d bytes; the expected bytes are not stored)" % (c["name"], len(got))


def have_live_wasm() -> bool:
    return os.path.exists(WASM) and shutil.which("node") is not None


def run_wasm(cases, inputs=None, repeat=1, timeout=1200):
    """Runs `cases` through the reference's wasm under node: a list of (bytes | None, error | None, ms list)."""
    with tempfile.TemporaryDirectory() as tmp:
        man = []
        for i, c in enumerate(cases):
            src = inputs[i] if inputs is not None else make_input(c)
            p = os.path.join(tmp, "in%d.bin" % i)
            np.ascontiguousarray(src, np.uint8).tofile(p)
            man.append(dict(input=p, output=os.path.join(tmp, "out%d.bin" % i), repeat=repeat,
                            **{k: c[k] for k in ("sw", "sh", "dw", "dh", "color_type", "algorithm")}))
        mp = os.path.join(tmp, "manifest.json")
        with open(mp, "w") as f:
            json.dump({"wasm": WASM, "cases": man}, f)
        out = subprocess.run(["node", LOADER, mp], stdout=subprocess.PIPE, check=True, timeout=timeout).stdout.decode()
        res = []
        for m, line in zip(man, out.strip().splitlines()):
            r = json.loads(line)
            if r["ok"]:
                with open(m["output"], "rb") as f:
                    res.append((f.read(), None, r["ms"]))
            else:
                res.append((None, r["error"], []))
        assert len(res) == len(cases), out[-2000:]
        return res


def random_cases(seed: int, count: int, max_side: int = 2048, max_pixels: int = 1 << 19):
    """`count` seeded random cases: sides log-uniform in [1, max_side] (areas capped so that the model stays quick), all colour
    types and algorithms; every eighth case keeps dst = src, every fifth has a one-pixel axis."""
    rng = np.random.RandomState(seed)

    def side():
        return int(min(max_side, max(1, round(2.0 ** rng.uniform(0, np.log2(max_side))))))

    def pair():
        w, h = side(), side()
        while w * h > max_pixels:
            w, h = max(1, w // 2), max(1, h // 2)
        return w, h

    out = []
    for i in range(count):
        (sw, sh), (dw, dh) = pair(), pair()
        if i % 8 == 3:
            dw, dh = sw, sh
        if i % 5 == 1:
            which = rng.randint(4)
            sw, sh, dw, dh = [1 if which == k else v for k, v in enumerate((sw, sh, dw, dh))]
        ct, algo = int(rng.randint(4)), int(rng.randint(3))
        out.append(dict(name="random%d_%d_%s_%dx%d_to_%dx%d_c%d" % (seed, i, ALGO_NAMES[algo], sw, sh, dw, dh, ct),
                        sw=sw, sh=sh, dw=dw, dh=dh, color_type=ct, algorithm=algo, gen="lcg", seed=1000 + i))
    return out
