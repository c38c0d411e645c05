#!/usr/bin/env python3
"""Generate the resize golden vectors with the REFERENCE's own code.

Runs `resizeImage` of the reference's compiled WebAssembly build (oracle/_ref/pixo_bg.wasm) under node via
tests/ref_resize_wasm.js on deterministic inputs (tests/synth.py generators by name and seed: no input files are stored) and
writes tests/golden/resize_cases.json: per case the shape, colour type, algorithm, generator, and sha256 + length of the
output; outputs of small cases are stored verbatim under tests/golden/resize/.  The reference's error strings are cases too.
Build container only (needs node + the staged wasm).

    python tests/golden/make_golden_resize.py
"""
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import resize_cases as RC  # noqa: E402

STORE_LIMIT = 12000  # output bytes stored verbatim


def case(sw, sh, dw, dh, ct, algo, gen="lcg", seed=7):
    return dict(name="%s_%dx%d_to_%dx%d_c%d_%s_s%d" % (RC.ALGO_NAMES[algo], sw, sh, dw, dh, ct, gen, seed),
                sw=sw, sh=sh, dw=dw, dh=dh, color_type=ct, algorithm=algo, gen=gen, seed=seed)


def cases():
    out = []
    # every algorithm x every colour type over: up-scale, down-scale, identity, one axis only, 1x1 -> n, n -> 1x1,
    # prime sizes up by more than 6x, down by more than 8x
    shapes = [(37, 23, 64, 41), (64, 48, 17, 13), (31, 31, 31, 31), (53, 47, 53, 20), (1, 1, 9, 7), (9, 7, 1, 1),
              (7, 5, 53, 43), (200, 150, 20, 15)]
    for (sw, sh, dw, dh) in shapes:
        for algo in (0, 1, 2):
            for ct in (0, 1, 2, 3):
                out.append(case(sw, sh, dw, dh, ct, algo, "lcg", 7 + ct))
    for algo in (0, 1, 2):
        # named generators: smooth content, ramps, hard edges
        out.append(case(160, 120, 61, 47, 2, algo, "photo", 3))
        out.append(case(96, 64, 211, 97, 2, algo, "gradient", 0))
        out.append(case(64, 64, 23, 101, 2, algo, "checkerboard", 0))
        out.append(case(127, 61, 40, 40, 0, algo, "noise", 5))
        out.append(case(89, 97, 30, 300, 3, algo, "rgba_noise", 5))
        # one-pixel axes, mixed up/down, long thin images
        out.append(case(1, 64, 1, 16, 0, algo, "lcg", 11))
        out.append(case(64, 1, 200, 1, 3, algo, "lcg", 12))
        out.append(case(257, 3, 3, 257, 1, algo, "lcg", 13))
        out.append(case(1000, 2, 3, 5, 2, algo, "lcg", 14))
        out.append(case(300, 200, 2048, 1365, 2, algo, "photo", 9))
        out.append(case(640, 480, 1280, 960, 1, algo, "lcg", 15))
        # the sizes users run
        out.append(case(1920, 1080, 640, 360, 2, algo, "photo", 4))
        out.append(case(1920, 1080, 640, 360, 3, algo, "lcg", 4))
        out.append(case(1920, 1080, 640, 360, 0, algo, "noise", 4))
        out.append(case(4096, 4096, 1024, 1024, 2, algo, "noise", 6))
    errors = [
        dict(name="err_zero_source", sw=0, sh=48, dw=10, dh=10, color_type=3, algorithm=1, gen="bytes", data_len=0, seed=1),
        dict(name="err_zero_destination", sw=10, sh=10, dw=0, dh=48, color_type=3, algorithm=1, gen="bytes", data_len=400, seed=1),
        dict(name="err_zero_source_before_destination", sw=0, sh=48, dw=0, dh=0, color_type=3, algorithm=1, gen="bytes", data_len=0, seed=1),
        dict(name="err_data_length", sw=47, sh=48, dw=10, dh=10, color_type=3, algorithm=2, gen="bytes", data_len=9216, seed=1),
        dict(name="err_too_large", sw=16777217, sh=13, dw=4, dh=4, color_type=2, algorithm=0, gen="bytes", data_len=12, seed=1),
        dict(name="err_too_large_destination", sw=4, sh=4, dw=5, dh=16777217, color_type=2, algorithm=0, gen="bytes", data_len=48, seed=1),
        dict(name="err_too_large_before_data_length", sw=16777217, sh=13, dw=4, dh=4, color_type=2, algorithm=0, gen="bytes", data_len=0, seed=1),
        dict(name="err_zero_before_too_large", sw=16777217, sh=0, dw=4, dh=4, color_type=2, algorithm=0, gen="bytes", data_len=0, seed=1),
        dict(name="err_color_type", sw=4, sh=4, dw=2, dh=2, color_type=9, algorithm=1, gen="bytes", data_len=64, seed=1),
        dict(name="err_algorithm", sw=4, sh=4, dw=2, dh=2, color_type=3, algorithm=7, gen="bytes", data_len=64, seed=1),
        dict(name="err_color_type_before_algorithm", sw=0, sh=0, dw=2, dh=2, color_type=9, algorithm=7, gen="bytes", data_len=0, seed=1),
        dict(name="err_algorithm_before_dimensions", sw=0, sh=0, dw=2, dh=2, color_type=3, algorithm=7, gen="bytes", data_len=0, seed=1),
    ]
    return out, errors


def main():
    good, errors = cases()
    os.makedirs(os.path.join(RC.GOLDEN, "resize"), exist_ok=True)
    rows = []
    for i in range(0, len(good), 8):
        chunk = good[i:i + 8]
        for c, (data, err, _) in zip(chunk, RC.run_wasm(chunk)):
            assert err is None, (c, err)
            assert len(data) == c["dw"] * c["dh"] * RC.BPP[c["color_type"]], c
            row = dict(c, len=len(data), sha256=hashlib.sha256(data).hexdigest(), file=None)
            if len(data) <= STORE_LIMIT:
                row["file"] = "resize/%s.bin" % c["name"]
                with open(os.path.join(RC.GOLDEN, row["file"]), "wb") as f:
                    f.write(data)
            rows.append(row)
            print(c["name"], len(data), file=sys.stderr)
    for c, (data, err, _) in zip(errors, RC.run_wasm(errors)):
        assert data is None, c
        rows.append(dict(c, error=err))
        print(c["name"], err, file=sys.stderr)
    with open(RC.CASES_JSON, "w") as f:
        json.dump(rows, f, indent=0)
        f.write("\n")
    print("%d cases (%d stored in full)" % (len(rows), sum(1 for r in rows if r.get("file"))))


if __name__ == "__main__":
    main()
