#!/usr/bin/env python3
"""Record the expected bytes of tests/resize_reach_cases.py.

Every case runs through the independent numpy model (tests/resize_model.py) and through the kernels' arithmetic compiled for
the host (tests/emu_resize); the two must agree byte for byte, or nothing is written.  tests/golden/resize_reach_cases.json
then holds, per case, `len` and `sha256`, and the bytes themselves as hex where there are at most 64 of them.  This is
recorded MODEL output: the reference's wasm build is not involved here (it is not present where these vectors were made), the
model itself is pinned to that build by the vectors of tests/golden/resize_cases.json.  The case the model needs about half a
minute for is marked "model_checked_by": "maker": the suite holds it to the host arithmetic only.

    python tests/golden/make_golden_resize_reach.py
"""
import hashlib
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import emu_resize_lib as E  # noqa: E402
import resize_cases as RC  # noqa: E402
import resize_model as M  # noqa: E402
import resize_reach_cases as RR  # noqa: E402

HEX_LIMIT = 64


def main():
    rows = []
    for c in RR.CASES:
        px = RC.make_input(c)
        args = (c["sw"], c["sh"], c["dw"], c["dh"], RR.bpp(c), c["algorithm"])
        t0 = time.time()
        want = M.resize(px, *args)
        seconds = time.time() - t0
        host = E.resize(px, *args)
        diff = RC.first_difference(host, want)
        assert diff is None, "%s: host arithmetic against the model: %s" % (c["name"], diff)
        assert len(want) == c["dw"] * c["dh"] * RR.bpp(c), c["name"]
        row = dict(name=c["name"], len=len(want), sha256=hashlib.sha256(want).hexdigest())
        if len(want) <= HEX_LIMIT:
            row["hex"] = want.hex()
        if c["name"] == RR.MAKER_ONLY:
            row["model_checked_by"] = "maker"
        rows.append(row)
        print("%-44s %9d bytes  model %.1f s" % (c["name"], len(want), seconds), file=sys.stderr)
    with open(RR.CASES_JSON, "w") as f:
        json.dump(rows, f, indent=0)
        f.write("\n")
    print("%d cases (%d stored as hex)" % (len(rows), sum(1 for r in rows if "hex" in r)))


if __name__ == "__main__":
    main()
