#!/usr/bin/env python3
"""Record what this library's own zlib, PNG and PNG batch entries return: length and sha256 of the whole output of every case
of tests/png_own_bytes_cases.py, into tests/golden/png_own_bytes.json.  Needs the GPU.  Run it on the revision whose bytes
are to be kept, BEFORE a change that must not move them, and select that revision's library with PIXO_HIP_LIB (built by
`AB_REV=<revision> tools/ab_build.sh parent`); the header names both.

    PIXO_HIP_LIB=tools/ab/ab_parent.so python tests/golden/make_golden_png_own_bytes.py <revision>
"""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    import png_own_bytes_cases as OB
    from pixo_amd import _lib
    revision = sys.argv[1]
    cases = []
    for name, run in OB.CASES:
        cases.append(dict(name=name, **OB.digest(run())))
        print(name, cases[-1]["len"], cases[-1]["sha256"][:16])
    json.dump({"revision": revision, "library": os.path.relpath(_lib.LIB_PATH, ROOT), "cases": cases},
              open(os.path.join(HERE, "png_own_bytes.json"), "w"), indent=0)


if __name__ == "__main__":
    main()
