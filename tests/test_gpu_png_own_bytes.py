"""Every zlib, PNG and PNG batch entry returns the bytes it returned at the revision tests/golden/png_own_bytes.json was
recorded from (its header names it): each case of tests/png_own_bytes_cases.py is encoded again and its whole output held
against the recorded length and sha256.  The single entries and the batch entries share one DEFLATE tail, so a batch that
equals its single files (tests/test_gpu_png_batch.py) no longer shows that either is right; this file and the reference's
fixtures do."""
import json
import os

import pytest

import png_own_bytes_cases as OB

GOLDEN = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "png_own_bytes.json")))
WANT = {c["name"]: c for c in GOLDEN["cases"]}


def test_the_golden_holds_exactly_the_tables_names():
    assert [c["name"] for c in GOLDEN["cases"]] == OB.NAMES
    assert GOLDEN["revision"] and GOLDEN["library"]
    assert all(len(c["sha256"]) == 64 and c["len"] > 0 for c in GOLDEN["cases"])


@pytest.mark.gpu
@pytest.mark.parametrize("name,run", OB.CASES, ids=OB.NAMES)
def test_own_bytes(name, run):
    got = OB.digest(run())
    assert (got["len"], got["sha256"]) == (WANT[name]["len"], WANT[name]["sha256"]), name
