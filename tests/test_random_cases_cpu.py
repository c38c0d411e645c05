"""The seeded case generator (tests/random_cases.py) on the CPU: committed seeds give committed digests of their first
descriptors, so a change of the generator — which silently changes what the GPU random slice tests — has to be deliberate;
every descriptor is plain JSON, replayable by seed and index alone, and the oracle accepts every one of them."""
import json

import pytest

import oracle_lib as O
import random_cases as R

DIGESTS = {  # sha-256 of the first 200 descriptors, one JSON line each (random_cases.digest)
    932: "bb23810222da712edee2fdec392f351f7bb265d241f7376ae631e505430d712f",
    955: "44cca539dde275df1af38a231686ba0c6c8ed6e9ec3c2ff7690fc40d4e1d38f9",
    20261016: "ea3b0db023905d3ed71631b91274bda4b068d57a7dfd63445f3cbe394b165360",
}


@pytest.mark.parametrize("seed", sorted(DIGESTS))
def test_committed_seeds_give_committed_descriptors(seed):
    assert R.digest(seed, 200) == DIGESTS[seed]


def test_case_i_depends_on_seed_and_index_alone():
    every = list(R.cases(955, 50))
    assert [list(R.cases(955, 1, i))[0] for i in (0, 17, 49)] == [every[0], every[17], every[49]]
    for d in every:
        assert json.loads(json.dumps(d)) == d
        assert R.replay_line(d).startswith("REPLAY python tests/route_runner.py 955 %d 1 " % d["i"])


@pytest.mark.parametrize("focus", [None] + sorted(R.FOCUS))
def test_every_descriptor_is_accepted_by_the_oracle(focus):
    n = 0
    for d in R.cases(4242, 40, focus=focus):
        if d["kind"] == "jpeg" and d["w"] * d["h"] > 1 << 21:
            continue  # (the few large cases: the GPU slice runs them)
        want = R.expected(d, O)
        assert want is not None and len(want) > 0, R.replay_line(d)
        if d["kind"] == "jpeg" and not d["entry"].startswith("coefficients"):
            assert len(want) == (d.get("batch") or 1)
            assert all(f[:2] == b"\xff\xd8" and f[-2:] == b"\xff\xd9" for f in want)
        n += 1
    assert n >= 30


def test_the_generator_reaches_every_entry_content_and_edge():
    ds = [d for s in DIGESTS for d in R.cases(s, 400)]
    jp = [d for d in ds if d["kind"] == "jpeg"]
    assert {d["entry"] for d in ds} == {e for e, _ in R.JPEG_ENTRIES + R.PNG_ENTRIES}
    assert {d["content"] for d in jp} == set(R.CONTENTS)
    assert {d["strategy"] for d in ds if d["kind"] == "png"} == set(range(9))
    assert {d["bpp"] for d in ds if d["kind"] == "png"} == {1, 2, 3, 4, 6, 8}
    assert any(d["w"] < 4 for d in jp) and any(d["w"] >= 65534 for d in jp) and any(d["w"] * d["h"] > 1 << 24 for d in jp)
    assert any(d["w"] % 512 in (1, 511) for d in jp)
    assert {d.get("offset") for d in jp} >= {0, 1, 2, 3}
    assert {d.get("dest") for d in jp} >= {"exact", "short", "roomy"} and {d.get("mem") for d in jp} >= {"pinned", "pageable"}
    assert {1, 100} <= {d["q"] for d in jp}
    assert any(d["trim"] for d in ds)
    assert any(d["restart"] is not None and d["restart"] * (1 if d["ct"] == 0 else 3) < 96 for d in jp)
    assert any(d["opt"] for d in jp) and any(d["prog"] for d in jp) and any(d["trellis"] for d in jp)
