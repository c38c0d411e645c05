"""The high-effort finder's arithmetic (pixo_amd/csrc/png_deflate_math.h: chain_link, chain_step, kept_length, lazy_defers,
lazy_next) compiled for the host and walked one position after the other (tests/emu_png_deflate_effort/), against the
plain model (tests/deflate_effort_model.py) on the cases of tests/deflate_effort_cases.py.  No GPU."""
import numpy as np
import pytest

import deflate_effort_cases as EC
import deflate_effort_model as M
import deflate_reference as R
import emu_png_deflate_effort_lib as E

GRID = [(64, 4), (64, 8), (256, 4), (256, 8)]  # the set the constants are chosen from


def test_the_rules_one_by_one():
    L = E.lib()
    assert L.emu_chain_link(10, 0) == 0  # no head
    assert L.emu_chain_link(10, 4) == 7  # head: position + 1
    assert L.emu_chain_link(40000, 40000 - 32768 + 1) == 32768 and L.emu_chain_link(40000, 40000 - 32768) == 0
    assert L.emu_chain_step(0, 0) == 0 and L.emu_chain_step(0, 5) == 5 and L.emu_chain_step(5, 7) == 12
    assert L.emu_chain_step(32000, 768) == 32768 and L.emu_chain_step(32000, 769) == 0
    assert [L.emu_kept_length(l, d) for l, d in ((2, 1), (3, 4096), (3, 4097), (4, 32768))] == [0, 3, 0, 4]
    assert L.emu_lazy_next(9, 5, 6) == 10 and L.emu_lazy_next(9, 5, 5) == 14 and L.emu_lazy_next(9, 0, 0) == 10
    assert L.emu_lazy_next(9, 0, 3) == 10


@pytest.mark.parametrize("substep", [64, 256])
@pytest.mark.parametrize("name", ["window_chain", "chain_depth", "tiny_7"])
def test_links_are_the_distances_to_the_heads_the_model_saw(name, substep):
    _, data, _, _, _ = EC.get(name, substep, 8)
    h_all = R.hash4_all(data)
    for chunk, c0 in enumerate(range(0, len(data), R.CHUNK)):
        n = min(R.CHUNK, len(data) - c0)
        seen = M.heads_seen(h_all, len(data), c0, n, substep)
        at = np.arange(len(seen)) + max(c0 - R.WINDOW, 0)
        want = np.where((seen >= 0) & (at - seen <= R.WINDOW), at - seen, 0)
        assert np.array_equal(E.links(data, chunk, substep), want)


@pytest.mark.parametrize("substep,probes", GRID)
@pytest.mark.parametrize("name", EC.NAMES)
def test_tokens_of_the_host_build_are_the_models(name, substep, probes):
    _, data, bpp, row, _ = EC.get(name, substep, probes)
    assert E.tokens(data, bpp, row, substep, probes) == EC.model(name, substep, probes)[0]
