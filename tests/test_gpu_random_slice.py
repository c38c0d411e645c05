"""A seeded random slice of every encoder route, on the GPU, checked against the oracle (tests/random_cases.py draws the cases,
tests/route_runner.py runs them in a fresh child process per block, one child at a time).

Blocks: the default switches over three committed seeds (random call histories: nothing is trimmed between cases unless a
case says so), and one block per debug switch of include/pixo_hip.h.  Asserted: every file / tuple / PNG stream equals the
oracle's; the look-back fallback happened under spin_budget=0 and nowhere else; the default blocks together reached every
route that needs no switch; every forced block shows its route and never the route the switch turns off."""
import json
import os
import subprocess
import sys

import pytest

from pixo_amd import jpeg

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
RUNNER = os.path.join(HERE, "route_runner.py")

DEFAULT_SEEDS = (932, 955, 20261016)
DEFAULT_CASES = 360

# switches, focus, cases, routes that must show up, routes that must never show up
FORCED = [
    ("two_kernel_scan", None, 100, {"TWO_KERNEL"}, {"FUSED", "FUSED_SEGMENTED", "FUSED_DIRECT", "BATCH_FUSED"}),
    ("fused_batch", "batch", 80, {"BATCH_FUSED"}, {"DENSE_STREAM_RULE"}),
    ("multipass_entropy", None, 100, {"MULTI_PASS", "PROG_MULTI_PASS"},
     {"SINGLE_PASS_TUPLE", "FUSED", "FUSED_SEGMENTED", "PROG_SINGLE_PASS", "SEGMENTED_TUPLE"}),
    ("host_entropy", None, 100, {"HOST_ENTROPY"}, set()),
    ("one_piece", "big", 30, set(), {"PIECES"}),
    ("piece_groups=1", "big", 50, {"PIECES"}, set()),
    ("piece_medium=2,piece_schedule=1:2:5", "big", 30, set(), set()),
    ("direct_stores", "big", 50, {"DIRECT_STORES"}, set()),
    ("no_direct_small", None, 100, set(), {"FUSED_DIRECT", "DIRECT_STORES", "PROG_DIRECT_SMALL"}),
    ("no_side_stats", "side", 80, set(), {"SIDE_STATS"}),
    ("coef_form=scalar", None, 100, {"COEF_SCALAR"}, {"COEF_PACKED"}),
    ("coef_form=packed", None, 100, {"COEF_PACKED"}, {"COEF_SCALAR"}),
    ("trellis_form=lane", "trellis", 80, {"TRELLIS_LANE"}, {"TRELLIS_GROUP"}),
    ("trellis_form=group", "trellis", 80, {"TRELLIS_GROUP"}, {"TRELLIS_LANE"}),
    ("batch_parts=3", "batch", 80, {"SUB_BATCHES"}, set()),
    ("bands_upload_min_mb=1,bands_upload_mb=1", "host1mb", 60, {"HOST_BANDS", "PIECES", "PIECES_REDO"}, set()),
    ("plain_host", None, 100, set(), set()),
    ("spin_budget=0", "restart", 100, {"FALLBACK"}, set()),
]

# Routes the default switches must reach over the default blocks.
DEFAULT_ROUTES = {
    "FUSED", "FUSED_SEGMENTED", "FUSED_DIRECT", "TWO_KERNEL", "DENSE_STREAM_RULE", "SINGLE_PASS_TUPLE", "MULTI_PASS",
    "RESTUFF_GROW", "CALLER_RETRY", "DIRECT_STORES", "COEF_SCALAR", "LOAD_ALIGNED", "LOAD_FUNNEL", "LOAD_BYTES",
    "PROG_SINGLE_PASS", "PROG_DIRECT_SMALL", "SIDE_STATS", "TRELLIS_GROUP", "BATCH_FUSED", "BATCH_TWO_KERNEL",
    "BANDS_MULTI", "PNG_REGS", "PNG_GENERAL", "PNG_BIGRAMS_REGS", "SEGMENTED_TUPLE",
}
# What only a switch reaches (HOST_ENTROPY, FALLBACK, PROG_MULTI_PASS), or what the default thresholds keep for sizes beyond
# this slice: HOST_BANDS (96 MiB of host pixels), SUB_BATCHES (64 MiB batches), PIECES (large scans into malloc'd or roomy storage).
SWITCH_ONLY = {"HOST_ENTROPY", "FALLBACK", "PROG_MULTI_PASS", "HOST_BANDS", "SUB_BATCHES", "PIECES", "PIECES_REDO"}
# Routes of large launches that the default blocks reach only by chance: the packed DCT / quantiser forms (more than 2048
# workgroups) and the one-lane trellis search (more than 32768 blocks) are forced by their blocks below; the general bigram
# form of the PNG kernel (rows too long for registers) and its 512-thread register form (rows of 16-32 KiB) are not required of it.
LARGE_ONLY = {"COEF_PACKED", "TRELLIS_LANE", "PNG_BIGRAMS", "PNG_REGS512"}


def test_route_lists_name_every_route_bit():
    assert DEFAULT_ROUTES | SWITCH_ONLY | LARGE_ONLY == set(jpeg.ROUTES)
    assert not DEFAULT_ROUTES & SWITCH_ONLY and not DEFAULT_ROUTES & LARGE_ONLY


ABNORMAL = (124, 134, 137, 139)  # time limit, abort, kill, segmentation fault (and any negative status: a signal)


def _stop_everything(why):
    """A child ended abnormally (a crash, a signal, a time limit): it may have left the GPU faulted or hung, so no further
    child is started, in this test or any other, and the whole run ends here with the child's last lines."""
    pytest.exit("GPU random slice stopped: " + why, returncode=3)


def _child(seed, start, count, switches="-", focus=None, timeout=240):
    """One child, waited for.  A mismatch or error (exit 1) fails this test with the child's last lines (its replay line);
    an abnormal end stops the run (_stop_everything)."""
    cmd = [sys.executable, RUNNER, str(seed), str(start), str(count), switches or "-", focus or "-"]
    try:
        p = subprocess.run(cmd, capture_output=True, text=True, timeout=timeout)
    except subprocess.TimeoutExpired as e:
        tail = (e.stdout or b"")
        tail = tail.decode(errors="replace") if isinstance(tail, bytes) else tail
        _stop_everything("child timed out after %d s (%s):\n%s" % (timeout, " ".join(cmd[1:]), "\n".join(tail.splitlines()[-3:])))
    lines = p.stdout.splitlines()
    if p.returncode < 0 or p.returncode in ABNORMAL:
        _stop_everything("child exit %d (%s):\n%s\n%s" % (p.returncode, " ".join(cmd[1:]), "\n".join(lines[-3:]), p.stderr[-2000:]))
    if p.returncode != 0:
        pytest.fail("child exit %d (%s):\n%s\n%s" % (p.returncode, " ".join(cmd[1:]), "\n".join(lines[-3:]), p.stderr[-2000:]))
    res = [l for l in lines if l.startswith("RESULT ")]
    assert res, "child printed no RESULT line:\n" + "\n".join(lines[-3:])
    return json.loads(res[-1][len("RESULT "):])


def _bits(names):
    return sum(1 << jpeg.ROUTES[n] for n in names)


def test_default_switches_random_histories_reach_every_route():
    total, hist, failures = 0, {}, []
    for seed in DEFAULT_SEEDS:
        r = _child(seed, 0, DEFAULT_CASES)
        assert r["cases"] == DEFAULT_CASES
        assert r["fallbacks"] == 0, "seed %d: %d look-back fallbacks under the default switches" % (seed, r["fallbacks"])
        total += r["cases"]
        for k, v in r["routes"].items():
            hist[k] = hist.get(k, 0) + v
    print("default blocks: %d cases, route histogram %s" % (total, json.dumps(dict(sorted(hist.items())))))
    missing = sorted(DEFAULT_ROUTES - set(hist))
    assert not missing, "routes the default blocks never reached: %s (histogram %s)" % (missing, hist)
    leaked = sorted(set(hist) & (SWITCH_ONLY - {"PIECES", "PIECES_REDO"}))
    assert not leaked, "switch-only routes under the default switches: %s" % leaked


@pytest.mark.parametrize("switches,focus,count,must,never", FORCED, ids=[f[0] for f in FORCED])
def test_forced_switch_block(switches, focus, count, must, never):
    seed = 7000 + [f[0] for f in FORCED].index(switches)
    r = _child(seed, 0, count, switches, focus)
    assert r["cases"] == count
    if switches == "spin_budget=0":
        assert r["fallbacks"] > 0, "spin_budget=0 forced no fallback"
    else:
        assert r["fallbacks"] == 0, "%d look-back fallbacks under %s" % (r["fallbacks"], switches)
    seen = set(r["routes"])
    assert must <= seen, "%s: routes %s never served a case (histogram %s)" % (switches, sorted(must - seen), r["routes"])
    bad = [(i, e, jpeg.route_names(b & _bits(never))) for i, e, b in r["per_case"] if b & _bits(never)]
    assert not bad, "%s: the switch did not force its route on cases %s" % (switches, bad[:5])
