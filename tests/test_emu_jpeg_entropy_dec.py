"""The device Huffman decode's own code (pixo_amd/csrc/jpeg_entropy_dec_math.h) compiled for the host and run pass by pass
(tests/emu_jpeg_entropy_dec): cold decode, hand-over rounds workgroup by workgroup and launch by launch, verify, write, DC —
against the host's decoder over every committed decode case, the border files of tests/jpeg_entropy_cases.py, a scan that never
synchronises, malformed scans; and the stand-alone program that runs the same over every case and a few thousand seeded
mutations of their scans with the host sanitizers.  No GPU.  Nothing sanitised is loaded into python: the program is a child
process with its own main."""
import glob
import os
import subprocess

import numpy as np
import pytest

import jpeg_decode_cases as JC
import jpeg_entropy_cases as EC


def test_geometry_and_record():
    g = EC.geometry()
    assert g["sub_bytes"] % 16 == 0 and g["group_subs"] == 256 and g["record_bytes"] % 16 == 0
    # twice the largest count of profiles/jpeg_entropy_rounds.txt
    with open(os.path.join(os.path.dirname(JC.HERE), "profiles", "jpeg_entropy_rounds.txt")) as f:
        last = f.read().strip().splitlines()[-1]
    assert last.endswith("the cap is twice that: %d" % g["round_cap"]), last


@pytest.mark.parametrize("c", JC.CASES + JC.SYNTH, ids=JC.IDS + JC.SYNTH_IDS)
def test_committed_cases_give_the_hosts_coefficients(c):
    """Every case the host accepts and the device takes: vouched, and every coefficient of every component the host's"""
    e = EC.emulate(JC.data(c))
    assert e["host_ok"]
    if e["status"] == 3:
        return  # a restart interval, no MCUs or a scan of a few bytes: the host's from the start
    assert e["status"] == 0 and e["vouched"] and e["rounds"] < EC.geometry()["round_cap"]
    assert np.array_equal(e["coef"], e["host_coef"])


@pytest.mark.parametrize("name", sorted(EC.borders()))
def test_border_files(name):
    e = EC.emulate(EC.borders()[name])
    assert e["status"] == 0 and e["host_ok"] and e["vouched"], e
    assert np.array_equal(e["coef"], e["host_coef"])


def test_border_files_have_their_properties():
    g, b = EC.geometry(), EC.borders()
    S, G = g["sub_bytes"], g["group_subs"]
    s = EC.scan_of(b["ff00_straddles_a_border"])
    assert any(s[k - 1:k + 1] == b"\xff\x00" for k in range(S, len(s) - 4, S))
    s = EC.scan_of(b["ff00_ends_at_a_border"])
    assert any(s[k - 2:k] == b"\xff\x00" for k in range(S, len(s) - 4, S))
    for n in (S - 1, S, S + 1, G * S - 1, G * S, G * S + 1):
        assert len(EC.scan_of(b["scan_of_%d_bytes" % n])) == n
    assert EC.emulate(b["scan_of_%d_bytes" % (G * S)])["launches"] == 1 and EC.emulate(b["scan_of_%d_bytes" % (G * S + 1)])["launches"] == 2
    assert EC.emulate(b["three_workgroups"])["subs"] > 2 * G
    assert EC.scan_of(b["stuffed_ff_is_the_last_scan_byte"])[-4:] == b"\xff\x00\xff\xd9"
    assert EC.scan_of(b["fill_bytes_in_front_of_eoi"])[-7:] == b"\xff" * 6 + b"\xd9"
    assert not EC.scan_of(b["no_eoi"]).endswith(b"\xff\xd9")


def test_a_scan_that_never_synchronises_needs_a_round_per_subsequence():
    """Round k repairs exactly subsequence k: below the cap vouched with subs - 1 rounds, above it not vouched at the cap"""
    cap = EC.geometry()["round_cap"]
    e = EC.emulate(EC.never_synchronises(cap - 32))
    assert e["vouched"] and e["rounds"] == e["subs"] - 1 < cap and np.array_equal(e["coef"], e["host_coef"])
    e = EC.emulate(EC.never_synchronises(cap + 18))
    assert e["subs"] > cap + 1 and not e["vouched"] and e["why"] == EC.NOT_SETTLED and e["rounds"] == cap and e["host_ok"]
    # and under a smaller cap the first is not vouched either
    e = EC.emulate(EC.never_synchronises(cap - 32), cap=10)
    assert not e["vouched"] and e["why"] == EC.NOT_SETTLED and e["rounds"] == 10


@pytest.mark.parametrize("name", sorted(EC.malformed()))
def test_what_the_host_refuses_is_not_vouched_for(name):
    e = EC.emulate(EC.malformed()[name][0])
    assert e["status"] == 0 and not e["host_ok"] and not e["vouched"]


def test_refused_cases_and_cut_files_are_not_vouched_for():
    """Every committed case cut inside its scan at a few places: the host refuses, the emulated device does not vouch"""
    for c in (JC.CASES + JC.SYNTH)[::5]:
        d = JC.data(c)
        head = len(d) - len(EC.scan_of(d))
        for cut in (head + (len(d) - head) // 3, len(d) - 12):
            e = EC.emulate(d[:cut])
            if e["status"] == 0 and not e["host_ok"]:
                assert not e["vouched"], (c["name"], cut)
            elif e["status"] == 0 and e["vouched"]:
                assert np.array_equal(e["coef"], e["host_coef"]), (c["name"], cut)


def test_stand_alone_program_over_cases_and_mutations():
    """Every case and 40 seeded mutations of each one's scan (about 5,500 runs, each at the round cap and at a cap of 2):
    "vouched" implies the host's coefficients; a lane that asks for a byte outside what its workgroup stages aborts the program,
    and with the host sanitizers built in where their runtime is installed, so does any out-of-bounds access."""
    EC.lib()
    files = sorted(glob.glob(os.path.join(JC.DIR, "*.jpg"))) + sorted(glob.glob(os.path.join(JC.SYNTH_DIR, "*.jpg")))
    assert len(files) == len(JC.CASES) + len(JC.SYNTH)
    r = subprocess.run([EC.MAIN, "40"] + files, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    out = r.stdout.decode()
    assert r.returncode == 0, out + r.stderr.decode()[-4000:]
    f = dict(x.split("=") for x in out.split()[1:])
    # (the program says which build it is; the Makefile leaves the sanitizers out only where their runtime does not link, and
    # then this test still checks "vouched implies the host's coefficients" and the staged ranges — DESIGN.md §4.6g says which
    # build the recorded runs used)
    print("stand-alone program: " + out.split()[0])
    assert out.split()[0] in ("sanitized", "plain") and int(f["runs"]) == 41 * len(files)
    assert int(f["vouched"]) > 1000 and int(f["redone"]) > 1000 and int(f["host_refused"]) > 1000
