"""The JPEG decode kernel's own code (pixo_amd/csrc/jpeg_decode_math.h) and the host decoder (jpeg_decode_host.cpp) compiled
for the host (tests/emu_jpeg_decode): tile by tile with the halo and the edge replication against the committed libjpeg
pixels and the sequential model — the files Pillow wrote and the ones no encoder writes (JC.SYNTH) —; the arithmetic cases of
tests/jpeg_decode_arith.py (the IDCT at the edge of its region, scaled tables, strips of the colour images, upsampler stripes);
the 32-bit bound; and the stand-alone program that runs the marker walk, the entropy decoder and the kernel's code over every
case and a few thousand seeded mutations with the host sanitizers.  No GPU.  Nothing sanitised is loaded into python: the
program is a child process with its own main."""
import glob
import os
import subprocess

import numpy as np
import pytest

import emu_jpeg_decode_lib as E
import jpeg_decode_arith as AR
import jpeg_decode_cases as JC
import jpeg_decode_model as M


@pytest.mark.parametrize("c", JC.CASES + JC.SYNTH, ids=JC.IDS + JC.SYNTH_IDS)
def test_tiles_with_halo_give_libjpeg_pixels_at_every_alignment(c):
    """Every tile of the image through phase A and phase B, lane by lane; the image at a 16-byte boundary (whole dwordx4
    stores) and 1 and 3 bytes behind one (byte stores)."""
    n = len(JC.expected(c))
    for misalign in (0, 1, 3):
        rc, msg, w, h, ct, px = E.decode(JC.data(c), n, misalign)
        assert (rc, msg) == (0, "") and (w, h, ct) == (c["w"], c["h"], c["color_type"])
        assert JC.mismatch(px, c) == "", misalign


def test_structs_and_lds_budget():
    L = E.lib()
    assert L.emu_jd_record_bytes() == 448
    sizes = [L.emu_jd_lds_bytes(k) for k in range(4)]
    assert sizes == [64 * 64, 3 * 64 * 64, 16 * 2 * 4 * 64 + 2 * 18 * 4 * 64, 16 * 2 * 4 * 2 * 64 + 2 * 18 * 6 * 64]
    assert max(sizes) * 2 <= 160 * 1024  # at least two workgroups to a CU


def test_every_case_lies_inside_the_32_bit_bound():
    """jpeg_decode_math.h's sufficient bound on the dequantised blocks, inside which 32-bit arithmetic is libjpeg's: the
    comparisons above are made inside it."""
    for c in JC.CASES + JC.SYNTH:
        assert E.within_bound(JC.data(c)) == 1, c["name"]


def emulated(data, want, misalign=0):
    """'' when the kernel's code gives `want` (a uint8 array) from the file"""
    rc, msg, w, h, ct, px = E.decode(data, want.size, misalign)
    if (rc, msg) != (0, "") or (h, w) != want.shape[:2]:
        return "status %d %r, %d x %d" % (rc, msg, w, h)
    bad = np.flatnonzero(np.frombuffer(px, np.uint8) != want.reshape(-1))
    return "%d bytes differ, first at byte %d" % (bad.size, bad[0]) if bad.size else ""


@pytest.mark.parametrize("q", [1, 4])
def test_idct_basis_sweep_and_dense_blocks_at_the_edge_of_the_region(q):
    """Every basis function alone at the largest amplitude that keeps the samples in -512..511 (and half of it, and on DC +-1016)
    and 200 dense blocks at 0.6 .. 0.9 of the 32-bit bound: the kernel's 32-bit code is the model's (and Pillow's: the CPU tests)"""
    data, want, _ = AR.idct_sweep(q)
    assert emulated(data, want) == "" and emulated(data, want, 3) == ""
    # the dense blocks lie inside the header's sufficient bound (a) by its own evaluation; most lone amplitudes lie beyond it
    # ((3, 3) at 2127 weighs 163,000) and still no intermediate leaves 32 bits, which the comparison above shows
    dense = np.array(AR.dense_blocks(200, AR.DENSE_SEED, q)).reshape(8, 25, 64)
    assert E.within_bound(AR.W.write(200, 64, AR.W.gray(), {0: AR.ONES * q}, [dense], q16=(0,))) == 1
    assert E.within_bound(data) == 0


@pytest.mark.parametrize("name", AR.SCALED)
def test_scaled_tables(name):
    """Tables times 2 and 4: libjpeg's pixels (the CPU tests).  Times 16 the blocks leave -512..511, where libjpeg's masked table
    wraps: ours are the CLAMPED samples, the model's, as jpeg_decode_math.h documents"""
    for factor in (2, 4, 16):
        data, want = AR.scaled(name, factor)
        assert E.within_bound(data) == (1 if factor == 2 else 0)  # (a) is sufficient, not necessary: times 4 is still libjpeg's
        assert emulated(data, want) == "", factor


@pytest.mark.parametrize("name", AR.COLOUR_IMAGES)
def test_colour_conversion_over_strips_of_the_input_space(name):
    """One tile row (four block rows) of the 2048 x 2048 image at each end and in the middle of its first variable, all 256 values
    of the second; the whole images run on the device"""
    for rows in (range(0, 4), range(126, 130), range(252, 256)):
        data, blocks = AR.colour_image(name, rows)
        want = np.broadcast_to(blocks[:, None, :, None, :], (4, 8, 256, 8, 3)).reshape(32, 2048, 3)
        assert emulated(data, want) == "", rows


@pytest.mark.parametrize("mode,trim", [("422", 1), ("422", 2), ("420", 1), ("420", 2)])
def test_upsamplers_over_stripes_of_neighbour_values(mode, trim):
    """Every 13th pair of the lattice and the four extra pairs; the whole lattice runs on the device"""
    data, want = AR.upsampler_image(mode, trim, AR.LATTICE[::13] + AR.LATTICE[-4:])
    assert emulated(data, want) == "" and emulated(data, want, 1) == ""


def test_emulation_refuses_as_the_model_does():
    d = JC.data(JC.by_name("420_50x37_q80"))
    for bad in (d[:-60], d[:300], b"\x00" + d):
        rc, msg, *_ = E.decode(bad, 1 << 16)
        with pytest.raises(M.Refused) as e:
            M.decode(bad)
        assert rc == 1 and msg == e.value.msg


def test_stand_alone_program_over_cases_and_mutations():
    """Every case and 60 seeded mutations of each (about 8,000 runs): each must end with pixels or a refusal — with the host
    sanitizers built in where their runtime is installed, a crash, an out-of-bounds access or undefined behaviour ends the
    program with a report and a non-zero status."""
    E.lib()
    files = sorted(glob.glob(os.path.join(JC.DIR, "*.jpg"))) + sorted(glob.glob(os.path.join(JC.SYNTH_DIR, "*.jpg")))
    assert len(files) == len(JC.CASES) + len(JC.SYNTH)
    r = subprocess.run([E.MAIN, "60"] + files, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    out = r.stdout.decode()
    assert r.returncode == 0, out + r.stderr.decode()[-4000:]
    how, runs, decoded, refused = out.split()
    assert how in ("sanitized", "plain") and runs == "runs=%d" % (61 * len(files))
    assert int(decoded.split("=")[1]) >= len(files) and int(refused.split("=")[1]) > 1000
