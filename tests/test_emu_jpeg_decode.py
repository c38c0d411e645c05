"""The JPEG decode kernel's own code (pixo_amd/csrc/jpeg_decode_math.h) and the host decoder (jpeg_decode_host.cpp) compiled
for the host (tests/emu_jpeg_decode): tile by tile with the halo and the edge replication against the committed libjpeg
pixels and the sequential model; the 32-bit bound; and the stand-alone program that runs the marker walk, the entropy decoder
and the kernel's code over every case and a few thousand seeded mutations with the host sanitizers.  No GPU.  Nothing
sanitised is loaded into python: the program is a child process with its own main."""
import glob
import os
import subprocess

import pytest

import emu_jpeg_decode_lib as E
import jpeg_decode_cases as JC
import jpeg_decode_model as M


@pytest.mark.parametrize("c", JC.CASES, ids=JC.IDS)
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
    for c in JC.CASES:
        assert E.within_bound(JC.data(c)) == 1, c["name"]


def test_emulation_refuses_as_the_model_does():
    d = JC.data(JC.by_name("420_50x37_q80"))
    for bad in (d[:-60], d[:300], b"\x00" + d):
        rc, msg, *_ = E.decode(bad, 1 << 16)
        with pytest.raises(M.Refused) as e:
            M.decode(bad)
        assert rc == 1 and msg == e.value.msg


def test_stand_alone_program_over_cases_and_mutations():
    """Every case and 60 seeded mutations of each (about 4,000 runs): each must end with pixels or a refusal — with the host
    sanitizers built in where their runtime is installed, a crash, an out-of-bounds access or undefined behaviour ends the
    program with a report and a non-zero status."""
    E.lib()
    files = sorted(glob.glob(os.path.join(JC.DIR, "*.jpg")))
    assert len(files) == len(JC.CASES)
    r = subprocess.run([E.MAIN, "60"] + files, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=300)
    out = r.stdout.decode()
    assert r.returncode == 0, out + r.stderr.decode()[-4000:]
    how, runs, decoded, refused = out.split()
    assert how in ("sanitized", "plain") and runs == "runs=%d" % (61 * len(files))
    assert int(decoded.split("=")[1]) >= len(files) and int(refused.split("=")[1]) > 1000
