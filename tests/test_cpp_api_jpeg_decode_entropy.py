"""`pixo::decode::decode_jpeg_batch(files, one_thread, device_entropy = true)` of include/pixo.hpp, compiled with g++ and linked
against the C-ABI library.  Without a GPU: it compiles, links, and the refusals that touch no device surface as the mirror's
errors.  On the GPU: one mixed batch, the images equal what the Python binding makes of the same files, with and without the flag."""
import os
import subprocess

import pytest

import jpeg_decode_cases as JC
import jpeg_entropy_cases as EC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "test_jpeg_decode_entropy")


def build():
    lib = os.path.join(ROOT, "pixo_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-o", EXE, os.path.join(ROOT, "tests", "cpp", "test_jpeg_decode_entropy.cpp"),
                           "-L" + lib, "-lpixo_hip", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"])


def test_cpp_jpeg_decode_entropy_compiles_links_and_checks():
    build()
    r = subprocess.run([EXE, "checks"], capture_output=True, text=True)
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("one_thread", (False, True))
def test_cpp_jpeg_decode_batch_entropy(tmp_path, one_thread):
    from pixo_amd import decode
    build()
    files = [JC.data(JC.by_name(n)) for n in ("gray_50x37_q80", "444_50x37_q95", "422_50x37_q80_rst5", "420_50x37_q80", "gray_1x1_q80")]
    files += [EC.borders()["ff00_straddles_a_border"], EC.never_synchronises(EC.geometry()["round_cap"] + 18)]
    paths = []
    for i, f in enumerate(files):
        paths.append(str(tmp_path / ("%d.jpg" % i)))
        open(paths[-1], "wb").write(f)
    r = subprocess.run([EXE, str(tmp_path / "out.bin"), "1" if one_thread else "0"] + paths, capture_output=True, text=True)
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout + r.stderr
    want = decode.decode_jpeg_batch(files, one_thread=one_thread, device_entropy=True)
    assert want == decode.decode_jpeg_batch(files)
    assert r.stdout.splitlines()[:len(files)] == ["%d %d %d %d" % (im.width, im.height, int(im.color_type), len(im.pixels)) for im in want]
    assert (tmp_path / "out.bin").read_bytes() == b"".join(im.pixels for im in want)
