"""`pixo::decode::decode_png_batch(files, one_thread, device_inflate = true)` of include/pixo.hpp, compiled with g++ and linked
against the C-ABI library.  Without a GPU: it compiles, links, and the refusals that touch no device surface as the mirror's
errors.  On the GPU: the images equal what the Python binding makes of the same files, with and without the flag."""
import os
import subprocess

import pytest

import png_decode_cases as PC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "test_png_decode_batch_inflate")


def build():
    lib = os.path.join(ROOT, "pixo_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-o", EXE, os.path.join(ROOT, "tests", "cpp", "test_png_decode_batch_inflate.cpp"),
                           "-L" + lib, "-lpixo_hip", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"])


def test_cpp_png_decode_batch_inflate_compiles_links_and_checks():
    build()
    r = subprocess.run([EXE, "checks"], capture_output=True, text=True)
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("one_thread", (False, True))
def test_cpp_png_decode_batch_inflate(tmp_path, one_thread):
    from pixo_amd import decode
    build()
    files = [PC.make(67, 65, PC.RGB, 8, seed=201), PC.make(33, 70, PC.INDEXED, 4, seed=202, trns=bytes([0, 128])),
             PC.make(1, 1, PC.GRAY, 8, seed=203), PC.make(64, 4, PC.RGBA, 8, seed=204), PC.make(9, 131, PC.GRAY_ALPHA, 16, seed=205),
             PC.make(129, 130, PC.RGB, 8, seed=206, idat_split=500)]
    paths = []
    for i, f in enumerate(files):
        paths.append(str(tmp_path / ("%d.png" % i)))
        open(paths[-1], "wb").write(f)
    r = subprocess.run([EXE, str(tmp_path / "out.bin"), "1" if one_thread else "0"] + paths, capture_output=True, text=True)
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout + r.stderr
    want = decode.decode_png_batch(files, one_thread=one_thread, device_inflate=True)
    assert want == decode.decode_png_batch(files)
    assert r.stdout.splitlines()[:len(files)] == ["%d %d %d %d" % (im.width, im.height, int(im.color_type), len(im.pixels)) for im in want]
    assert (tmp_path / "out.bin").read_bytes() == b"".join(im.pixels for im in want)
