"""`pixo::png::encode_images` of include/pixo.hpp, compiled with g++ and linked against the C-ABI library.  Without a GPU:
it compiles, links, and the calls that must throw do (their checks run before a device is touched).  On the GPU: its files
equal those of a loop of `pixo::png::encode` in the same program, and the ones the Python binding makes of the same block."""
import os
import subprocess

import pytest

import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "png_encode_images")


def build():
    lib = os.path.join(ROOT, "pixo_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-o", EXE, os.path.join(ROOT, "tests", "cpp", "png_encode_images.cpp"),
                           "-L" + lib, "-lpixo_hip", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"])


def test_cpp_png_encode_images_compiles_links_and_checks():
    build()
    r = subprocess.run([EXE, "checks"], capture_output=True, text=True)
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_cpp_png_encode_images(tmp_path):
    from pixo_amd import ColorType, png
    build()
    shapes = [(150, 90, 3), (5, 3, 0), (97, 53, 2), (33, 70, 1)]  # (width, height, colour type), at odd places in the block
    records, at = [], 3
    for w, h, ct in shapes:
        records.append((w, h, ct, at))
        at += w * h * (ct + 1) + 5
    block = synth.lcg_bytes(at, 77)
    block.tofile(tmp_path / "block.bin")
    args = [str(v) for r in records for v in r]
    for preset in (0, 1):
        r = subprocess.run([EXE, str(tmp_path / "block.bin"), str(preset), str(tmp_path / "f"), *args], capture_output=True, text=True)
        assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout + r.stderr
        want = png.encode_images(block, [(w, h, ColorType(ct), o) for w, h, ct, o in records], png.PngOptions.builder(0, 0).preset(preset).build())
        assert [(tmp_path / ("fimages%d.png" % i)).read_bytes() for i in range(len(records))] == want
        assert [(tmp_path / ("floop%d.png" % i)).read_bytes() for i in range(len(records))] == want
