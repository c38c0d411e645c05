"""`pixo::convert::layout_images`, `convert_images`, `convert_images_device`, `convert` and `convert_device` of
include/pixo.hpp, compiled with g++ and linked against the C-ABI library.  Without a GPU: they compile, link, the layout is the
binding's, and a refusal surfaces as the mirror's error with its kind and the library's message (the checks run before a device
is touched).  On the GPU: every image of the block equals the numpy model's conversion of the same pixels."""
import os
import subprocess

import numpy as np
import pytest

import convert_cases as CC
import convert_model as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "test_convert_images")


def build():
    lib = os.path.join(ROOT, "pixo_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-o", EXE, os.path.join(ROOT, "tests", "cpp", "test_convert_images.cpp"),
                           "-L" + lib, "-lpixo_hip", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"])


def test_cpp_convert_images_compiles_links_and_checks():
    build()
    r = subprocess.run([EXE, "checks"], capture_output=True, text=True)
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_cpp_convert_images(tmp_path):
    from pixo_amd import convert
    build()
    shapes = [(37, 23, M.RGBA), (64, 41, M.GRAY_ALPHA), (1, 1, M.GRAY), (129, 7, M.RGB), (5, 300, M.RGBA)]
    records, block = CC.block_of(shapes, 650)
    block.tofile(tmp_path / "px.bin")
    for target in (M.OPAQUE, M.TO_GRAY):
        laid, total = convert.layout_images(records, target)
        r = subprocess.run([EXE, str(tmp_path / "px.bin"), str(target), str(tmp_path / "out.bin")] + [str(v) for s in shapes for v in s],
                           capture_output=True, text=True)
        assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout + r.stderr
        out = np.fromfile(tmp_path / "out.bin", np.uint8)
        assert out.size == total
        for i, (s, d) in enumerate(zip(records, laid)):
            assert np.array_equal(CC.image_bytes(out, d), M.convert(CC.image_bytes(block, s), s[2], int(d[2]))), "target %d, image %d" % (target, i)
