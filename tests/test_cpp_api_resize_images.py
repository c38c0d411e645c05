"""`pixo::resize::fit_images`, `resize_images` and `resize_images_device` of include/pixo.hpp, compiled with g++ and linked
against the C-ABI library.  Without a GPU: they compile, link, the fitted sizes are the binding's, and a refusal surfaces as
the mirror's error with its kind and the library's message (the checks run before a device is touched).  On the GPU: every
image of the block equals what the Python binding makes of the same pixels."""
import os
import subprocess

import numpy as np
import pytest

import resize_cases as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "test_resize_images")


def build():
    lib = os.path.join(ROOT, "pixo_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-o", EXE, os.path.join(ROOT, "tests", "cpp", "test_resize_images.cpp"),
                           "-L" + lib, "-lpixo_hip", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"])


def test_cpp_resize_images_compiles_links_and_checks():
    build()
    r = subprocess.run([EXE, "checks"], capture_output=True, text=True)
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_cpp_resize_images(tmp_path):
    from pixo_amd import resize
    build()
    shapes = [(37, 23, 2), (64, 41, 3), (1, 1, 0), (129, 7, 1), (5, 300, 2)]
    pixels = [RC.make_input(dict(sw=w, sh=h, color_type=ct, gen="lcg", seed=650 + i)) for i, (w, h, ct) in enumerate(shapes)]
    records, at = [], 0
    for px, (w, h, ct) in zip(pixels, shapes):
        records.append((w, h, ct, at))
        at = (at + px.size + 15) // 16 * 16
    block = np.zeros(at, np.uint8)
    for px, (_, _, _, o) in zip(pixels, records):
        block[o:o + px.size] = px
    block.tofile(tmp_path / "px.bin")
    fitted, total = resize.fit_images(records, 20, 16)
    for algo in (0, 1, 2):
        r = subprocess.run([EXE, str(tmp_path / "px.bin"), "20", "16", str(algo), str(tmp_path / "out.bin")] + [str(v) for s in shapes for v in s],
                           capture_output=True, text=True)
        assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout + r.stderr
        out = (tmp_path / "out.bin").read_bytes()
        assert len(out) == total
        want = resize.resize_images(block, records, fitted, algo)
        for i, (w, h, ct, o) in enumerate(fitted):
            assert out[o:o + w * h * (int(ct) + 1)] == want[i], "algorithm %d, image %d" % (algo, i)
