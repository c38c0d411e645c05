"""`pixo::png::encode_batch` of include/pixo.hpp, compiled with g++ and linked against the C-ABI library.  Without a GPU:
it compiles, links, and the calls that must throw do (their checks run before a device is touched).  On the GPU: its files
equal the ones the Python binding makes of the same pixels."""
import os
import subprocess

import numpy as np
import pytest

import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "test_png_encode_batch")


def build():
    lib = os.path.join(ROOT, "pixo_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-o", EXE, os.path.join(ROOT, "tests", "cpp", "test_png_encode_batch.cpp"),
                           "-L" + lib, "-lpixo_hip", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"])


def test_cpp_png_encode_batch_compiles_links_and_checks():
    build()
    r = subprocess.run([EXE, "checks"], capture_output=True, text=True)
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_cpp_png_encode_batch(tmp_path):
    from pixo_amd import png
    build()
    w, h, batch = 150, 90, 3
    px = np.concatenate([synth.rgba_noise_alpha1(w, h, 21 + i) for i in range(batch)])
    px.tofile(tmp_path / "px.bin")
    for preset in (0, 1):
        r = subprocess.run([EXE, str(tmp_path / "px.bin"), str(w), str(h), str(preset), str(batch), str(tmp_path / "f")], capture_output=True, text=True)
        assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout + r.stderr
        want = png.encode_batch(px, png.PngOptions.builder(w, h).preset(preset).build(), batch)
        assert [(tmp_path / ("f%d.png" % i)).read_bytes() for i in range(batch)] == want
