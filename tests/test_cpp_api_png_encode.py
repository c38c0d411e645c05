"""`pixo::png::encode` of include/pixo.hpp, compiled with g++ against the C-ABI library and called once on the GPU: the file
equals the one the Python binding makes of the same pixels."""
import os
import subprocess

import pytest

import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "test_png_encode")


@pytest.mark.gpu
def test_cpp_png_encode(tmp_path):
    from pixo_amd import png
    lib = os.path.join(ROOT, "pixo_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-o", EXE, os.path.join(ROOT, "tests", "cpp", "test_png_encode.cpp"),
                           "-L" + lib, "-lpixo_hip", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"])
    w, h = 150, 90
    px = synth.rgba_noise_alpha1(w, h, 21)
    px.tofile(tmp_path / "px.bin")
    out = tmp_path / "cpp.png"
    r = subprocess.run([EXE, str(tmp_path / "px.bin"), str(w), str(h), "1", str(out)], capture_output=True, text=True)
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout + r.stderr
    o = png.PngOptions.builder(w, h).preset(1).flags(png.NO_RAYON).build()
    assert out.read_bytes() == png.encode(px, o)
