"""`pixo::png::encode` of include/pixo.hpp with quantisation, compiled with g++ against the C-ABI library and called on the
GPU: through `PngOptions::quantization` and through the explicit overload the file equals the Python binding's lossy file, and
with the mode Off the lossless one."""
import os
import subprocess

import pytest

import png_quantize_cases as QC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "test_png_quantize")


@pytest.mark.gpu
def test_cpp_png_encode_routes_on_quantization(tmp_path):
    from pixo_amd import png
    lib = os.path.join(ROOT, "pixo_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-o", EXE, os.path.join(ROOT, "tests", "cpp", "test_png_quantize.cpp"),
                           "-L" + lib, "-lpixo_hip", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"])
    c = next(c for c in QC.CASES if c["name"] == "pal_n1000_130x65_c2_p2")
    c = dict(c, preset=1)
    px = QC.make_input(c)
    px.tofile(tmp_path / "px.bin")
    outs = [tmp_path / n for n in ("member.png", "overload.png", "off.png")]
    r = subprocess.run([EXE, str(tmp_path / "px.bin"), str(c["w"]), str(c["h"])] + [str(o) for o in outs], capture_output=True, text=True)
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout + r.stderr
    lossy = png.encode(px, QC.options(c))
    plain = QC.options(c)
    plain.quantization = png.QuantizationOptions()
    assert outs[0].read_bytes() == lossy and outs[1].read_bytes() == lossy
    assert outs[2].read_bytes() == png.encode(px, plain) != lossy
    assert lossy[25] == 3  # IHDR colour type: the indexed file
