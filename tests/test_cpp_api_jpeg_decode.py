"""`pixo::decode::decode_jpeg`, `decode_jpeg_batch` and `decode_jpeg_batch_device` of include/pixo.hpp, compiled with g++ and
linked against the C-ABI library.  Without a GPU: it compiles, links, and a refusal surfaces as the mirror's error with its
kind and the library's message (the walk runs before a device is touched).  On the GPU: three cases come back as the
committed libjpeg-turbo pixels."""
import os
import subprocess

import pytest

import jpeg_decode_cases as JC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "test_jpeg_decode")


def build():
    lib = os.path.join(ROOT, "pixo_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-o", EXE, os.path.join(ROOT, "tests", "cpp", "test_jpeg_decode.cpp"),
                           "-L" + lib, "-lpixo_hip", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"])


def test_cpp_jpeg_decode_compiles_links_and_checks():
    build()
    r = subprocess.run([EXE, "checks"], capture_output=True, text=True)
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_cpp_jpeg_decode(tmp_path):
    build()
    cases = [JC.by_name(n) for n in ("420_50x37_q80_rst5", "gray_17x17_q80", "422_33x17_q80_opt")]
    r = subprocess.run([EXE, str(tmp_path / "out.bin")] + [JC.path(c) for c in cases], capture_output=True, text=True)
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout + r.stderr
    assert r.stdout.splitlines()[:len(cases)] == ["%d %d %d %d" % (c["w"], c["h"], c["color_type"], len(JC.expected(c))) for c in cases]
    assert (tmp_path / "out.bin").read_bytes() == b"".join(JC.expected(c) for c in cases)
