"""`pixo::resize::resize_batch` and `resize_batch_device` of include/pixo.hpp, compiled with g++ and linked against the C-ABI
library.  Without a GPU: they compile, link, and a refusal surfaces as the mirror's error with its kind and the library's
message (the checks run before a device is touched).  On the GPU: the block equals what the Python binding makes of the same
pixels."""
import os
import subprocess

import numpy as np
import pytest

import resize_cases as RC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "test_resize_batch")


def build():
    lib = os.path.join(ROOT, "pixo_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-o", EXE, os.path.join(ROOT, "tests", "cpp", "test_resize_batch.cpp"),
                           "-L" + lib, "-lpixo_hip", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"])


def test_cpp_resize_batch_compiles_links_and_checks():
    build()
    r = subprocess.run([EXE, "checks"], capture_output=True, text=True)
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_cpp_resize_batch(tmp_path):
    from pixo_amd import resize
    build()
    sizes = [(37, 23), (64, 41), (1, 1), (129, 7)]
    srcs = [(RC.make_input(dict(sw=w, sh=h, color_type=2, gen="lcg", seed=600 + i)), w, h) for i, (w, h) in enumerate(sizes)]
    np.concatenate([px for px, _, _ in srcs]).tofile(tmp_path / "px.bin")
    for algo in (0, 1, 2):
        r = subprocess.run([EXE, str(tmp_path / "px.bin"), "17", "13", str(algo), str(tmp_path / "out.bin")] + [str(v) for wh in sizes for v in wh],
                           capture_output=True, text=True)
        assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout + r.stderr
        assert (tmp_path / "out.bin").read_bytes() == b"".join(resize.resize_batch(srcs, 17, 13, 2, algo))
