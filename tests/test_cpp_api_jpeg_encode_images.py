"""`pixo::jpeg::encode_images` and `encode_images_device` of include/pixo.hpp, compiled with g++ and linked against the C-ABI
library.  Without a GPU: they compile, link, and the calls that must throw do, with the mirror's error kind and the library's
message (their checks run before a device is touched).  On the GPU: the host form's and the device form's files of three
images equal those of a loop of `pixo::jpeg::encode` in the same program, and the ones the Python binding's single entry makes."""
import os
import subprocess

import pytest

import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "test_jpeg_encode_images")


def build():
    lib = os.path.join(ROOT, "pixo_amd")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-o", EXE, os.path.join(ROOT, "tests", "cpp", "test_jpeg_encode_images.cpp"),
                           "-L" + lib, "-lpixo_hip", "-ldl", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"])


def test_cpp_jpeg_encode_images_compiles_links_and_checks():
    build()
    r = subprocess.run([EXE, "checks"], capture_output=True, text=True)
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout + r.stderr


@pytest.mark.gpu
def test_cpp_jpeg_encode_images(tmp_path):
    import torch
    from pixo_amd import ColorType, jpeg
    build()
    shapes = [(150, 90, 2), (5, 3, 0), (97, 53, 2)]  # (width, height, colour type), at odd places in the block
    records, at = [], 3
    for w, h, ct in shapes:
        records.append((w, h, ct, at))
        at += w * h * (ct + 1) + 5
    block = synth.lcg_bytes(at, 78)
    block.tofile(tmp_path / "block.bin")
    args = [str(v) for r in records for v in r]
    for preset, ss in ((0, 1), (0, 0), (1, 1)):
        r = subprocess.run([EXE, str(tmp_path / "block.bin"), str(preset), str(ss), str(tmp_path / "f"), *args], capture_output=True, text=True)
        assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout + r.stderr
        o = jpeg.JpegOptions.builder(0, 0).quality(80).preset(preset).subsampling(jpeg.Subsampling(ss)).build()
        for i, (w, h, ct, off) in enumerate(records):
            one = jpeg.JpegOptions(**{**o.__dict__, "width": w, "height": h, "color_type": ColorType(ct)})
            want = jpeg.encode_device(torch.from_numpy(block[off:off + w * h * (ct + 1)].copy()).cuda(), one)
            for form in ("host", "device", "loop"):
                assert (tmp_path / ("f%s%d.jpg" % (form, i))).read_bytes() == want, (preset, ss, form, i)
