"""The pieces of the PNG tail that need no device (pixo_amd/csrc/png_encode_api.cpp: the segment table's layout, the Adler-32
joined from the chunks' sums, the file head, the IDAT frames with their joined CRC-32 and IEND) in a stand-alone program
built with AddressSanitizer and UndefinedBehaviorSanitizer on the host side and linked against the library for everything
else (tests/cpp/test_png_tail_host.cpp).  Every buffer there is an exact heap block, so a byte too far is reported."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_png_tail_host_pieces_under_sanitizers(tmp_path):
    exe, obj, lib = str(tmp_path / "test_png_tail_host"), str(tmp_path / "test_png_tail_host.o"), os.path.join(ROOT, "pixo_amd")
    san = ["-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=undefined"]  # (host side only, compile and link)
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950", "-std=c++17", "-O1", "-g", "-fPIC"] + san +
                          ["-c", os.path.join(ROOT, "tests", "cpp", "test_png_tail_host.cpp"), "-o", obj])
    subprocess.check_call(["/opt/rocm/bin/hipcc", "--offload-arch=gfx950"] + san + [obj, "-o", exe,
                           "-L" + lib, "-lpixo_hip", "-Wl,-rpath," + lib, "-Wl,-rpath,/opt/rocm/lib"])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and "all checks passed" in r.stdout, r.stdout + r.stderr
