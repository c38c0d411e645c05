"""pixo_amd/csrc/baseline_plan.hpp — the route of a whole baseline file — compiled with g++ alone (no HIP, no library) and
table-tested: large / medium / small scans, the bytes-per-block rules, host bands, direct stores, caller storage, batches and
the debug switches that bear on them (tests/cpp/test_baseline_plan.cpp)."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_baseline_plan_table(tmp_path):
    exe = str(tmp_path / "test_baseline_plan")
    src = os.path.join(ROOT, "tests", "cpp", "test_baseline_plan.cpp")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", "-o", exe, src])
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "all checks passed" in r.stdout
