#!/usr/bin/env python3
"""The JPEG decode batch with the Huffman decode on the device (PIXO_DECODE_DEVICE_ENTROPY, jpeg_entropy_dec.hip) against the
same entry without the flag, on the same build in the same run, the two alternating.  The three workloads of
tools/jpeg_decode_batch_timing.py.  Wall time of pixo_hip_jpeg_decode_batch_device up to the synchronisation of its stream,
median and minimum of ROUNDS rounds after WARMUP warm-up rounds; the legs from pixo_hip_debug_jpeg_decode_batch_timed (under
the flag [0] is the host's share: records and scans laid out, the files decoded again) and the device leg of the entropy passes
from pixo_hip_debug_jpeg_entropy_last (HIP events from the scans' upload to the DC launch, the host waits for the round
counters included); rounds used and files decoded again per workload.  Before timing, the images with the flag are compared
with the images without.

    python tools/jpeg_entropy_timing.py [--out profiles/jpeg_entropy_timing.txt]
"""
import argparse
import os
import socket
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import torch  # noqa: E402

from jpeg_decode_batch_timing import workloads  # noqa: E402
from pixo_amd import _lib, decode  # noqa: E402

WARMUP, ROUNDS = 2, 5


def med(v):
    return "%9.2f (%8.2f)" % (statistics.median(v), min(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    L = _lib.load()
    g = decode.decode_jpeg_entropy_geometry()
    lines = ["JPEG decode batch, Huffman decode on the device against on the host (8 threads), %s on %s (%s)" % (
        L.pixo_hip_version().decode(), torch.cuda.get_device_name(0), socket.gethostname()),
        "subsequence %d bytes, %d a workgroup, round cap %d; ms, median (min) of %d rounds after %d warm-up rounds, the forms alternating" % (
            g["sub_bytes"], g["group_subs"], g["round_cap"], ROUNDS, WARMUP),
        "call = wall time up to the synchronisation of the stream", ""]
    print("\n".join(lines), flush=True)
    for name, files in workloads().items():
        _, total = decode.decode_jpeg_batch_info(files)
        out = torch.empty(total, dtype=torch.uint8, device="cuda")
        other = torch.empty(total, dtype=torch.uint8, device="cuda")
        decode.decode_jpeg_batch_device(files, out=out)
        decode.decode_jpeg_batch_device(files, out=other, device_entropy=True)
        torch.cuda.synchronize()
        assert torch.equal(out, other), name
        t = {"host": [], "device": []}
        legs = {"host": [], "device": []}
        last = []
        for r in range(WARMUP + ROUNDS):
            for form in t:
                t0 = time.perf_counter()
                decode.decode_jpeg_batch_device(files, out=out, device_entropy=form == "device")
                torch.cuda.synchronize()
                if r >= WARMUP:
                    t[form].append((time.perf_counter() - t0) * 1e3)
            for form in t:
                ms = decode.decode_jpeg_batch_timed(files, device_entropy=form == "device")
                if r >= WARMUP:
                    legs[form].append(ms)
                    if form == "device":
                        last.append(decode.decode_jpeg_entropy_last())
        plan = decode.decode_jpeg_batch_plan(files, device_entropy=True)
        lines.append("%s: %.1f MiB of files, %.1f MiB of pixels, %d of %d files on the device, %d sub-batch(es)" % (
            name, sum(len(f) for f in files) / 2**20, total / 2**20, sum(plan["on_device"]), len(files), len(plan["sub_first"]) - 1))
        lines.append("  entropy decode on the      call ms")
        for form in t:
            lines.append("  %-22s %s" % (form, med(t[form])))
        for form in t:
            leg = [statistics.median(x[i] for x in legs[form]) for i in range(5)]
            lines.append("  legs, %-6s (timed entry, host block): host's share %.2f, coefficient uploads %.2f, decode kernels %.2f, copy down %.2f, whole call %.2f" % (
                (form,) + tuple(leg)))
        lines.append("  device leg of the entropy passes %.2f ms; rounds used %d; files decoded again by the host %d" % (
            statistics.median(x["device_ms"] for x in last), max(x["rounds"] for x in last), max(x["files_redone"] for x in last)))
        lines.append("  host / device: %.2f" % (statistics.median(t["host"]) / statistics.median(t["device"])))
        lines.append("")
        print("\n".join(lines[-8:]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
