"""Per-call wall time of the whole-file entry points (the host layer between the C ABI and the routes), one JSON line.
For A/B runs of two builds of the same C ABI: run once per build with PIXO_HIP_LIB=<library>, alternating, in one session
on one card; the spread of the same build against itself is the margin.
    python tools/entry_legs_timing.py [label]"""
import json, os, sys, time
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "tests"))
import numpy as np, torch
import synth
from pixo_amd import jpeg


def median_us(fn, warm, reps):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter(); fn(); ts.append(time.perf_counter() - t0)
    ts.sort()
    return round(ts[len(ts) // 2] * 1e6, 1)


def main():
    label = sys.argv[1] if len(sys.argv) > 1 else "build"
    dev = torch.device("cuda:0")
    S420 = jpeg.Subsampling(1)
    out = {"label": label, "lib": os.environ.get("PIXO_HIP_LIB", "in-tree")}
    # whole-file 4096x4096: device pixels into pinned and pageable storage, host pixels into a block
    w = h = 4096
    px = synth.noise(w, h, 7)
    o = jpeg.JpegOptions.builder(w, h).quality(80).subsampling(S420).build()
    d = torch.from_numpy(px).to(dev); torch.cuda.synchronize()
    pinned = torch.empty(w * h * 2, dtype=torch.uint8).pin_memory()
    pageable = np.empty(w * h * 2, dtype=np.uint8); pageable[:] = 0
    out["4096_device_into_pinned"] = median_us(lambda: jpeg.encode_device_into(pinned, d, o), 10, 100)
    out["4096_device_into_pageable"] = median_us(lambda: jpeg.encode_device_into(pageable, d, o), 10, 60)
    out["4096_encode_host"] = median_us(lambda: jpeg.encode(px, o), 5, 40)
    del d, pinned, pageable
    # 1080p preset 2 (trellis + progressive + optimised tables)
    w, h = 1920, 1080
    px = synth.noise(w, h, 11)
    o2 = jpeg.JpegOptions.max(w, h, 80)
    d = torch.from_numpy(px).to(dev); torch.cuda.synchronize()
    pinned = torch.empty(w * h * 2, dtype=torch.uint8).pin_memory()
    out["1080p_preset2_encode_host"] = median_us(lambda: jpeg.encode(px, o2), 10, 100)
    out["1080p_preset2_device_into_pinned"] = median_us(lambda: jpeg.encode_device_into(pinned, d, o2), 10, 100)
    # 64 x 1080p: blocks of the library's, and a pinned arena
    batch = 64
    o = jpeg.JpegOptions.builder(w, h).quality(80).subsampling(S420).build()
    one = torch.from_numpy(px).to(dev)
    db = one.reshape(1, -1).repeat(batch, 1).contiguous(); torch.cuda.synchronize()
    arena = torch.empty(batch * w * h * 2, dtype=torch.uint8).pin_memory()

    def blocks():
        files, lens = jpeg.encode_batch_device_raw(db, o, batch)
        jpeg.free_files(files, batch)
    out["64x1080p_batch_device"] = median_us(blocks, 5, 40)
    out["64x1080p_batch_device_into_pinned"] = median_us(lambda: jpeg.encode_batch_device_into(arena, db, o, batch), 5, 40)
    del db, arena
    # a small file: the fixed cost per call
    w, h = 200, 150
    px = synth.noise(w, h, 3)
    o = jpeg.JpegOptions.builder(w, h).quality(80).subsampling(S420).build()
    out["200x150_encode_host"] = median_us(lambda: jpeg.encode(px, o), 50, 1000)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
