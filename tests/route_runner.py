"""One child of the GPU random slice (tests/test_gpu_random_slice.py): runs cases START .. START + COUNT - 1 of SEED
(tests/random_cases.py) under the debug switches SWITCHES ("-": none) and compares every output with the oracle.

    python tests/route_runner.py SEED START COUNT [SWITCHES|-] [FOCUS|-]

Per case: prints the case's replay line (flushed: a crash leaves it as the last line), clears the route record, makes the
call, compares, keeps the route bits.  Stops at the first mismatch or error (exit 1).  Ends with one line
`RESULT {json}`: the cases run, this child's look-back fallbacks, the route histogram and every case's route bits."""
import json
import os
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))

import numpy as np  # noqa: E402

import oracle_lib as O  # noqa: E402
import random_cases as R  # noqa: E402
from pixo_amd import ColorType, error, jpeg, png  # noqa: E402

_torch = None


def torch():
    global _torch
    if _torch is None:
        import torch as t
        _torch = t
    return _torch


def options(d):
    b = jpeg.JpegOptions.builder(d["w"], d["h"]).color_type(ColorType(d["ct"])).quality(d["q"]) \
        .subsampling(jpeg.Subsampling(d["ss"])).optimize_huffman(d["opt"]).progressive(d["prog"]).trellis_quant(d["trellis"])
    if d["restart"] is not None:
        b = b.restart_interval(d["restart"])
    return b.build()


def on_device(a, offset=0):
    """(keeper tensor, device address) of a copy of numpy array `a` in HBM, `offset` bytes past a 256-byte aligned start."""
    t = torch()
    raw = np.ascontiguousarray(a).view(np.uint8).reshape(-1)
    buf = t.zeros(raw.size + offset + 16, dtype=t.uint8, device="cuda:0")
    buf[offset:offset + raw.size] = t.from_numpy(raw).to("cuda:0")
    t.cuda.synchronize()
    return buf, buf.data_ptr() + offset


def host_storage(n, mem):
    """A uint8 numpy array of n bytes: pinned (a view of a pinned torch tensor) or pageable."""
    n = max(int(n), 1)
    if mem == "pinned":
        keep = torch().empty(n, dtype=torch().uint8).pin_memory()
        return keep, keep.numpy()
    a = np.empty(n, np.uint8)
    return a, a


def _sized(need, dest):
    return {"exact": need, "short": need - 1, "roomy": need + 4096}[dest]


def _into(d, need, call):
    """call(size) writes into storage of `size` bytes and returns (length, array); `short` storage must be refused with the
    size needed, and a retry with that size must succeed (the reserve-and-retry protocol)."""
    size = _sized(need, d["dest"])
    if d["dest"] == "short":
        try:
            call(size)
        except error.BufferTooSmall as e:
            assert e.needed == need, ("needed", e.needed, need)
            size = e.needed
        else:
            raise AssertionError("storage of %d bytes for a %d-byte file was accepted" % (size, need))
    return call(size)


def run_jpeg(d, want):
    """-> list of files (or a coefficient tuple) the library made for case d."""
    e, px = d["entry"], R.pixels(d)
    if e == "encode":
        return [jpeg.encode(px, options(d))]
    if e == "encode_into":
        out = bytearray(b"stale bytes")
        jpeg.encode_into(out, px, options(d))
        return [bytes(out)]
    if e == "encode_jpeg":
        return [jpeg.encode_jpeg(px, d["w"], d["h"], d["ct"], d["q"], d["preset"], d["ss"])]
    if e == "encode_into_buffer":
        def call(size):
            keep, arr = host_storage(size, d["mem"])
            n = jpeg.encode_into_buffer(arr[:size], px, options(d))
            return [bytes(arr[:n])]
        return _into(d, len(want[0]), call)
    if e == "encode_device":
        keep, ptr = on_device(px, d.get("offset", 0))
        return [jpeg.encode_device(ptr, options(d))]
    if e == "encode_device_into":
        keep, ptr = on_device(px, d.get("offset", 0))

        def call(size):
            hold, arr = host_storage(size, d["mem"])
            n = jpeg.encode_device_into(arr[:size], ptr, options(d))
            return [bytes(arr[:n])]
        return _into(d, len(want[0]), call)
    if e in ("batch_device", "batch_device_into", "batch_multi"):
        keep, ptr = on_device(px)
        b = d["batch"]
        if e == "batch_device":
            return jpeg.encode_batch_device(ptr, options(d), b)
        fn = jpeg.encode_batch_device_into if e == "batch_device_into" else \
            (lambda arena, p, o, n: jpeg.encode_batch_multi(arena, keep[:px.size], o, n, [0, 0]))
        offs, lens = fn(None, ptr, options(d), b)  # size query
        need = offs[-1] + lens[-1]

        def call(size):
            hold, arr = host_storage(size, d.get("mem", "pageable"))
            o2, l2 = fn(arr[:size], ptr, options(d), b)
            return [bytes(arr[o:o + n]) for o, n in zip(o2, l2)]
        return _into(d, need, call)
    if e == "encode_multi":
        return [jpeg.encode_multi(px, options(d), [0] * d["k"])]
    if e == "coefficients":
        return jpeg.coefficients(px, options(d))
    if e == "coefficients_device":
        t = torch()
        keep, ptr = on_device(px, d.get("offset", 0))
        yb, cbn = jpeg.coefficient_geometry(d["w"], d["h"], d["ct"], d["ss"])
        y = t.full((yb, 64), 0x5A5A, dtype=t.int16, device="cuda:0")
        cb = t.full((max(cbn, 1), 64), 0x5A5A, dtype=t.int16, device="cuda:0")
        cr = t.full((max(cbn, 1), 64), 0x5A5A, dtype=t.int16, device="cuda:0")
        jpeg.coefficients_device(ptr, d["w"], d["h"], d["ct"], d["ss"], d["q"], y, cb, cr)
        t.cuda.synchronize()
        return y.cpu().numpy(), cb.cpu().numpy()[:cbn], cr.cpu().numpy()[:cbn]
    y, cb, cr = O.coeffs(R.image(d), d["w"], d["h"], d["ct"], d["ss"], d["q"])
    if e == "entropy_encode":
        return [jpeg.entropy_encode(y, cb, cr, options(d))]
    if e == "entropy_encode_device":
        keep = [on_device(a)[0] for a in (y, cb if cb.size else np.zeros(64, np.int16), cr if cr.size else np.zeros(64, np.int16))]
        return [jpeg.entropy_encode_device(*[k.data_ptr() for k in keep], options(d))]
    raise ValueError("unknown entry %r" % e)


def run_png(d):
    t_px = R.pixels(d)
    w, h, bpp, st = d["w"], d["h"], d["bpp"], d["strategy"]
    if d["entry"] == "png":
        return png.apply_filters(t_px, w, h, bpp, st)
    t = torch()
    keep, ptr = on_device(t_px, d["offset"])
    out = t.zeros(png.filtered_size(w, h, bpp), dtype=t.uint8, device="cuda:0")
    if d["entry"] == "png_device":
        ad = png.apply_filters_device(ptr, w, h, bpp, out, st)
        return out.cpu().numpy(), ad
    sums = t.zeros(2 * h, dtype=t.int64, device="cuda:0")
    scratch = t.zeros(4, dtype=t.int32, device="cuda:0")
    png.apply_filters_async(ptr, w, h, bpp, out, sums, scratch, st, 0, t.cuda.current_stream().cuda_stream)
    t.cuda.synchronize()
    return out.cpu().numpy(), png.adler32_from_row_sums(sums.cpu().numpy().view(np.uint64), w, h, bpp)


def check(d, got, want):
    if d["kind"] == "png" or d["entry"].startswith("coefficients"):
        for i, (g, w) in enumerate(zip(got, want)):
            if isinstance(w, np.ndarray):
                assert np.array_equal(np.asarray(g).reshape(w.shape), w), "output %d differs from the oracle's" % i
            else:
                assert g == w, ("adler32", g, w)
        return
    assert len(got) == len(want), ("files", len(got), len(want))
    for i, (g, w) in enumerate(zip(got, want)):
        if g != w:
            k = next((j for j in range(min(len(g), len(w))) if g[j] != w[j]), min(len(g), len(w)))
            raise AssertionError("file %d differs from the oracle's: %d vs %d bytes, first difference at byte %d" % (i, len(g), len(w), k))


def main(argv):
    seed, start, count = int(argv[0]), int(argv[1]), int(argv[2])
    switches = argv[3] if len(argv) > 3 and argv[3] != "-" else ""
    focus = argv[4] if len(argv) > 4 and argv[4] != "-" else None
    jpeg.debug_configure(switches)
    fb0 = jpeg.lookback_fallbacks()
    hist, per_case, n, t0 = {}, [], 0, time.time()
    try:
        for d in R.cases(seed, count, start, focus):
            print(R.replay_line(d, switches), flush=True)
            want = R.expected(d, O)
            if d.get("trim"):
                jpeg.trim()
            jpeg.debug_routes(clear=True)
            got = run_png(d) if d["kind"] == "png" else run_jpeg(d, want)
            bits = jpeg.debug_routes(clear=True)
            check(d, got, want)
            per_case.append([d["i"], d["entry"], bits])
            for name in jpeg.route_names(bits):
                hist[name] = hist.get(name, 0) + 1
            n += 1
    except Exception as e:  # the replay line above names the case
        print("FAIL %s: %s" % (type(e).__name__, e), flush=True)
        return 1
    finally:
        jpeg.debug_configure("")
    print("RESULT " + json.dumps({"cases": n, "seconds": round(time.time() - t0, 2), "fallbacks": jpeg.lookback_fallbacks() - fb0,
                                  "routes": hist, "per_case": per_case}), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
