"""The cases of tests/golden/png_own_bytes.json: the whole output of every zlib, PNG and PNG batch entry point on inputs the
other suites already build, recorded as length and sha256 from one revision's library (tests/golden/
make_golden_png_own_bytes.py) and held against every later one (tests/test_gpu_png_own_bytes.py).  The IDAT bodies are this
library's own DEFLATE, so nothing of the reference is involved: the file pins what the entries return, whatever is behind
them.  CASES is an ordered list of (name, run); building it needs no GPU, `run()` does and returns the bytes to digest (the
files of a batch each behind its length as 8 little-endian bytes).  Test harness only."""
import hashlib
import struct

import numpy as np

import device_pointer_cases as DP
import png_file_cases as PF
import png_quantize_cases as QC
import synth

ZLIB_OUT_OFFSETS = (0, 1, 2, 3)
BPP = {0: 1, 1: 2, 2: 3, 3: 4}


def P():
    from pixo_amd import png
    return png


def cuda(px):
    import torch
    return torch.from_numpy(np.ascontiguousarray(px, dtype=np.uint8).reshape(-1).copy()).cuda()


def digest(data):
    return {"len": len(data), "sha256": hashlib.sha256(data).hexdigest()}


def joined(files):
    return b"".join(struct.pack("<Q", len(f)) + f for f in files)


def opts(w, h, ct, preset=0, flags=0, quantization=None):
    from pixo_amd import ColorType
    o = P().PngOptions.builder(w, h).color_type(ColorType(ct)).preset(preset).flags(flags).build()
    if quantization is not None:
        o.quantization = quantization
    return o


def photo_like(w, h, bpp, seed):
    """(tests/test_gpu_png_batch.py's content: the scene in any colour type, noise where the image is too small for it)"""
    if min(w, h) < 16:
        return synth.lcg_bytes(w * h * bpp, seed)
    rgb = synth.scene(w, h, seed).reshape(h, w, 3)
    if bpp == 3:
        return rgb.reshape(-1)
    if bpp == 1:
        return rgb[:, :, 1].reshape(-1).copy()
    if bpp == 2:
        return np.stack([rgb[:, :, 1], 255 - rgb[:, :, 0] // 2], axis=2).reshape(-1)
    return np.concatenate([rgb, 255 - rgb[:, :, :1] // 3], axis=2).reshape(-1)


def zlib_device(data, level, bpp, row, effort, out_offset):
    """The stream as the device entry leaves it in a caller's buffer that starts out_offset bytes past an aligned address"""
    import torch
    cap = max(P().stored_bound(len(data)), 8)
    d_in = cuda(np.frombuffer(data, np.uint8)) if data else 0
    d_all, d_out = DP.at_offset(cap, out_offset)
    n = P().zlib_compress_device(d_in, len(data), d_out, cap, level, bpp, row, effort)
    torch.cuda.synchronize()
    assert DP.untouched(d_all, out_offset, cap)
    return d_out[:n].cpu().numpy().tobytes()


def with_batch_bytes(limit, run):
    from pixo_amd import _lib
    L = _lib.load()
    L.pixo_hip_debug_configure(("png_batch_bytes=%d" % limit).encode())
    try:
        return run()
    finally:
        L.pixo_hip_debug_configure(None)


def into_pageable_arena(d_all, o, n):
    offsets, lens = P().encode_batch_device_into(None, d_all, o, n)
    arena = np.full(offsets[-1] + lens[-1] + 8, 0xEE, np.uint8)
    assert P().encode_batch_device_into(arena, d_all, o, n) == (offsets, lens)
    return struct.pack("<%dQ" % (2 * n), *(offsets + lens)) + arena.tobytes()


def _cases():
    out = []

    def add(name, run):
        out.append((name, run))

    # ---- zlib: host and device entry --------------------------------------------------------------------------------------
    for name, data, bpp, row, _ in DP.zlib_cases() + [("empty_0", b"", 0, 0, False)]:
        for effort in (0, 1):
            add("zlib_host_%s_e%d" % (name, effort), lambda data=data, bpp=bpp, row=row, effort=effort: P().zlib_compress(data, 6, bpp, row, effort))
            for off in ZLIB_OUT_OFFSETS:
                add("zlib_device_%s_e%d_out%d" % (name, effort, off),
                    lambda data=data, bpp=bpp, row=row, effort=effort, off=off: zlib_device(data, 6, bpp, row, effort, off))
    three = DP.zlib_cases()[1][1]
    for level in (0, 1, 6, 9):  # (the header's FLEVEL only)
        add("zlib_host_level%d" % level, lambda level=level: P().zlib_compress(three, level))
        add("zlib_device_level%d" % level, lambda level=level: zlib_device(three, level, 0, 0, 0, 0))

    # ---- single PNG ---------------------------------------------------------------------------------------------------------
    preset0_groups = {(512, 512, 2, 0), (512, 512, 3, 0)}  # (tests/test_gpu_png_batch.py GROUPS with preset 0)
    for c in PF.CASES:
        add("png_encode_" + c["name"], lambda c=c: P().encode(PF.make_input(c), PF.options(c)))
        if (c["w"], c["h"], c["color_type"], c["preset"]) in preset0_groups:
            def parallel(c=c):
                o = PF.options(c)
                o.flags = 0
                return P().encode(PF.make_input(c), o)
            add("png_encode_flags0_" + c["name"], parallel)
    for ct in (0, 1, 2, 3):
        add("png_device_1x1_c%d" % ct, lambda ct=ct: P().encode_device(cuda(synth.lcg_bytes(BPP[ct], 7 + ct)), opts(1, 1, ct)))
    for w, h in ((254, 257), (255, 256)):  # streams of 65,535 and 65,536 bytes
        add("png_device_gray_%dx%d" % (w, h), lambda w=w, h=h: P().encode_device(cuda(photo_like(w, h, 1, 20)), opts(w, h, 0)))
    add("png_encode_two_idat_300x300", lambda: P().encode(synth.rgba_noise_alpha1(300, 300, 12), P().PngOptions.fast(300, 300)))
    add("png_device_effort_high_200x150", lambda: P().encode_device(cuda(photo_like(200, 150, 3, 31)), opts(200, 150, 2, flags=P().EFFORT_HIGH)))
    pal = next(c for c in PF.CASES if c["gen"] == "pal" and c["preset"] == 1)
    add("png_device_trns_" + pal["name"], lambda: P().encode_device(cuda(PF.make_input(pal)), PF.options(pal)))

    # ---- lossy --------------------------------------------------------------------------------------------------------------
    for tag, c in (("applied", QC.APPLIED[0]), ("declined", QC.DECLINED[0])):
        add("png_lossy_%s_%s" % (tag, c["name"]), lambda c=c: P().encode(QC.make_input(c), QC.options(c)))

    # ---- batch --------------------------------------------------------------------------------------------------------------
    def gray3():
        images = [photo_like(254, 257, 1, 20 + i) for i in range(3)]
        return joined(P().encode_batch_device(cuda(np.concatenate(images)), opts(254, 257, 0), 3))
    add("batch_gray_3x254x257", gray3)

    def tiny(w, h, ct, n):
        images = [photo_like(w, h, ct + 1, 50 + i) for i in range(n)]
        return joined(P().encode_batch_device(cuda(np.concatenate(images)), opts(w, h, ct), n))
    for w, h, ct, n in ((37, 29, 2, 1), (1, 1, 2, 3), (5, 3, 1, 5), (61, 47, 0, 3), (61, 47, 3, 3)):
        add("batch_tiny_%dx%d_c%d_n%d" % (w, h, ct, n), lambda w=w, h=h, ct=ct, n=n: tiny(w, h, ct, n))

    def lossy2():
        q = P().QuantizationOptions(P().QuantizationMode.FORCE, 64, True)
        images = [photo_like(128, 96, 4, 70 + i) for i in range(2)]
        return joined(P().encode_batch_device(cuda(np.concatenate(images)), opts(128, 96, 3, quantization=q), 2))
    add("batch_lossy_2x128x96", lossy2)

    def seven():
        return cuda(np.concatenate([photo_like(128, 96, 3, 80 + i) for i in range(7)]))
    add("batch_sub_batches_7x128x96",
        lambda: with_batch_bytes(96 * (3 * 128 + 1) * 5 // 2, lambda: joined(P().encode_batch_device(seven(), opts(128, 96, 2), 7))))

    def arena():
        images = [photo_like(61, 47, 3, 90 + i) for i in range(3)]
        return into_pageable_arena(cuda(np.concatenate(images)), opts(61, 47, 2), 3)
    add("batch_into_pageable_arena_3x61x47", arena)
    return out


CASES = _cases()
NAMES = [name for name, _ in CASES]
assert len(set(NAMES)) == len(NAMES)
