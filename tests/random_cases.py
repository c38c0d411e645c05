"""Seeded random cases for the route tests: `cases(seed, n)` yields plain JSON-able descriptors drawn from the seed alone
(never from a clock or a budget), so case i of seed S is always the same call.  `replay_line(d)` is the one line a failing
case prints; `pixels(d)` makes its input.

Every dimension is weighted towards where kernels break: 1-9 and 15-17 pixel edges, widths at the coefficient kernel's tile
boundaries (multiples of 512 / 1536 pixels +- 1), rare strips up to 65535 pixels, restart intervals on both sides of the
single-pass coders' 96-block segment limit, whole MCU rows and longer than the image, q = 1 / 100 and 90..100, 0xFF-heavy
content, every entry point with exact / short / roomy / pinned / pageable storage, device pointers at odd offsets.

Run as `python tests/random_cases.py SEED START COUNT` to print the descriptors of a slice (CPU only)."""
import hashlib
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import synth  # noqa: E402

GRAY, RGB = 0, 2

# entry points and their weights (the first list: pixels in; the tuple entries need no trellis)
JPEG_ENTRIES = [
    ("encode", 22), ("encode_into", 4), ("encode_into_buffer", 10), ("encode_jpeg", 6),
    ("encode_device", 14), ("encode_device_into", 12), ("batch_device", 5), ("batch_device_into", 4),
    ("batch_multi", 2), ("encode_multi", 3), ("coefficients", 6), ("coefficients_device", 5),
    ("entropy_encode", 4), ("entropy_encode_device", 4),
]
PNG_ENTRIES = [("png", 6), ("png_device", 3), ("png_async", 2)]
CONTENTS = ["noise", "ramp", "flat", "specks", "binary", "scene", "photo", "extremes", "noise_q100"]
TUPLE_ENTRIES = ("coefficients", "coefficients_device", "entropy_encode", "entropy_encode_device")
BATCH_ENTRIES = ("batch_device", "batch_device_into", "batch_multi")


def _pick(rng, items):
    names = [n for n, _ in items]
    w = np.array([x for _, x in items], np.float64)
    return names[int(rng.choice(len(names), p=w / w.sum()))]


def _size(rng, entry):
    r = rng.rand()
    if r < 0.22:
        return int(rng.randint(1, 10)), int(rng.randint(1, 10))
    if r < 0.34:
        return int(rng.randint(15, 18)), int(rng.randint(15, 18))
    if r < 0.50:  # tile boundaries of the coefficient / fused kernels: 512 pixels (RGB), 1536 (gray), +-1
        base = int(rng.choice([512, 1024, 1536, 2048, 3072]))
        return max(1, base + int(rng.randint(-1, 2))), int(rng.randint(1, 40))
    if r < 0.53 and entry not in BATCH_ENTRIES:  # strips: one pixel or a few rows, up to the format's 65535
        w = int(rng.choice([65535, 65534, 40001, 17000]))
        return w, int(rng.randint(1, 3))
    if r < 0.533 and entry not in BATCH_ENTRIES:  # large: more than 2048 workgroups (the packed DCT / quantiser forms)
        return 4100, int(rng.choice([4100, 4200]))
    if r < 0.70:
        return int(rng.randint(20, 700)), int(rng.randint(20, 500))
    return int(rng.randint(1, 300)), int(rng.randint(1, 200))


def _restart(rng, w, h, ct, ss):
    unit = 16 if (ct == RGB and ss) else 8
    per_mcu = 1 if ct == GRAY else (6 if ss else 3)
    units = ((w + unit - 1) // unit) * ((h + unit - 1) // unit)
    row = (w + unit - 1) // unit
    r = rng.rand()
    if r < 0.55:
        return None
    if r < 0.67:  # segments below the single-pass coders' 96 blocks: the multi-pass kernels
        return int(rng.randint(1, max(2, 96 // per_mcu)))
    if r < 0.79:  # 96 blocks or more
        return int(min(65535, rng.randint((96 + per_mcu - 1) // per_mcu, 96 // per_mcu + 400)))
    if r < 0.92 and row <= 65535:  # whole MCU rows: segments of the fused kernel
        k = int(rng.randint(1, 4))
        return int(min(65535, k * row)) or 1
    return int(min(65535, units + int(rng.randint(0, 50))))  # longer than the image: no markers at all


def _jpeg_case(rng):
    entry = _pick(rng, JPEG_ENTRIES)
    d = {"kind": "jpeg", "entry": entry}
    w, h = _size(rng, entry)
    ct = GRAY if rng.rand() < 0.3 else RGB
    ss = int(rng.rand() < 0.6)
    r = rng.rand()
    q = 100 if r < 0.12 else (1 if r < 0.17 else (int(rng.randint(90, 101)) if r < 0.5 else int(rng.randint(1, 101))))
    content = CONTENTS[int(rng.randint(0, len(CONTENTS)))]
    if content == "noise_q100":
        q = 100
    if ct == GRAY and content in ("scene", "photo"):
        content = "noise"
    opt = bool(rng.rand() < 0.3)
    prog = bool(rng.rand() < 0.2)
    trellis = bool(rng.rand() < 0.2)
    if w * h > 4 << 20:  # keep the oracle's share of a large case small: baseline, standard tables
        opt = prog = trellis = False
        content = "noise" if content in ("scene", "photo") else content
    if trellis and w * h > 1 << 20:
        trellis = False
    restart = _restart(rng, w, h, ct, ss)
    d.update(w=w, h=h, ct=ct, ss=ss, q=q, content=content, cseed=int(rng.randint(1, 1 << 30)),
             opt=opt, prog=prog, trellis=trellis, restart=restart)
    if entry in TUPLE_ENTRIES:
        d["trellis"] = False
        if entry.startswith("coefficients"):
            d.update(opt=False, prog=False, restart=None)
    if entry == "encode_jpeg":  # the flat export: preset 0 / 1 / 2 decides the flags, no restart interval
        d.update(preset=int(rng.randint(0, 3)), restart=None, opt=False, prog=False, trellis=False)
    if entry in BATCH_ENTRIES:
        d["batch"] = int(rng.choice([2, 3, 5, 8]))
        if w * h * d["batch"] > 3 << 20:
            d["w"], d["h"] = int(rng.randint(16, 700)), int(rng.randint(8, 300))
    if entry == "encode_multi":
        d["k"] = int(rng.choice([1, 2, 3]))
    if entry in ("encode_into_buffer", "encode_device_into", "batch_device_into", "batch_multi"):
        d["dest"] = ["exact", "short", "roomy"][int(rng.randint(0, 3))]
    if entry in ("encode_device_into", "encode_into_buffer", "batch_device_into"):
        d["mem"] = "pinned" if rng.rand() < 0.6 else "pageable"
    if entry in ("encode_device", "encode_device_into", "coefficients_device"):
        d["offset"] = int(rng.choice([0, 0, 1, 2, 3]))
    d["trim"] = bool(rng.rand() < 0.03)
    return d


def _png_case(rng):
    entry = _pick(rng, PNG_ENTRIES)
    bpp = int(rng.choice([1, 2, 3, 4, 6, 8]))
    r = rng.rand()
    if r < 0.2:
        w, h = int(rng.randint(1, 10)), int(rng.randint(1, 10))
    elif r < 0.35:
        w, h = int(rng.randint(2000, 6000)), int(rng.randint(1, 40))
    else:
        w, h = int(rng.randint(1, 700)), int(rng.randint(1, 120))
    return {"kind": "png", "entry": entry, "w": w, "h": h, "bpp": bpp, "strategy": int(rng.randint(0, 9)),
            "content": ["noise", "ramp", "flat", "binary"][int(rng.randint(0, 4))], "cseed": int(rng.randint(1, 1 << 30)),
            "offset": int(rng.choice([0, 0, 1, 3])) if entry != "png" else 0, "trim": bool(rng.rand() < 0.03)}


# A block of forced switches draws its cases with a FOCUS: after the ordinary draw, one field is redrawn so that the forced
# route can apply to most cases (a trellis block needs trellis files, a batch block batches, ...).
FOCUS = {
    "trellis": "trellis on every JPEG case that takes pixels",
    "side": "preset 2 (optimised tables + trellis) on small images",
    "prog": "progressive files",
    "batch": "batch entry points",
    "batch1": "batch entry points of one device",
    "host1mb": "host pixels of 1-3 MB through encode / encode_into_buffer",
    "big": "scans of several thousand blocks through every entry",
    "restart": "restart intervals",
}


def _apply_focus(d, focus, rng):
    if d["kind"] != "jpeg" or not focus:
        return d
    pixel_entry = d["entry"] not in TUPLE_ENTRIES and d["entry"] != "encode_jpeg"
    if focus == "trellis" and pixel_entry:
        d["trellis"] = True
        if d["w"] * d["h"] > 1 << 20:
            d["w"], d["h"] = int(rng.randint(8, 700)), int(rng.randint(8, 500))
    elif focus == "side" and pixel_entry:
        d.update(trellis=True, opt=True, prog=False, w=int(rng.randint(8, 600)), h=int(rng.randint(8, 400)))
    elif focus == "prog" and d["entry"] not in ("coefficients", "coefficients_device", "encode_jpeg"):
        d["prog"] = True
        if d["w"] * d["h"] > 4 << 20:
            d["w"], d["h"] = int(rng.randint(8, 1500)), int(rng.randint(8, 900))
    elif focus in ("batch", "batch1"):
        d["entry"] = ["batch_device", "batch_device_into", "batch_multi"][int(rng.randint(0, 3 if focus == "batch" else 2))]
        d.update(batch=int(rng.choice([3, 5, 8])), w=int(rng.randint(16, 900)), h=int(rng.randint(8, 400)),
                 dest=d.get("dest") or "roomy", mem=d.get("mem") or "pinned", trellis=False)
        d.pop("offset", None)
        d.pop("k", None)
    elif focus == "host1mb":
        d["entry"] = "encode" if rng.rand() < 0.6 else "encode_into_buffer"
        d.update(w=int(rng.randint(600, 1100)), h=int(rng.randint(600, 900)), trellis=False, prog=False)
        if d["entry"] == "encode_into_buffer":
            d.setdefault("dest", "roomy")
            d.setdefault("mem", "pageable")
        d.pop("offset", None)
        d.pop("k", None)
        d.pop("batch", None)
    elif focus == "big" and d["entry"] not in BATCH_ENTRIES:
        d.update(w=int(rng.randint(1200, 2100)), h=int(rng.randint(900, 1300)), trellis=False)
    elif focus == "restart" and d["entry"] not in ("coefficients", "coefficients_device", "encode_jpeg"):
        while d["restart"] is None:
            d["restart"] = _restart(rng, d["w"], d["h"], d["ct"], d["ss"])
    return d


def cases(seed, n, start=0, focus=None):
    """Descriptors start .. start + n - 1 of `seed` (case i depends on seed, i and focus alone)."""
    assert focus is None or focus in FOCUS, focus
    for i in range(start, start + n):
        rng = np.random.RandomState((int(seed) * 1000003 + i) & 0xFFFFFFFF)
        d = _png_case(rng) if rng.rand() < 0.15 else _jpeg_case(rng)
        d = _apply_focus(d, focus, rng)
        d["seed"], d["i"] = int(seed), int(i)
        if focus:
            d["focus"] = focus
        yield d


def replay_line(d, switches=""):
    """The line that replays case d alone: python tests/route_runner.py SEED START 1 SWITCHES FOCUS."""
    return "REPLAY python tests/route_runner.py %d %d 1 %s %s  %s" % (d["seed"], d["i"], switches or "-", d.get("focus") or "-",
                                                                       json.dumps(d, sort_keys=True))


def digest(seed, n):
    """SHA-256 of the first n descriptors of `seed`, one JSON line each (tests/test_random_cases_cpu.py pins these)."""
    hsh = hashlib.sha256()
    for d in cases(seed, n):
        hsh.update((json.dumps(d, sort_keys=True) + "\n").encode())
    return hsh.hexdigest()


def _content(kind, n, seed):
    if kind in ("noise", "noise_q100"):
        return synth.lcg_bytes(n, seed)
    if kind == "ramp":
        return ((np.arange(n, dtype=np.int64) // 3 // ((seed % 97) + 8)) % 256).astype(np.uint8)
    if kind == "flat":
        return np.full(n, seed % 256, np.uint8)
    if kind == "specks":
        b = np.full(n, seed % 256, np.uint8)
        b[synth.lcg_bytes(n, seed) < 2] = 255 - (seed % 256)
        return b
    if kind == "extremes":
        return np.array([0, 1, 254, 255], np.uint8)[synth.lcg_bytes(n, seed) >> 6]
    b = synth.lcg_bytes(n, seed)  # binary
    return np.where(b < 128, 0, 255).astype(np.uint8)


def image(d, index=0):
    """The pixels of image `index` of case d (a batch's images differ by their seed)."""
    w, h = d["w"], d["h"]
    seed = d["cseed"] + 7919 * index
    if d["kind"] == "png":
        return _content(d["content"], w * h * d["bpp"], seed)
    if d["content"] == "scene":
        return synth.scene(w, h, seed)
    if d["content"] == "photo":
        return synth.photo(w, h, seed)
    return _content(d["content"], w * h * (1 if d["ct"] == GRAY else 3), seed)


def pixels(d):
    """All input bytes of case d: one image, or a batch's images back to back."""
    if d.get("batch"):
        return np.concatenate([image(d, i).reshape(-1) for i in range(d["batch"])])
    return image(d).reshape(-1)


def oracle_options(d, O):
    return O.make_options(d["w"], d["h"], d["ct"], d["q"], d["ss"], restart=d["restart"], optimize_huffman=d["opt"],
                          progressive=d["prog"], trellis=d["trellis"])


def expected(d, O):
    """What the oracle makes of case d: a list of files (JPEG), a (y, cb, cr) tuple (coefficients) or (stream, adler32) (PNG)."""
    if d["kind"] == "png":
        return O.png_filter(image(d), d["w"], d["h"], d["bpp"], d["strategy"], stateful_fast=(d["h"] <= 32))
    if d["entry"].startswith("coefficients"):
        return O.coeffs(image(d), d["w"], d["h"], d["ct"], d["ss"], d["q"])
    if d["entry"] == "encode_jpeg":
        return [O.encode_flat(image(d), d["w"], d["h"], d["ct"], d["q"], d["preset"], d["ss"])]
    opts = oracle_options(d, O)
    return [O.encode(image(d, i), opts) for i in range(d.get("batch") or 1)]


if __name__ == "__main__":
    s, a, n = (int(x) for x in sys.argv[1:4])
    for d in cases(s, n, a, sys.argv[4] if len(sys.argv) > 4 and sys.argv[4] != "-" else None):
        print(json.dumps(d, sort_keys=True))
