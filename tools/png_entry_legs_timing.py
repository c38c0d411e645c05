"""Per-call wall time of the PNG, zlib and resize entry points (the host layer between the C ABI and the kernels), one JSON line.
The sibling of entry_legs_timing.py for A/B runs of two builds of the same C ABI: run once per build with PIXO_HIP_LIB=<library>,
alternating, in one session on one card; the spread of the same build against itself is the margin.
    python tools/png_entry_legs_timing.py [label]"""
import json, os, sys
root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, root); sys.path.insert(0, os.path.join(root, "tests")); sys.path.insert(0, os.path.join(root, "tools"))
import torch
import synth
from entry_legs_timing import median_us
from pixo_amd import ColorType, png, resize


def main():
    label = sys.argv[1] if len(sys.argv) > 1 else "build"
    dev = torch.device("cuda:0")
    out = {"label": label, "lib": os.environ.get("PIXO_HIP_LIB", "in-tree")}
    # 4096x4096 RGBA: whole files from device and host pixels, the prepared stream, the row filters through the band path
    w = h = 4096
    px = synth.rgba_noise_alpha1(w, h, 7)
    o = png.PngOptions.from_preset(w, h, 1)
    d = torch.from_numpy(px).to(dev)
    d_out = torch.empty(o.full_size(), dtype=torch.uint8, device=dev); torch.cuda.synchronize()
    out["4096_png_encode_device"] = median_us(lambda: png.encode_device(d, o), 3, 20)
    out["4096_png_encode_host"] = median_us(lambda: png.encode(px, o), 3, 20)
    out["4096_png_prepare_device"] = median_us(lambda: png.prepare_device(d, o, d_out), 5, 60)
    out["4096_png_apply_filters_bands"] = median_us(lambda: png.apply_filters(px, w, h, 4), 3, 20)
    # a few MiB through the device zlib stage alone
    n = 6 << 20
    cap = png.stored_bound(n)
    d_z = torch.empty(cap, dtype=torch.uint8, device=dev); torch.cuda.synchronize()
    out["6MiB_zlib_compress_device"] = median_us(lambda: png.zlib_compress_device(d, n, d_z, cap, bpp=4, row=4 * w + 1), 5, 60)
    del d, d_out, d_z
    # small calls, where a fixed cost per call of the DEFLATE tail shows: whole files of 64x64 and 256x256 RGB at preset 0, 4 KiB of zlib
    for side in (64, 256):
        d_s = torch.from_numpy(synth.scene(side, side, 31)).to(dev)
        os_ = png.PngOptions.builder(side, side).color_type(ColorType.Rgb).preset(0).build(); torch.cuda.synchronize()
        out["%dx%d_png_encode_device" % (side, side)] = median_us(lambda: png.encode_device(d_s, os_), 50, 1000)
    d_4k = torch.from_numpy(synth.scene(64, 64, 31)[:4096].copy()).to(dev)
    d_z = torch.empty(png.stored_bound(4096), dtype=torch.uint8, device=dev); torch.cuda.synchronize()
    out["4KiB_zlib_compress_device"] = median_us(lambda: png.zlib_compress_device(d_4k, 4096, d_z, d_z.numel()), 50, 1000)
    # a batch: the 64 x 256x256 photo row of png_batch_timing.py, preset 0
    import numpy as np
    from png_batch_timing import images
    d_all = torch.from_numpy(np.concatenate(images("photo", 64, 256, 256))).to(dev)
    ob = png.PngOptions.builder(256, 256).color_type(ColorType.Rgb).preset(0).build(); torch.cuda.synchronize()
    out["64x256x256_png_encode_batch_device"] = median_us(lambda: png.encode_batch_device(d_all, ob, 64), 3, 30)
    del d_s, d_4k, d_z, d_all
    # a small image: the fixed cost per call of the row filters
    sw, sh = 200, 150
    small = synth.rgba_noise_alpha1(sw, sh, 3)
    out["200x150_png_apply_filters"] = median_us(lambda: png.apply_filters(small, sw, sh, 4), 50, 1000)
    # Lanczos3, host and device pixels: 1080p -> 720p, and 64x64 -> 32x32 where the host layer is most of the call
    for name, (a, b, c, e), (warm, reps) in (("1080p_to_720p", (1920, 1080, 1280, 720), (10, 100)), ("64_to_32", (64, 64, 32, 32), (50, 1000))):
        src = synth.noise(a, b, 5)
        ro = resize.ResizeOptions.builder(a, b).dst(c, e).color_type(ColorType.Rgb).algorithm(resize.ResizeAlgorithm.Lanczos3).build()
        d_src = torch.from_numpy(src).to(dev)
        d_dst = torch.empty(ro.output_len(), dtype=torch.uint8, device=dev); torch.cuda.synchronize()

        def on_device():
            resize.resize_device(d_src, ro, d_dst)
            torch.cuda.synchronize()
        out["resize_lanczos3_%s_host" % name] = median_us(lambda: resize.resize(src, ro), warm, reps)
        out["resize_lanczos3_%s_device" % name] = median_us(on_device, warm, reps)
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
