"""The decoder model (tests/png_decode_model.py) pinned independently on well-formed files, where conventions coincide: Pillow
decodes the same file.  8-bit gray, gray+alpha, RGB and RGBA must be equal; palette files after convert("RGB") / ("RGBA");
sub-8-bit gray after Pillow's own scaling to "L".  16-bit files are compared with the high bytes of the raw stream instead:
Pillow keeps 16-bit gray as 16-bit and rescales other 16-bit files its own way, the reference keeps the high byte."""
import io
import zlib

import pytest

import png_decode_cases as PC
import png_decode_model as M

from PIL import Image

# (palettes are full here: for an index beyond PLTE Pillow has a convention of its own; the reference's is pinned in
# tests/test_emu_png_unfilter.py)
FILES = [("c%d_d%d_%dx%d" % (ct, d, w, h), PC.make(w, h, ct, d, seed=3 + i, trns=PC.trns_for(ct, d, w)))
         for (w, h) in [(1, 1), (7, 3), (67, 65), (33, 131)] for i, (ct, d) in enumerate(PC.COMBOS)] + list(PC.layout_cases())[:13]
MODES = {M.OUT_GRAY: "L", M.OUT_GRAY_ALPHA: "LA", M.OUT_RGB: "RGB", M.OUT_RGBA: "RGBA"}


@pytest.mark.parametrize("name,png", FILES, ids=[n for n, _ in FILES])
def test_model_agrees_with_an_independent_decoder(name, png):
    w, h, pixels, ct = PC.model(png)
    f = M.walk(png)
    if f["depth"] == 16:
        rb = M.row_bytes(f["color_type"], 16, w)
        raw = M.reconstruct(zlib.decompress(f["idat"]), h, rb, M.filter_unit(f["color_type"], 16))
        assert pixels == raw[0::2]
        return
    im = Image.open(io.BytesIO(png))
    im.load()
    assert im.size == (w, h)
    assert im.convert(MODES[ct]).tobytes() == pixels


def test_paeth_ties_and_scaling_follow_the_specification():
    assert [M.paeth(*t) for t in [(5, 5, 5), (10, 10, 12), (11, 8, 10), (100, 50, 50), (50, 100, 50), (50, 50, 100)]] == [5, 10, 8, 100, 100, 50]
    assert [M.scale_to_8bit(s, 2) for s in range(4)] == [0, 85, 170, 255]
    assert M.scale_to_8bit(8, 4) == 0x88 and M.scale_to_8bit(1, 1) == 255
