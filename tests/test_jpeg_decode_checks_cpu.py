"""JPEG decode without a GPU: every refusal with its status and message, the order of the checks, `decode_jpeg_info`,
`decode_jpeg_batch_info` and the plan (one launch per class present whatever N, the sub-batch cut), and the host's entropy
decoder — `pixo_hip_debug_jpeg_decode_coefficients` — against the sequential model on every case and against the coefficients
the oracle wrote into its own files, which pins the entropy decode independently of any IDCT."""
import glob
import os

import numpy as np
import pytest

import jpeg_decode_cases as JC
import jpeg_decode_model as M
import oracle_lib as O
import synth
from pixo_amd import ColorType, decode, error, jpeg

INVALID, UNSUPPORTED = error.InvalidDecode, error.UnsupportedDecode
GOOD = JC.data(JC.by_name("420_50x37_q80"))
GRAY = JC.data(JC.by_name("gray_9x9_q80"))


def segment(d, marker, nth=0):
    """(start of the marker's 0xFF, end of its segment) of the nth segment with this marker in front of the scan"""
    p = 2
    while True:
        assert d[p] == 0xFF
        m, n = d[p + 1], (d[p + 2] << 8) | d[p + 3]
        if m == marker:
            if nth == 0:
                return p, p + 2 + n
            nth -= 1
        assert m != 0xDA, "no such segment"
        p += 2 + n


def patched(d, marker, at, value, nth=0):
    """Byte `at` of the segment's payload (behind its length) set to `value`"""
    a, _ = segment(d, marker, nth)
    return d[:a + 4 + at] + bytes([value]) + d[a + 5 + at:]


def relength(d, marker, payload, nth=0):
    """The segment replaced by one with this payload"""
    a, b = segment(d, marker, nth)
    return d[:a + 2] + (len(payload) + 2).to_bytes(2, "big") + payload + d[b:]


def payload(d, marker, nth=0):
    a, b = segment(d, marker, nth)
    return d[a + 4:b]


def seg(marker, body):
    return bytes([0xFF, marker]) + (len(body) + 2).to_bytes(2, "big") + body


def tiny_gray(scan, dc=(1, [0]), ac=(1, [0xF1]), w=8, h=8):
    """One gray block; the DC and AC tables hold one code of one bit each ('0'), for the given symbols"""
    def dht(cls, length, vals):
        bits = [0] * 16
        bits[length - 1] = len(vals)
        return seg(0xC4, bytes([cls << 4]) + bytes(bits) + bytes(vals))
    return (b"\xff\xd8" + seg(0xDB, b"\x00" + b"\x01" * 64) + seg(0xC0, bytes([8, h >> 8, h & 255, w >> 8, w & 255, 1, 1, 0x11, 0]))
            + dht(0, *dc) + dht(1, *ac) + seg(0xDA, bytes([1, 1, 0x00, 0, 63, 0])) + scan + b"\xff\xd9")


def adobe(transform):
    return seg(0xEE, b"Adobe\x00\x64\x00\x00\x00\x00" + bytes([transform]))


SOF, DHT, DQT, DRI, SOS = 0xC0, 0xC4, 0xDB, 0xDD, 0xDA
sof = payload(GOOD, SOF)
REFUSALS = [
    # ---- the reference's, in its words ----
    ("empty", b"", INVALID, "not a JPEG file"),
    ("png", b"\x89PNG\r\n\x1a\n", INVALID, "not a JPEG file"),
    ("soi_only", b"\xff\xd8", INVALID, "unexpected end of file"),
    ("soi_eoi", b"\xff\xd8\xff\xd9", INVALID, "no image data found"),
    ("zero_dimensions_no_scan", b"\xff\xd8" + seg(DQT, b"\x00" + b"\x10" * 64) + seg(SOF, bytes([8, 0, 0, 0, 8, 1, 1, 0x11, 0])) + b"\xff\xd9",
     INVALID, "no image data found"),
    ("truncated_marker", b"\xff\xd8\xff\xdb\x00", INVALID, "truncated marker"),
    ("length_one", b"\xff\xd8\xff\xdb\x00\x01", INVALID, "invalid marker length"),
    ("length_beyond_file", GOOD[:40], INVALID, "invalid marker length"),
    ("progressive", GOOD[:2] + seg(0xC2, sof) + GOOD[2:], UNSUPPORTED, "progressive JPEG not supported"),
    ("precision", patched(GOOD, SOF, 0, 12), UNSUPPORTED, "12-bit precision not supported"),
    ("precision_before_components", patched(patched(GOOD, SOF, 0, 12), SOF, 5, 4), UNSUPPORTED, "12-bit precision not supported"),
    ("components", patched(GOOD, SOF, 5, 4), UNSUPPORTED, "4 components not supported"),
    ("sof0_length", relength(GOOD, SOF, sof[:7]), INVALID, "invalid SOF0 length"),
    ("sof0_truncated", relength(GOOD, SOF, sof[:12]), INVALID, "truncated SOF0 components"),
    ("sampling_zero", patched(GOOD, SOF, 7, 0x02), INVALID, "invalid sampling factors 0x2 for component 1"),
    ("sof0_table_id", patched(GOOD, SOF, 8, 7), INVALID, "invalid quantization table ID 7 for component 1"),
    ("dqt_id", patched(GOOD, DQT, 0, 0x05), INVALID, "invalid quantization table ID"),
    ("dqt_truncated", relength(GOOD, DQT, payload(GOOD, DQT)[:40]), INVALID, "truncated DQT"),
    ("dht_id", patched(GOOD, DHT, 0, 0x04), INVALID, "invalid Huffman table ID"),
    ("dht_truncated", relength(GOOD, DHT, payload(GOOD, DHT)[:9]), INVALID, "truncated DHT"),
    ("dht_values", relength(GOOD, DHT, payload(GOOD, DHT)[:20]), INVALID, "truncated DHT values"),
    ("dri_length", GOOD[:2] + seg(DRI, b"\x00\x01\x00") + GOOD[2:], INVALID, "invalid DRI length"),
    ("sos_empty", relength(GOOD, SOS, b""), INVALID, "empty SOS segment"),
    ("sos_count", patched(GOOD, SOS, 0, 2), INVALID, "SOS component count mismatch"),
    ("sos_truncated", relength(GOOD, SOS, payload(GOOD, SOS)[:5]), INVALID, "truncated SOS segment"),
    ("sos_dc_id", patched(GOOD, SOS, 2, 0x50), INVALID, "invalid DC Huffman table ID 5 for component 1"),
    ("sos_ac_id", patched(GOOD, SOS, 2, 0x06), INVALID, "invalid AC Huffman table ID 6 for component 1"),
    # ---- this library's ----
    ("sos_before_sof0", b"\xff\xd8" + seg(SOS, b"\x00\x00\x3f\x00") + b"\x00\xff\xd9", INVALID, "SOS before SOF0"),
    ("sampling_440", patched(GOOD, SOF, 7, 0x12), UNSUPPORTED, "sampling factors 1x2 1x1 1x1 not supported"),
    ("sampling_411", patched(GOOD, SOF, 7, 0x41), UNSUPPORTED, "sampling factors 4x1 1x1 1x1 not supported"),
    ("sampling_chroma", patched(GOOD, SOF, 10, 0x21), UNSUPPORTED, "sampling factors 2x2 2x1 1x1 not supported"),
    ("scan_components", patched(GOOD, SOS, 1, 9), UNSUPPORTED, "a scan that does not hold all components in frame order is not supported"),
    ("adobe_transform_0", GOOD[:2] + adobe(0) + GOOD[2:], UNSUPPORTED, "Adobe colour transform 0 not supported"),
    ("rgb_ids", patched(patched(patched(patched(patched(patched(GOOD, SOF, 6, 82), SOF, 9, 71), SOF, 12, 66), SOS, 1, 82), SOS, 3, 71), SOS, 5, 66),
     UNSUPPORTED, "RGB component ids not supported"),
    ("no_quant_table", patched(GOOD, SOF, 8, 3), INVALID, "quantization table 3 is not defined"),
    ("no_dc_table", patched(GOOD, SOS, 2, 0x20), INVALID, "DC Huffman table 2 is not defined"),
    ("no_ac_table", patched(GOOD, SOS, 2, 0x03), INVALID, "AC Huffman table 3 is not defined"),
    ("scan_too_short_for_the_frame", patched(patched(GOOD, SOF, 1, 0xFF), SOF, 3, 0xFF), INVALID, "entropy-coded segment ends early"),
    ("dht_no_prefix_code", relength(GRAY, DHT, b"\x00" + bytes([3] + [0] * 15) + b"\x00\x01\x02"), INVALID, "invalid Huffman code lengths"),
]


@pytest.mark.parametrize("name,data,kind,msg", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_walk_refusals_have_their_status_and_message(name, data, kind, msg):
    prefix = "Decode error: " if kind is INVALID else "Unsupported: "
    for call in (decode.decode_jpeg_info, decode.decode_jpeg, lambda d: decode.decode_jpeg_coefficients(d, 0)):
        with pytest.raises(kind) as e:
            call(data)
        assert str(e.value) == prefix + msg
    with pytest.raises(kind) as e:
        decode.decode_jpeg_batch_info([GOOD, data])
    assert str(e.value) == prefix + msg + " (image 1)"


rst = JC.data(JC.by_name("420_50x37_q80_rst1"))
first_rst = rst.index(b"\xff\xd0", segment(rst, SOS)[1])
SCAN_REFUSALS = [
    ("truncated", GOOD[:-60], "entropy-coded segment ends early"),
    ("cut_behind_sos", GOOD[:segment(GOOD, SOS)[1] + 30] + b"\xff\xd9", "entropy-coded segment ends early"),
    ("rst_out_of_sequence", rst[:first_rst + 1] + b"\xd1" + rst[first_rst + 2:], "missing or out-of-sequence restart marker"),
    ("rst_missing", rst[:first_rst] + rst[first_rst + 2:], "missing or out-of-sequence restart marker"),
    ("rst_too_early", patched(rst, DRI, 1, 2), "entropy-coded segment ends early"),
    ("index_past_63", tiny_gray(b"\x2a\xbf"), "coefficient index past 63"),
    ("code_in_no_table", tiny_gray(b"\xff\x00\xff\x00\xff\x00"), "Huffman code not in the table"),
]


@pytest.mark.parametrize("name,data,msg", SCAN_REFUSALS, ids=[r[0] for r in SCAN_REFUSALS])
def test_scan_refusals_have_their_status_and_message(name, data, msg):
    decode.decode_jpeg_info(data)  # the walk has nothing to say
    with pytest.raises(INVALID) as e:
        decode.decode_jpeg_coefficients(data, 0)
    assert str(e.value) == "Decode error: " + msg
    with pytest.raises(M.Refused) as m:  # ... and the model agrees
        M.decode(data)
    assert str(m.value) == "Decode error: " + msg


def test_tiny_file_decodes_when_its_scan_is_sound():
    """The crafted one-block file the refusals above are made from, with an end of block in its AC table"""
    ok = tiny_gray(b"\x17\xff\x00", ac=(2, [0xF1, 0x00]))  # codes 00 -> (15, 1), 01 -> end of block: 0 | 00 1 | 01 | 11 pad
    z = decode.decode_jpeg_coefficients(ok, 0)
    assert z.shape == (1, 1, 64) and z[0, 0, 16] == 1 and np.count_nonzero(z) == 1
    assert np.array_equal(M.coefficients(ok)[1][0], z)


def test_order_of_checks_and_batch_head():
    with pytest.raises(error.CompressionError, match="batch must be 1..65535"):
        decode.decode_jpeg_batch_info([])
    # the file with the lowest index answers, in phase 1 whatever a later file holds
    with pytest.raises(UNSUPPORTED) as e:
        decode.decode_jpeg_batch_info([GOOD, patched(GOOD, SOF, 0, 12), b"", GOOD[:40]])
    assert str(e.value) == "Unsupported: 12-bit precision not supported (image 1)"
    # a file's own order: the segment in front answers
    both = patched(patched(GOOD, DQT, 0, 0x05), SOF, 0, 12)
    with pytest.raises(INVALID, match="invalid quantization table ID"):
        decode.decode_jpeg_info(both)


def test_zero_height_with_a_scan_is_no_special_case():
    """The reference decodes such a file to an image without pixels; so does the walk here (no MCUs, no tiles, no bytes)"""
    f = tiny_gray(b"\x00", h=0)
    assert decode.decode_jpeg_info(f) == (8, 0, ColorType.Gray)
    assert decode.decode_jpeg_coefficients(f, 0).size == 0
    layout, total = decode.decode_jpeg_batch_info([f, GRAY])
    assert layout[0][3] == layout[1][3] == 0 and total == 81


def test_info_and_batch_layout():
    files = [JC.data(c) for c in JC.CASES]
    layout, total = decode.decode_jpeg_batch_info(files)
    at = 0
    for c, (w, h, ct, offset) in zip(JC.CASES, layout):
        assert decode.decode_jpeg_info(JC.data(c)) == (w, h, ct) == (c["w"], c["h"], ColorType(c["color_type"]))
        assert offset == at and offset % 16 == 0
        end = at + w * h * (c["color_type"] + 1)
        at = (end + 15) // 16 * 16
    assert total == end
    assert decode.decode_jpeg_tile_mcus() == JC.TILE_MCUS


def test_plan_one_launch_per_class_whatever_n():
    by_mode = {m: [JC.data(c) for c in JC.CASES if c["mode"] == m][:5] for m in JC.MCU}
    for modes in (["gray"], ["420"], ["gray", "444"], ["444", "422", "420"], ["gray", "444", "422", "420"]):
        for repeat in (1, 40):
            files = [f for m in modes for f in by_mode[m]] * repeat
            plan = decode.decode_jpeg_batch_plan(files)
            assert plan["launches"] == len(modes) and plan["sub_first"] == [0, len(files)]
            assert set(plan["classes"]) == set(modes)
            assert plan["threads"] == min(8, len(files))
            assert decode.decode_jpeg_batch_plan(files, one_thread=True)["threads"] == 1


def test_plan_cuts_sub_batches_by_coefficient_bytes():
    """Every 50x37 4:2:0 image holds 16 MCUs = 64 + 16 + 16 blocks, each plane rounded up to 64 blocks: 192 blocks, 24,576 bytes.
    A limit of 50,000 bytes holds two."""
    files = [JC.data(JC.by_name("420_50x37_q80"))] * 5 + [JC.data(JC.by_name("gray_50x37_q80"))] * 3
    jpeg.debug_configure("decode_batch_bytes=50000")
    try:
        plan = decode.decode_jpeg_batch_plan(files)
    finally:
        jpeg.debug_configure("")
    assert plan["sub_first"] == [0, 2, 4, 8]  # (a gray 50x37 image: 35 blocks -> 64, 8,192 bytes)
    assert plan["launches"] == 4  # 4:2:0, 4:2:0, then 4:2:0 and gray


@pytest.mark.parametrize("c", JC.CASES, ids=JC.IDS)
def test_coefficients_are_the_models(c):
    f, coefs = JC.model(c)
    for ci in range(len(coefs)):
        got = decode.decode_jpeg_coefficients(JC.data(c), ci)
        assert got.shape == coefs[ci].shape and np.array_equal(got, coefs[ci]), ci


@pytest.mark.parametrize("ct,ss", [(0, 0), (2, 0), (2, 1)], ids=["gray", "444", "420"])
def test_coefficients_are_what_the_oracle_wrote(ct, ss):
    """Files the oracle encodes (standard and optimised tables, restart intervals): the decoder reads back the coefficients
    the oracle computed — no IDCT, no model involved."""
    for (w, h, seed) in [(50, 37, 5), (16, 16, 6), (33, 17, 7)]:
        px = synth.noise_gray(w, h, seed) if ct == 0 else synth.noise(w, h, seed)
        y, cb, cr = O.coeffs(px, w, h, ct, ss, 75)
        zz = lambda a: a[:, M.ZIGZAG]
        for kw in (dict(), dict(optimize_huffman=True), dict(restart=1), dict(restart=5, optimize_huffman=True)):
            f = O.encode(px, O.make_options(w, h, ct, 75, ss, **kw))
            got = decode.decode_jpeg_coefficients(f, 0)
            if ss == 1:  # the oracle's luma: TL, TR, BL, BR per MCU in raster MCU order
                my, mx = got.shape[0] // 2, got.shape[1] // 2
                want = zz(y).reshape(my, mx, 2, 2, 64).transpose(0, 2, 1, 3, 4).reshape(2 * my, 2 * mx, 64)
            else:
                want = zz(y).reshape(got.shape)
            assert np.array_equal(got, want), kw
            if ct:
                for ci, plane in ((1, cb), (2, cr)):
                    got = decode.decode_jpeg_coefficients(f, ci)
                    assert np.array_equal(got, zz(plane).reshape(got.shape)), (kw, ci)


def test_reference_made_files_are_read_or_refused():
    """The reference's own files (tests/golden/jpeg/): the walk accepts every baseline one; the progressive ones are refused
    with the reference's message."""
    for path in sorted(glob.glob(os.path.join(JC.HERE, "golden", "jpeg", "*.jpg")))[::4]:
        with open(path, "rb") as f:
            data = f.read()
        w, h, ct = decode.decode_jpeg_info(data)
        fm, coefs = M.coefficients(data)
        assert (w, h) == (fm.width, fm.height)
        for ci in range(len(coefs)):
            assert np.array_equal(decode.decode_jpeg_coefficients(data, ci), coefs[ci]), os.path.basename(path)
    for path in sorted(glob.glob(os.path.join(JC.HERE, "golden", "jpeg_p2", "*.jpg")))[:5]:
        with open(path, "rb") as f:
            with pytest.raises(UNSUPPORTED, match="progressive JPEG not supported"):
                decode.decode_jpeg_info(f.read())
