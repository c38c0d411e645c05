"""JPEG decode of the files no encoder writes, without a GPU: the test writer (tests/jpeg_write.py) round-trips through the
sequential model; the model gives the committed libjpeg-turbo pixels of every structural case (tests/jpeg_decode_cases.py
SYNTH); the library's walk, entropy decoder and records read those files as the model does; the generator reruns to the
committed bytes; and the arithmetic cases (tests/jpeg_decode_arith.py) — the model against a live Pillow where that is built on
libjpeg-turbo.  The kernel's own code runs over the same cases in tests/test_emu_jpeg_decode.py."""
import filecmp
import io
import os
import sys
import zlib

import numpy as np
import pytest

import jpeg_decode_arith as AR
import jpeg_decode_cases as JC
import jpeg_decode_model as M
import jpeg_write as W
from pixo_amd import decode, error


def turbo():
    from PIL import features
    return features.check_feature("libjpeg_turbo")


def pillow(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)))


def natural(z):
    out = np.zeros(z.shape, np.int64)
    out[..., M.ZIGZAG] = z
    return out


# ---- the writer ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", JC.SYNTH, ids=JC.SYNTH_IDS)
def test_writer_round_trips_every_structural_case(c):
    """x = the case's coefficients, frame and tables: coefficients(write(x)) == x — with the writer's default segments and
    optimal tables, and once more with a restart interval of 2 and every used table forced onto codes of 9 to 16 bits"""
    f, x = JC.model(c)
    comps = [dict(id=k["id"], h=k["h"], v=k["v"], tq=k["tq"], td=k["td"], ta=k["ta"]) for k in f.comps]
    q = {t: natural(np.array(v)) for t, v in f.q.items()}
    keys = {(0, k["td"]) for k in comps} | {(1, k["ta"]) for k in comps}
    for kw in (dict(), dict(restart=2, huff={k: W.long_codes_table for k in keys}, rst_fill=lambda i: i % 3)):
        g, y = M.coefficients(W.write(f.width, f.height, comps, q, [natural(a) for a in x], **kw))
        assert (g.width, g.height, g.restart) == (f.width, f.height, kw.get("restart", 0))
        assert len(y) == len(x) and all(np.array_equal(a, b) for a, b in zip(x, y))


def test_writer_codes_every_magnitude_run_and_block_end():
    """DC differences of every category 0..11, AC sizes 1..10 at every run 0..15 the block has room for, ZRL up to three in a row
    and blocks that end with and without an end of block, through the general and the DC-only path of the writer"""
    rng = np.random.default_rng(3)
    blocks = []
    for size in range(1, 11):
        for run in range(0, 62):
            z = np.zeros(64, np.int64)
            z[1 + run] = rng.choice([-1, 1]) * rng.integers(1 << (size - 1), 1 << size)
            if run % 2:
                z[63] = 1
            blocks.append(z)
    dc = [0, 1, -1, 2, -3, 4, -7, 8, -15, 16, -31, 32, -63, 64, -127, 128, -255, 256, -511, 512, -1023, 1024, -1023, 1024, -1023]
    for i, z in enumerate(blocks):
        z[0] = dc[i % len(dc)]
    zz = np.zeros((-(-len(blocks) // 20) * 20, 64), np.int64)
    zz[:len(blocks)] = blocks
    x = [natural(zz.reshape(-1, 20, 64))]  # (the blocks above were filled in zigzag order)
    info = {}
    data = W.write(160, x[0].shape[0] * 8, W.gray(), {0: AR.ONES}, x, info=info)
    assert set(range(12)) <= set(info["symbols"][(0, 0)]) and W.ZRL in info["symbols"][(1, 0)] and W.EOB in info["symbols"][(1, 0)]
    assert {s & 15 for s in info["symbols"][(1, 0)]} >= set(range(1, 11)) and {s >> 4 for s in info["symbols"][(1, 0)]} == set(range(16))
    assert np.array_equal(M.coefficients(data)[1][0], x[0][..., M.ZIGZAG])
    only_dc = [np.zeros_like(x[0])]
    only_dc[0][..., 0] = x[0][..., 0]
    assert np.array_equal(M.coefficients(W.write(160, x[0].shape[0] * 8, W.gray(), {0: AR.ONES}, only_dc))[1][0], only_dc[0][..., M.ZIGZAG])


def test_writer_tables():
    assert W.optimal_table({5: 10}) == ([1] + [0] * 15, [5])
    bits, vals = W.optimal_table({s: 1 << s for s in range(20)})  # Fibonacci-like counts: lengths beyond 16 are folded back
    assert max(n + 1 for n in range(16) if bits[n]) == 16 and sorted(vals) == list(range(20))
    full = W.codes_of(*W.optimal_table({0: 5, 1: 3, 2: 1, 3: 1}, reserve=False))
    assert max(full.values(), key=lambda cl: cl[1]) and any(code == (1 << n) - 1 for code, n in full.values()), "the last code word is all ones"
    kept = W.codes_of(*W.optimal_table({0: 5, 1: 3, 2: 1, 3: 1}))
    assert not any(code == (1 << n) - 1 for code, n in kept.values())
    assert all(n >= 9 for _, n in W.codes_of(*W.long_codes_table({s: s + 1 for s in range(40)})).values())


# ---- the structural cases ------------------------------------------------------------------------------------------------------
def test_every_case_of_the_issue_is_there():
    names = " ".join(JC.SYNTH_IDS)
    for part in ("q3_012_444", "q3_012_422", "q3_012_420", "q3_302_444", "q3_302_422", "q3_302_420", "huff3_012_012_4", "huff3_302_230_4",
                 "ids_0_1_2_", "ids_10_200_3_", "ids_89_67_99_", "gray_written_2x2", "one_dqt_one_dht_gray", "one_dqt_one_dht_444", "one_dqt_one_dht_422",
                 "one_dqt_one_dht_420", "dqt_twice", "dht_twice", "dqt_8_16_8_bit", "codes_9_to_16_bits", "code_of_16_bits", "single_symbol_tables_flat",
                 "single_symbol_dc_steps", "last_code_all_ones", "no_eob_63_acs", "three_zrl_then_k63", "two_zrl_then_tail_without_eob", "dc_category_11",
                 "ac_size_10", "rst1_fill_bytes_gray", "rst1_fill_bytes_420", "rst_interval_is_mcu_count", "rst_interval_above_mcu_count", "dri_4_then_dri_0",
                 "dri_0_then_dri_3", "last_scan_byte_is_stuffed_ff", "trailer_100_bytes", "no_eoi"):
        assert part in names, part
    assert len(JC.SYNTH) >= 45 and not set(JC.SYNTH_IDS) & set(JC.IDS)
    sizes = [os.path.getsize(JC.path(c)) for c in JC.SYNTH]
    assert max(sizes) < 8192


@pytest.mark.parametrize("c", JC.SYNTH, ids=JC.SYNTH_IDS)
def test_model_is_the_committed_expectation(c):
    w, h, px, ct = M.decode(JC.data(c))
    assert (w, h, ct) == (c["w"], c["h"], c["color_type"])
    assert JC.mismatch(px.tobytes(), c) == ""


def test_live_pillow_gives_the_committed_pixels_or_refuses_as_recorded():
    if not turbo():
        pytest.skip("this Pillow is not built on libjpeg-turbo")
    refused = 0
    for c in JC.SYNTH:
        if "pillow" in c:
            with pytest.raises(OSError) as e:
                pillow(JC.data(c))
            assert c["pillow"].startswith("refuses: " + str(e.value)), c["name"]
            refused += 1
        else:
            assert pillow(JC.data(c)).tobytes() == JC.expected(c), c["name"]
    assert refused == 3  # two tables that use the all-ones code word, one file without EOI


def test_generator_reruns_to_the_committed_bytes(tmp_path):
    if not turbo():
        pytest.skip("this Pillow is not built on libjpeg-turbo")
    sys.path.insert(0, os.path.join(JC.HERE, "golden"))
    try:
        import make_golden_jpeg_decode_synth as G
    finally:
        sys.path.pop(0)
    out = tmp_path / "jpeg_decode_synth"
    G.main(str(out), str(tmp_path / "cases.json"))
    names = sorted(os.listdir(JC.SYNTH_DIR))
    assert names == sorted(os.listdir(out)) and len(names) == 2 * len(JC.SYNTH)
    assert filecmp.cmpfiles(JC.SYNTH_DIR, out, [n for n in names if n.endswith(".jpg")], shallow=False)[1:] == ([], [])
    for n in names:  # (the pixels, not their compressed form: that is the zlib build's business)
        if n.endswith(".px.z"):
            with open(os.path.join(JC.SYNTH_DIR, n), "rb") as a, open(out / n, "rb") as b:
                assert zlib.decompress(a.read()) == zlib.decompress(b.read()), n
    assert filecmp.cmp(tmp_path / "cases.json", os.path.join(JC.HERE, "golden", "jpeg_decode_synth_cases.json"), shallow=False)


@pytest.mark.parametrize("c", JC.SYNTH, ids=JC.SYNTH_IDS)
def test_library_reads_frame_and_coefficients_as_the_model_does(c):
    f, coefs = JC.model(c)
    assert decode.decode_jpeg_info(JC.data(c)) == (c["w"], c["h"], c["color_type"])
    for ci in range(len(coefs)):
        got = decode.decode_jpeg_coefficients(JC.data(c), ci)
        assert got.shape == coefs[ci].shape and np.array_equal(got, coefs[ci]), ci


def test_records_carry_each_components_own_quantisation_table():
    """What the batch driver hands the kernel: component c's table is the one its `tq` names — three distinct tables in a file,
    beside ordinary files"""
    cases = JC.SYNTH + JC.small()[:6]
    got = decode.decode_jpeg_batch_tables([JC.data(c) for c in cases])
    distinct = 0
    for c, tables in zip(cases, got):
        f, coefs = JC.model(c)
        for ci in range(3):
            want = natural(np.array(f.q[f.comps[ci]["tq"]])) if ci < len(coefs) else np.zeros(64)
            assert np.array_equal(tables[ci], want), (c["name"], ci)
        distinct += len(coefs) == 3 and not np.array_equal(tables[1], tables[2])
    assert distinct >= 8


def test_sampling_factors_that_are_multiples_of_the_canonical_ones_are_refused():
    """4x4 2x2 2x2 describes the 4:2:0 geometry too; it is refused with the walk's message (Pillow refuses it as a broken data
    stream: libjpeg allows ten blocks to an MCU)"""
    d = JC.data(JC.by_name("ids_0_1_2_420_50x37"))
    at = d.index(b"\xff\xc0") + 4 + 6
    assert d[at + 1] == 0x22 and d[at + 4] == 0x11 and d[at + 7] == 0x11
    bad = d[:at + 1] + b"\x44" + d[at + 2:at + 4] + b"\x22" + d[at + 5:at + 7] + b"\x22" + d[at + 8:]
    with pytest.raises(error.UnsupportedDecode) as e:
        decode.decode_jpeg_info(bad)
    assert str(e.value) == "Unsupported: sampling factors 4x4 2x2 2x2 not supported"


# ---- the arithmetic cases: the model against live Pillow ------------------------------------------------------------------------
def test_largest_lone_amplitudes_are_what_the_header_states():
    """The largest lone dequantised coefficient that keeps every descaled sample in -512..511 (condition (b) of
    jpeg_decode_math.h), from the model's unclamped output: DC -4100 .. +4091; AC, either sign, from 2126 at (1, 1) to 4091 at
    (0, 4), (4, 0) and (4, 4), which scale like the DC"""
    k = np.arange(64)
    plus, minus = AR.largest_lone(k, np.ones(64, int), np.zeros(64, int)), AR.largest_lone(k, -np.ones(64, int), np.zeros(64, int))
    assert (plus[0], minus[0]) == (4091, 4100)
    assert np.array_equal(plus[1:], minus[1:]) and (plus[1:].min(), plus[1:].max()) == (2126, 4091)
    assert (plus[1], plus[8], plus[9], plus[63], plus[4], plus[32], plus[36]) == (2950, 2949, 2126, 2126, 4091, 4091, 4091)


@pytest.mark.parametrize("q", [1, 4])
def test_idct_sweep_model_is_live_pillow(q):
    """q = 1 reaches a magnitude of 1023 only — baseline Huffman coding holds no larger coefficient —, so the same sweep is also
    written with a flat table of 4, where the quantised magnitude of at most 1023 reaches every largest lone amplitude to within 3"""
    data, want, blocks = AR.idct_sweep(q)
    assert blocks == 2 * 2 * 64 + 2 * 2 * 2 * 63 + 200
    f, coefs = M.coefficients(data)
    assert f.q[0] == [q] * 64 and data[data.index(b"\xff\xdb") + 4] == 0x10 and coefs[0].shape[1] == 33
    d = np.abs(coefs[0] * q)
    assert d.max() == (1023 if q == 1 else 4092)  # (-4092 at the DC; 4088 elsewhere)
    assert M.decode(data)[2].tobytes() == want.tobytes()
    if not turbo():
        pytest.skip("this Pillow is not built on libjpeg-turbo")
    assert pillow(data).tobytes() == want.tobytes()


@pytest.mark.parametrize("name", AR.SCALED)
def test_scaled_tables_model_is_live_pillow_up_to_times_4(name):
    if not turbo():
        pytest.skip("this Pillow is not built on libjpeg-turbo")
    for factor in (2, 4):
        data, want = AR.scaled(name, factor)
        assert pillow(data).tobytes() == want.tobytes(), factor
    data, want = AR.scaled(name, 16)
    print("%s x16: %d of %d bytes differ from Pillow's (beyond -512..511 libjpeg's table wraps, the model clamps)" % (name, int((pillow(data) != want).sum()), want.size))


@pytest.mark.parametrize("name", AR.COLOUR_IMAGES)
def test_colour_images_formula_is_the_model_and_live_pillow(name):
    data, want = AR.colour_image(name)
    f, coefs = M.coefficients(AR.colour_image(name, range(100, 104))[0])
    assert np.array_equal(M.pixels(f, coefs)[2][::8, ::8], AR.colour_image(name, range(100, 104))[1])
    if not turbo():
        pytest.skip("this Pillow is not built on libjpeg-turbo")
    px = pillow(data)
    assert px.shape == (2048, 2048, 3)
    assert np.array_equal(px.reshape(256, 8, 256, 8, 3), np.broadcast_to(want[:, None, :, None, :], (256, 8, 256, 8, 3)))


def test_no_pixel_tells_fix_1_402_from_its_neighbours():
    """jdcolor's FIX(1.40200) = 91881 changed by one gives the same red for every Cr: no test of pixels can pin its last unit"""
    cr = np.arange(-128, 128)
    for k in (91880, 91882):
        assert np.array_equal((91881 * cr + 32768) >> 16, (k * cr + 32768) >> 16)
    assert not np.array_equal((91881 * cr + 32768) >> 16, (91900 * cr + 32768) >> 16)


@pytest.mark.parametrize("mode,trim", [("422", 1), ("422", 2), ("420", 1), ("420", 2)])
def test_upsampler_stripes_expectation_is_the_model_and_live_pillow(mode, trim):
    few = AR.LATTICE[::37] + AR.LATTICE[-4:]
    data, want = AR.upsampler_image(mode, trim, few)
    assert M.decode(data)[2].tobytes() == want.tobytes()
    if not turbo():
        pytest.skip("this Pillow is not built on libjpeg-turbo")
    data, want = AR.upsampler_image(mode, trim)
    assert want.shape == ((1 if mode == "422" else 2) * 8 * 6 * 260 - trim, 2 * 8 * 34 - trim, 3)
    assert pillow(data).tobytes() == want.tobytes()
