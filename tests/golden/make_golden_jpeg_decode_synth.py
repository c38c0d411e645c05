"""Writes tests/golden/jpeg_decode_synth/ and tests/golden/jpeg_decode_synth_cases.json: baseline JPEG files that no encoder
writes — three quantisation and three Huffman tables per file, odd component ids, tables in one segment or defined twice,
codes of 9 to 16 bits, blocks without an end of block, ZRL runs, the largest DC and AC magnitudes, restart intervals with fill
bytes and redefined DRI, odd file ends — written by tests/jpeg_write.py from quantised coefficients, each with the pixels
Pillow (libjpeg-turbo) decodes from it.  Every file is also decoded by tests/jpeg_decode_model.py, which must give Pillow's
pixels; where Pillow refuses a file the entry says what each side does ("pillow") and the committed pixels are the model's.
Every block lies inside the two conditions of pixo_amd/csrc/jpeg_decode_math.h's header.  Run by hand from the repository
root; reruns give identical bytes:
    python tests/golden/make_golden_jpeg_decode_synth.py"""
import hashlib
import io
import json
import os
import sys
import zlib

import numpy as np
from PIL import Image, ImageFile, features

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, ".."))
sys.path.insert(0, HERE)
import jpeg_decode_model as M  # noqa: E402
import jpeg_write as W  # noqa: E402
from make_golden_jpeg_decode import content  # noqa: E402

OUT = os.path.join(HERE, "jpeg_decode_synth")
DC, AC = W.DC, W.AC
FACTORS = {"gray": (1, 1), "444": (1, 1), "422": (2, 1), "420": (2, 2)}
_k = np.arange(8)
DCT = np.where(_k[:, None] == 0, np.sqrt(1 / 8), np.sqrt(2 / 8) * np.cos((2 * _k[None, :] + 1) * _k[:, None] * np.pi / 16))
# The weights of the header's bound (a)
A = np.array([8192, 32501, 10703, 71869, 8192, 50643, 19570, 35521]) / 8192.0


def qtab(scale, tilt=1.0):
    """A quantisation table, natural order: 1 + scale * (row * tilt + column), at most 255"""
    r, c = np.mgrid[0:8, 0:8]
    return np.clip(np.round(1 + scale * (r * tilt + c)), 1, 255).astype(np.int64).reshape(64)


def comps_of(mode):
    return W.gray() if mode == "gray" else W.colour(mode)


def quantise(mode, w, h, seed, comps, q, noise=12.0):
    """content() -> YCbCr (JFIF) -> chroma averaged down -> float DCT -> quantised coefficients per component, natural order"""
    px = content(w, h, seed, noise).astype(np.float64)
    r, g, b = px[..., 0], px[..., 1], px[..., 2]
    planes = [0.299 * r + 0.587 * g + 0.114 * b, 128 - 0.168736 * r - 0.331264 * g + 0.5 * b, 128 + 0.5 * r - 0.418688 * g - 0.081312 * b]
    hm, vm = FACTORS[mode]
    H, Wd = -(-h // (8 * vm)) * 8 * vm, -(-w // (8 * hm)) * 8 * hm
    out = []
    for ci, c in enumerate(comps):
        p = np.pad(planes[ci], ((0, H - h), (0, Wd - w)), mode="edge")
        if ci and mode != "gray":
            p = p.reshape(H // vm, vm, Wd // hm, hm).mean((1, 3))
        blocks = (p - 128).reshape(p.shape[0] // 8, 8, p.shape[1] // 8, 8).transpose(0, 2, 1, 3)
        f = DCT @ blocks @ DCT.T
        out.append(np.round(f.reshape(f.shape[:2] + (64,)) / np.asarray(q[c["tq"]])).astype(np.int64))
    return out


def inside_conditions(comps, q, coefs):
    """(a) W(d) <= 65000 and (b) every descaled sample in -512..511, for every block"""
    for c, z in zip(comps, coefs):
        d = (np.asarray(z) * np.asarray(q[c["tq"]])).reshape(z.shape[:2] + (8, 8))
        if (np.abs(d) * A[:, None] * A[None, :]).sum((-1, -2)).max() > 65000:
            return False
        s = M.unclamped(d)
        if s.min() < -512 or s.max() > 511:
            return False
    return True


def pillow(data, truncated=False):
    ImageFile.LOAD_TRUNCATED_IMAGES = truncated
    try:
        return np.asarray(Image.open(io.BytesIO(data)))
    finally:
        ImageFile.LOAD_TRUNCATED_IMAGES = False


def seeded_blocks(shape, seed, fill):
    """Coefficient planes from a seed; `fill(rng, z)` shapes block z (64 values, ZIGZAG order) in place"""
    rng = np.random.default_rng(seed)
    out = np.zeros(shape + (64,), np.int64)
    for y in range(shape[0]):
        for x in range(shape[1]):
            z = np.zeros(64, np.int64)
            fill(rng, z)
            out[y, x, W.ZIGZAG] = z
    return out


def main(OUT=OUT, listing=os.path.join(HERE, "jpeg_decode_synth_cases.json")):
    """(A test reruns this into a directory of its own and compares the bytes)"""
    assert features.check_feature("libjpeg_turbo"), "the goldens are libjpeg-turbo's pixels"
    os.makedirs(OUT, exist_ok=True)
    for n in os.listdir(OUT):
        os.remove(os.path.join(OUT, n))
    cases, seed = [], [500]

    def add(name, mode, w, h, comps, q, coefs, pillow_refuses=None, patch=None, **kw):
        """Write, decode with Pillow and the model, compare, commit"""
        assert inside_conditions(comps, q, coefs), name
        info = {}
        data = W.write(w, h, comps, q, coefs, info=info, **kw)
        if patch:
            data = patch(data)
        got = M.coefficients(data)[1]
        assert all(np.array_equal(np.asarray(a)[..., W.ZIGZAG], b) for a, b in zip(coefs, got)), name
        model = M.decode(data)[2]
        extra = {}
        if pillow_refuses is None:
            px = pillow(data)
            assert px.dtype == np.uint8 and px.shape == model.shape and px.tobytes() == model.tobytes(), name + ": the model is not Pillow"
        else:
            try:
                pillow(data)
                raise AssertionError(name + ": Pillow decodes it after all")
            except OSError as e:
                assert pillow_refuses in str(e), (name, str(e))
                extra = dict(pillow="refuses: " + str(e), source="model")
            px = model
        with open(os.path.join(OUT, name + ".jpg"), "wb") as f:
            f.write(data)
        with open(os.path.join(OUT, name + ".px.z"), "wb") as f:
            f.write(zlib.compress(px.tobytes(), 9))
        cases.append(dict(name=name, mode=mode, w=w, h=h, color_type=0 if mode == "gray" else 2, sha256=hashlib.sha256(px.tobytes()).hexdigest(), **extra))
        return data, info

    def natural(mode, w, h, comps, q, noise=12.0):
        seed[0] += 1
        return quantise(mode, w, h, seed[0], comps, q, noise)

    Q2 = {0: qtab(1.5), 1: qtab(3.0)}
    COLOUR = ("444", "422", "420")

    # ---- three quantisation tables: chroma 1 : 3 ----
    for ids, size in (((0, 1, 2), (50, 37)), ((3, 0, 2), (17, 17))):
        for mode in COLOUR:
            comps = W.colour(mode, tq=ids)
            q = {ids[0]: qtab(1.5), ids[1]: qtab(2.0, 0.5), ids[2]: 3 * qtab(2.0, 0.5)}
            add("q3_%d%d%d_%s_%dx%d" % (ids + (mode,) + size), mode, *size, comps, q, natural(mode, *size, comps, q))

    # ---- three DC and three AC Huffman tables, each from its own component's statistics ----
    for (td, ta), size in ((((0, 1, 2), (0, 1, 2)), (50, 37)), (((3, 0, 2), (2, 3, 0)), (17, 17))):
        for mode in COLOUR:
            comps = W.colour(mode, td=td, ta=ta)
            q = {0: qtab(1.0), 1: qtab(1.5, 2.0)}
            _, info = add("huff3_%d%d%d_%d%d%d_%s_%dx%d" % (td + ta + (mode,) + size), mode, *size, comps, q, natural(mode, *size, comps, q, noise=25.0))
            for cls, ids in ((DC, td), (AC, ta)):
                tables = [info["huff"][(cls, i)] for i in ids]
                assert tables[0] != tables[1] != tables[2] != tables[0], "the three tables must differ"
                if cls == AC:  # ... and each must lack a symbol that another component uses: the wrong table cannot decode
                    assert set(info["symbols"][(AC, ids[2])]) - set(tables[1][1]) or set(info["symbols"][(AC, ids[1])]) - set(tables[2][1])

    # ---- component ids ----
    for ids in ((0, 1, 2), (10, 200, 3), (ord("Y"), ord("C"), ord("c"))):
        comps = W.colour("420", ids=ids)
        add("ids_%d_%d_%d_420_50x37" % ids, "420", 50, 37, comps, Q2, natural("420", 50, 37, comps, Q2))
    comps = W.gray(id=0)
    add("ids_0_gray_17x17", "gray", 17, 17, comps, Q2, natural("gray", 17, 17, comps, Q2))
    # a lone component's sampling factors mean nothing (T.81 A.2.2); 2x2, 1x1, 1x1 is what every 4:2:0 file here is written as
    comps = W.gray()

    def written_2x2(data):  # (patched in: the writer lays blocks out by the factors, and a lone component has none)
        at = data.index(b"\xff\xc0") + 11
        assert data[at] == 0x11
        return data[:at] + b"\x22" + data[at + 1:]
    add("gray_written_2x2_50x37", "gray", 50, 37, comps, Q2, natural("gray", 50, 37, comps, Q2), patch=written_2x2)

    # ---- segments: all tables in one DQT and one DHT; a table defined twice; 8- and 16-bit tables in one DQT ----
    for mode in FACTORS:
        comps = comps_of(mode)
        ncol = mode != "gray"
        keys = [(DC, 0), (AC, 0)] + ([(DC, 1), (AC, 1)] if ncol else [])
        layout = [("DQT", [0, 1] if ncol else [0]), ("SOF",), ("DHT", keys), ("SOS",)]
        add("one_dqt_one_dht_%s_50x37" % mode, mode, 50, 37, comps, Q2, natural(mode, 50, 37, comps, Q2), layout=layout)
    comps = W.colour("420")
    layout = [("DQT", [(0, qtab(4.0), False), (1, qtab(0.5), False)]), ("DQT", [1]), ("SOF",), ("DQT", [0]),
              ("DHT", [(DC, 0)]), ("DHT", [(AC, 0)]), ("DHT", [(DC, 1)]), ("DHT", [(AC, 1)]), ("SOS",)]
    add("dqt_twice_420_50x37", "420", 50, 37, comps, Q2, natural("420", 50, 37, comps, Q2), layout=layout)
    decoy_dc = W.table_from_lengths({s: 4 for s in range(12)})
    decoy_ac = W.table_from_lengths({s: 8 for s in range(0, 256, 2)})
    layout = [("DQT", [0]), ("DQT", [1]), ("SOF",), ("DHT", [(DC, 0, decoy_dc), (AC, 1, decoy_ac), (AC, 0, decoy_ac), (DC, 1, decoy_dc)]),
              ("DHT", [(DC, 0), (AC, 0)]), ("DHT", [(DC, 1)]), ("DHT", [(AC, 1)]), ("SOS",)]
    add("dht_twice_420_50x37", "420", 50, 37, comps, Q2, natural("420", 50, 37, comps, Q2), layout=layout)
    for mode in ("444", "420"):
        comps = W.colour(mode, tq=(0, 1, 2))
        wide = qtab(2.0)
        wide[40:] = 300  # entries that need 16 bits, where the content leaves next to nothing
        q = {0: qtab(1.5), 1: wide, 2: qtab(2.5)}
        add("dqt_8_16_8_bit_%s_50x37" % mode, mode, 50, 37, comps, q, natural(mode, 50, 37, comps, q), layout=[("DQT", [0, 1, 2]), ("SOF",)]
            + [("DHT", [k]) for k in ((DC, 0), (AC, 0), (DC, 1), (AC, 1))] + [("SOS",)], q16=(1,))

    # ---- Huffman tables that force long codes ----
    Q1 = {0: qtab(1.0), 1: qtab(1.5)}
    for mode in ("gray", "420"):
        comps = comps_of(mode)
        tables = [(DC, 0), (AC, 0)] + ([(DC, 1), (AC, 1)] if mode != "gray" else [])
        _, info = add("codes_9_to_16_bits_%s_50x37" % mode, mode, 50, 37, comps, Q1, natural(mode, 50, 37, comps, Q1, noise=25.0),
                      huff={k: W.long_codes_table for k in tables})
        assert all(sum(info["huff"][k][0][:8]) == 0 and info["huff"][k][0][15] > 0 for k in tables if k[0] == AC)
        _, info = add("code_of_16_bits_%s_50x37" % mode, mode, 50, 37, comps, Q1, natural(mode, 50, 37, comps, Q1, noise=25.0),
                      huff={k: W.sixteen_bit_table for k in tables})
        assert all(info["huff"][k][0][15] == 2 for k in tables)
        # libjpeg refuses a table whose code words fill the code space (jdhuff.c: the all-ones word must stay free)
        add("last_code_all_ones_%s_50x37" % mode, mode, 50, 37, comps, Q1, natural(mode, 50, 37, comps, Q1, noise=25.0),
            huff={k: (lambda f: W.optimal_table(f, reserve=False)) for k in tables}, pillow_refuses="broken data stream")
    for mode in ("gray", "444"):
        comps = comps_of(mode)
        flat = [np.zeros((-(-37 // 8), -(-50 // 8), 64), np.int64) for _ in comps]
        _, info = add("single_symbol_tables_flat_%s_50x37" % mode, mode, 50, 37, comps, Q1, flat)
        assert all(t == ([1] + [0] * 15, [0]) for t in info["huff"].values())
    # a lone DC symbol that is not zero: every block steps up by the same difference
    comps = W.gray()
    ramp = np.zeros((3, 3, 64), np.int64)
    ramp[..., 0] = 100 * (1 + np.arange(9).reshape(3, 3))  # every difference, the first too, is 100: category 7
    q1 = {0: np.ones(64, np.int64)}
    _, info = add("single_symbol_dc_steps_gray_17x17", "gray", 17, 17, comps, q1, [ramp])
    assert info["huff"][(DC, 0)] == ([1] + [0] * 15, [7])

    # ---- blocks ----
    def no_eob(rng, z):
        z[0] = rng.integers(-40, 41)
        z[1:] = rng.choice([-2, -1, 1, 2], 63)

    def zrl3_k63(rng, z):
        z[0] = rng.integers(-200, 201)
        if rng.integers(0, 2):
            z[rng.integers(1, 15)] = rng.integers(1, 6)
        z[63] = rng.choice([-3, -1, 1, 2])  # at least 48 zeros in front of it

    def zrl2_tail(rng, z):
        z[0] = rng.integers(-200, 201)
        k0 = 33 + rng.integers(0, 12)  # 32 zeros and up to 11 more, then no zero to the block's end
        z[k0:] = rng.choice([-1, 1], 64 - k0)

    def ac_size10(rng, z):
        z[0] = rng.integers(-100, 101)
        z[rng.integers(1, 4)] = rng.choice([-1023, -512, 512, 1023, 700])
        z[rng.integers(4, 20)] = rng.integers(-20, 21)

    q1c = {0: np.ones(64, np.int64), 1: np.ones(64, np.int64)}
    for name, fill in (("no_eob_63_acs", no_eob), ("three_zrl_then_k63", zrl3_k63), ("two_zrl_then_tail_without_eob", zrl2_tail), ("ac_size_10", ac_size10)):
        for mode, (w, h) in (("gray", (17, 17)), ("420", (50, 37))):
            comps = comps_of(mode)
            seed[0] += 1
            coefs = [seeded_blocks((-(-h // (8 * FACTORS[mode][1])) * c["v"], -(-w // (8 * FACTORS[mode][0])) * c["h"]), seed[0] + 7 * i, fill) for i, c in enumerate(comps)]
            _, info = add("%s_%s_%dx%d" % (name, mode, w, h), mode, w, h, comps, q1c, coefs)
            syms = info["symbols"][(AC, 0)]
            if fill is no_eob:
                assert W.EOB not in syms and W.ZRL not in syms
            elif fill is zrl3_k63:
                assert W.EOB not in syms and syms[W.ZRL] >= 3
            elif fill is zrl2_tail:
                assert W.EOB not in syms and syms[W.ZRL] >= 2
            else:
                assert any(s & 15 == 10 for s in syms)
    for mode, (w, h) in (("gray", (17, 17)), ("420", (50, 37))):  # a pixel step from -1024 to +1016 at q = 1: flat 0 beside flat 255
        comps = comps_of(mode)
        coefs = []
        for c in comps:
            z = np.zeros((-(-h // (8 * FACTORS[mode][1])) * c["v"], -(-w // (8 * FACTORS[mode][0])) * c["h"], 64), np.int64)
            yy, xx = np.mgrid[0:z.shape[0], 0:z.shape[1]]
            z[..., 0] = np.where((yy + xx) % 2 == 0, -1024, 1016)
            coefs.append(z)
        _, info = add("dc_category_11_%s_%dx%d" % (mode, w, h), mode, w, h, comps, q1c, coefs)
        assert 11 in info["symbols"][(DC, 0)]

    # ---- restarts ----
    every_second = lambda i: (0, 1, 0, 3)[i % 4]  # one and three fill bytes, in front of every second RSTn
    for mode in ("gray", "420"):
        comps = comps_of(mode)
        data, _ = add("rst1_fill_bytes_%s_50x37" % mode, mode, 50, 37, comps, Q2, natural(mode, 50, 37, comps, Q2), restart=1, rst_fill=every_second)
        assert b"\xff\xff\xd1" in data and b"\xff\xff\xff\xff\xd3" in data
    comps, mcus = W.colour("420"), 4 * 3
    head = [("DQT", [0]), ("DQT", [1]), ("SOF",)] + [("DHT", [k]) for k in ((DC, 0), (AC, 0), (DC, 1), (AC, 1))]
    for name, dri in (("rst_interval_is_mcu_count", [mcus]), ("rst_interval_above_mcu_count", [mcus + 5]), ("dri_4_then_dri_0", [4, 0]), ("dri_0_then_dri_3", [0, 3])):
        layout = head[:2] + [("DRI", dri[0])] + head[2:] + [("DRI", d) for d in dri[1:]] + [("SOS",)]
        data, info = add("%s_420_50x37" % name, "420", 50, 37, comps, Q2, natural("420", 50, 37, comps, Q2), layout=layout)
        assert (b"\xff\xd0" in info["scan"]) == (dri[-1] == 3)

    # ---- file ends ----
    comps = W.gray()
    seed[0] += 1
    coefs = quantise("gray", 50, 37, seed[0], comps, Q2)
    coefs[0][-1, -1, 63] = 7  # the scan ends on three one bits, no end of block behind them
    for last in range(-60, 61):  # the last block's DC shifts them along, until the scan's last byte is 0xFF (then stuffed)
        coefs[0][-1, -1, 0] = last
        info = {}
        W.write(50, 37, comps, Q2, coefs, info=info)
        if info["scan"][-2:] == b"\xff\x00":
            break
    else:
        raise AssertionError("no file ends on 0xFF")
    data, _ = add("last_scan_byte_is_stuffed_ff_gray_50x37", "gray", 50, 37, comps, Q2, coefs)
    assert data[-4:] == b"\xff\x00\xff\xd9"
    comps = W.colour("420")
    trailer = bytes(np.random.default_rng(9).integers(0, 256, 100, dtype=np.uint8))
    add("trailer_100_bytes_420_50x37", "420", 50, 37, comps, Q2, natural("420", 50, 37, comps, Q2), trailer=trailer, fill={"EOI": 2})
    # Pillow wants the bytes behind the scan before it hands the last rows out; libjpeg itself, fed what is there, decodes all
    data, _ = add("no_eoi_420_50x37", "420", 50, 37, comps, Q2, natural("420", 50, 37, comps, Q2), eoi=False, pillow_refuses="image file is truncated")
    assert pillow(data, truncated=True).tobytes() == M.decode(data)[2].tobytes(), "libjpeg, fed the truncated file, is the model"
    cases[-1]["pillow"] += "; with ImageFile.LOAD_TRUNCATED_IMAGES libjpeg gives the committed pixels"

    with open(listing, "w") as f:
        json.dump(dict(cases=cases), f, indent=1)
    sizes = [os.path.getsize(os.path.join(OUT, n)) for n in os.listdir(OUT)]
    print("%d cases, %d bytes under %s, largest %d" % (len(cases), sum(sizes), OUT, max(sizes)))


if __name__ == "__main__":
    main()
