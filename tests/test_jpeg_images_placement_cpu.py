"""CPU-only: where the ragged coding pass of the JPEG images entry (scan_code_kernel<MODE, 2>, jpeg_scan_fused.hip) keeps the
block sums of its two-level look-back, from `jpeg.encode_images_plan` alone.

Segment k of a colour class's pass (first group f_k, g_k groups of 192 blocks) owns the words
    [(f_k >> 6) + k, (f_k >> 6) + k + ceil(g_k / 64))
of a table of (groups_total >> 6) + nsegs + 1 words (fused_code_state_words_ragged): its group 64 j + 63 writes word j, its
groups from 64 (j + 1) on read it.  The plan entry gives f_k; g_k is the next segment's f minus f_k; the formula is restated
here (words_of) and held against those.  Asserted per colour class: the ranges are ascending, pairwise disjoint and end inside
the table; and the copies a pass of 256 groups or more keeps (sup_layout, jpeg_scan_dev.h) do not reach into each other.

The tight case: first group 0 and 65 groups own words 0 and 1; the next segment begins at group 65, word (65 >> 6) + 1 = 2,
directly behind.  One group more in front (first group 1) leaves no room either: (66 >> 6) + 1 = 2 again."""
import numpy as np
import pytest

import jpeg_images_cases as K
from pixo_amd import ColorType, jpeg

GRAY, RGB = K.GRAY, K.RGB


def gray_of(g):
    """a gray image of exactly g groups: 1536 pixels are 192 blocks a row of blocks"""
    return (1536, 8 * g, ColorType.Gray, 0)


def rgb_of(g, ss):
    """an RGB image of exactly g groups: 64 units (4:4:4, 512 pixels) or 32 MCUs (4:2:0) a row"""
    return (512, (16 if ss == 1 else 8) * g, ColorType.Rgb, 0)


def words_of(first, groups):
    """per segment k of one pass: (begin, end) of its block sums — the kernel's `(floor_g >> 6) + sidx` and the
    (groups + 63) / 64 words it may write"""
    return [((f >> 6) + k, (f >> 6) + k + -(-g // 64)) for k, (f, g) in enumerate(zip(first, groups))]


def table_words(first, groups):
    return ((first[-1] + groups[-1]) >> 6) + len(first) + 1


def copies_and_stride(groups_total, sums):
    """sup_layout, restated"""
    if groups_total < 256:
        return 1, sums
    return 16, (512 + 32 if sums <= 512 else -(-sums // 32) * 32 + 32)


def check_pass(first, groups, where):
    assert first[0] == 0 and all(first[k + 1] == first[k] + groups[k] for k in range(len(first) - 1)), where
    w = words_of(first, groups)
    for k, (b, e) in enumerate(w):
        assert b < e, (where, k)
        if k:
            assert w[k - 1][1] <= b, (where, k, w[k - 1], w[k])  # ascending, and disjoint from every one before
    sums = table_words(first, groups)
    assert w[-1][1] <= sums, (where, w[-1], sums)
    copies, stride = copies_and_stride(first[-1] + groups[-1], sums)
    assert stride >= sums and copies & (copies - 1) == 0, where  # (a group picks its copy with g & (copies - 1))
    return w


def passes_of(records, o):
    """-> {colour: (first groups, groups)} from the plan entry"""
    groups = K.plan_groups(jpeg, records, o)
    first = jpeg.encode_images_plan(records, o)["first_group"]
    out = {}
    for ct in (GRAY, RGB):
        idx = [i for i, r in enumerate(records) if int(r[2]) == ct]
        if idx:
            out[ct] = ([first[i] for i in idx], [groups[i] for i in idx])
    return out


@pytest.mark.parametrize("ss", [1, 0], ids=["420", "444"])
def test_shapes_have_the_groups_they_claim(ss):
    o = K.template(jpeg, ss, 80)
    for cls in (K.klass(RGB, ss), "gray"):
        ct = GRAY if cls == "gray" else RGB
        claimed = sorted(K.SHAPES[cls])
        assert claimed == [1, 63, 64, 65, 128, 129]
        records = [(w, h, ColorType(ct), 0) for w, h in (K.SHAPES[cls][g] for g in claimed)]
        assert K.plan_groups(jpeg, records, o) == claimed, cls
        for g in claimed[1:]:  # the last group is full ...
            assert K.blocks(*K.SHAPES[cls][g], cls) == g * K.GROUP, (cls, g)
        # ... and one pixel more each way adds a column and a row of units (513 x 1009 at 4:2:0 is 66 full groups again; the
        # 64-group size, which the long list uses, ends in a partial group in every class)
        larger = [(w + 1, h + 1, ColorType(ct), 0) for w, h, _, _ in records]
        got = K.plan_groups(jpeg, larger, o)
        assert got == [K.groups(w, h, cls) for w, h, _, _ in larger] and all(a > b for a, b in zip(got[1:], claimed[1:])), cls
        w, h = K.SHAPES[cls][64]
        assert K.blocks(w + 1, h + 1, cls) % K.GROUP in {"444": (3,), "420": (6,), "gray": (33,)}[cls]
    shapes, claimed = K.long_list(ss)
    records = [(w, h, ColorType(ct), 0) for w, h, ct, _ in shapes]
    assert K.plan_groups(jpeg, records, o) == claimed
    for ct in (GRAY, RGB):
        per = [g for g, s in zip(claimed, shapes) if s[2] == ct]
        assert per[:6] == [1, 65, 64, 129, 1, 63] and sum(per) >= 256, per  # (256: the block sums in 16 copies)


def test_the_tight_case():
    o = K.template(jpeg, 0, 80)
    for lead, want in ((0, [(0, 2), (2, 3)]), (1, [(0, 1), (1, 3), (3, 4)])):
        records = ([gray_of(lead)] if lead else []) + [gray_of(65), gray_of(1)]
        first, groups = passes_of(records, o)[GRAY]
        assert groups == ([lead] if lead else []) + [65, 1]
        assert check_pass(first, groups, lead) == want
    # the long list with the 65-group images in front: either class begins with the tight case
    for ss in (1, 0):
        shapes, _ = K.long_list(ss)
        records = [(shapes[i][0], shapes[i][1], ColorType(shapes[i][2]), 0) for i in K.order(len(shapes), "tight")]
        for ct, (first, groups) in passes_of(records, K.template(jpeg, ss, 80)).items():
            w = check_pass(first, groups, (ss, ct))
            assert groups[0] == 65 and w[0] == (0, 2) and w[1][0] == 2


@pytest.mark.parametrize("segments", [2, 3])
def test_every_first_group_modulo_64_times_every_length(segments):
    """first group a (a segment of a groups in front; none for 0) x 1..200 groups, then one (a 65-group) or two (129 and 1)
    more segments behind: every range against every other, and the table's end"""
    o = K.template(jpeg, 0, 80)
    behind = [gray_of(65)] if segments == 2 else [gray_of(129), gray_of(1)]
    for a in range(64):
        for g in range(1, 201):
            records = ([gray_of(a)] if a else []) + [gray_of(g)] + behind
            first = jpeg.encode_images_plan(records, o)["first_group"]
            groups = ([a] if a else []) + [g] + [r[1] // 8 for r in behind]
            assert first == [sum(groups[:k]) for k in range(len(groups))], (a, g)
            check_pass(first, groups, (a, g))
    # (the groups of these shapes, once from the plan entry itself)
    assert K.plan_groups(jpeg, [gray_of(63), gray_of(200), gray_of(65)], o) == [63, 200, 65]


@pytest.mark.parametrize("ss", [1, 0], ids=["420", "444"])
def test_seeded_random_record_lists(ss):
    o = K.template(jpeg, ss, 80)
    rng = np.random.RandomState(20261021 + ss)
    edges = [1, 2, 62, 63, 64, 65, 66, 127, 128, 129, 130, 191, 192, 193, 255, 256, 257]
    for trial in range(300):
        records = []
        for _ in range(int(rng.randint(2, 24))):
            g = int(edges[rng.randint(len(edges))]) if rng.randint(3) else int(rng.randint(1, 400))
            if rng.randint(2):
                records.append(gray_of(g) if rng.randint(2) else (int(rng.randint(1, 3000)), int(rng.randint(1, 3000)), ColorType.Gray, 0))
            else:
                records.append(rgb_of(g, ss) if rng.randint(2) else (int(rng.randint(1, 2000)), int(rng.randint(1, 2000)), ColorType.Rgb, 0))
        for ct, (first, groups) in passes_of(records, o).items():
            cls = K.klass(ct, ss)
            assert groups == [K.groups(r[0], r[1], cls) for r in records if int(r[2]) == ct], trial
            check_pass(first, groups, (trial, ct))
