"""The sequential model of JPEG decode (tests/jpeg_decode_model.py) against the committed libjpeg-turbo pixels of every case,
against a live Pillow where that is built on libjpeg-turbo, and on the reference-made vectors under tests/golden/jpeg/
(baseline) and tests/golden/jpeg_p2/ (progressive: refused).  No GPU."""
import glob
import io
import os

import numpy as np
import pytest

import jpeg_decode_cases as JC
import jpeg_decode_model as M

GOLDEN = os.path.join(JC.HERE, "golden")
BASELINE = sorted(glob.glob(os.path.join(GOLDEN, "jpeg", "*.jpg")))
PROGRESSIVE = sorted(glob.glob(os.path.join(GOLDEN, "jpeg_p2", "*.jpg")))


def turbo():
    from PIL import features
    return features.check_feature("libjpeg_turbo")


def pillow(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)))


@pytest.mark.parametrize("c", JC.CASES, ids=JC.IDS)
def test_model_is_the_committed_expectation(c):
    w, h, px, ct = M.decode(JC.data(c))
    assert (w, h, ct) == (c["w"], c["h"], c["color_type"])
    assert JC.mismatch(px.tobytes(), c) == ""


def test_model_is_live_pillow_on_the_cases():
    if not turbo():
        pytest.skip("this Pillow is not built on libjpeg-turbo")
    for c in JC.CASES:
        assert pillow(JC.data(c)).tobytes() == JC.expected(c), c["name"]


def test_sixteen_bit_tables_read_as_their_eight_bit_twin():
    c = JC.by_name("420_50x37_q80_dqt16")
    d = JC.data(c)
    at = d.index(b"\xff\xdb")
    assert d[at + 4] >> 4 == 1, "the table has 16-bit entries"
    assert JC.mismatch(M.decode(JC.data(c))[2].tobytes(), c) == ""


def test_model_is_live_pillow_on_the_reference_made_baseline_files():
    if not turbo():
        pytest.skip("this Pillow is not built on libjpeg-turbo")
    assert len(BASELINE) >= 50
    for path in BASELINE:
        with open(path, "rb") as f:
            data = f.read()
        want = pillow(data)
        w, h, px, ct = M.decode(data)
        assert (h, w) == want.shape[:2] and px.tobytes() == want.tobytes(), os.path.basename(path)


def test_progressive_files_are_refused_with_the_references_message():
    assert len(PROGRESSIVE) >= 10
    for path in PROGRESSIVE:
        with open(path, "rb") as f:
            with pytest.raises(M.Refused) as e:
                M.decode(f.read())
        assert str(e.value) == "Unsupported: progressive JPEG not supported", os.path.basename(path)
