"""The launch geometry of the stem convolution (csrc/conv_stem_plan.cc): the
bands and tiles of all workgroups cover every output pixel once, every
position of the padded filter meets its input element through the strip or is
cleared, and LDS, the width and the table keep their limits."""

import pytest
import torch

from torch_cgx_amd import _C

# (batch, H, W, max_workgroups): small shapes, the widest, the benchmark's
GRID = [(2, 2, 8, 0), (1, 8, 8, 0), (2, 16, 24, 0), (2, 6, 224, 0),
        (3, 40, 16, 0), (5, 16, 16, 2), (1, 4, 768, 0), (256, 224, 224, 0)]
NATIVE = ((256, 224, 224),)  # what benchmarks/conv_stem_shapes.py has admitted


def _want_taps(b, h, w, row0, row1):
    # [rows, 176]: element of x under position 24r + 3s + c, -1 off it or a pad
    oh, ow = h // 2, w // 2
    row = torch.arange(row0, row1).view(-1, 1)
    k = torch.arange(176).view(1, -1)
    r, t = k // 24, k % 24
    ih = 2 * (row // ow % oh) - 3 + r
    iw = 2 * (row % ow) - 3 + t // 3
    real = (r < 7) & (t < 21) & (ih >= 0) & (ih < h) & (iw >= 0) & (iw < w)
    elem = ((row // (oh * ow) * h + ih) * w + iw) * 3 + t % 3
    return torch.where(real, elem, torch.full_like(elem, -1))


@pytest.mark.parametrize("shape", GRID, ids=lambda s: "x".join(map(str, s)))
def test_bands_cover_every_pixel_once_and_taps_find_their_elements(shape):
    b, h, w, wg = shape
    p = _C.conv_stem_plan(b, h, w, wg)
    rows = b * (h // 2) * (w // 2)
    assert p["eligible"] and p["rows"] == rows
    assert p["grid"] == p["splits"] <= p["bands"] and (wg == 0
                                                       or p["grid"] <= wg)
    assert p["bands_per_split"] == -(-p["bands"] // p["splits"])
    assert p["in_rows"] == 2 * p["band_rows"] + 5 and p["pitch"] == 6 * w + 48
    assert p["in_rows"] * p["pitch"] <= 16 * p["xvecs"] * p["threads"]
    assert p["lds_bytes"] <= p["lds_budget"] == 160 * 1024 and p["xvecs"] <= 8
    assert p["run"] == 16 * -(-p["tiles_per_band"] // 4) * p["bands_per_split"]
    assert p["pstride"] == 129 and p["partial_floats"] == 129 * p["splits"]
    walk = _C.conv_stem_walk(b, h, w, wg)
    assert tuple(walk.shape) == (p["grid"], p["bands_per_split"], 3)
    seen = torch.zeros(rows, dtype=torch.int32)
    for bands in walk.tolist():
        assert bands[0][0] >= 0                # one partial row each
        for row0, row1, tiles in bands:
            if row0 < 0:
                continue
            assert 0 < row1 - row0 <= tiles * p["tile"] < row1 - row0 + 32
            seen[row0:row1] += 1
    assert bool((seen == 1).all())
    # the taps of up to 2048 pixels at the start and at the end
    for row0, row1 in {(0, min(rows, 2048)), (max(rows - 2048, 0), rows)}:
        got = _C.conv_stem_taps(b, h, w, row0, row1)
        assert torch.equal(got, _want_taps(b, h, w, row0, row1))


def test_what_is_eligible_and_what_is_native():
    assert _C.conv_stem_plan(1, 2, 8)["max_w"] == 768
    for bad in ((2, 7, 8), (2, 0, 8), (2, 8, 12), (2, 8, 4), (2, 8, 0),
                (2, 8, 776), (0, 8, 8), (1, 2, 2), (1 << 14, 128, 128),
                (1 << 40, 8, 8)):
        p = _C.conv_stem_plan(*bad)
        assert not p["eligible"] and not p["native"], bad
    assert _C.conv_stem_plan(1, 2, 8)["rows"] == 4      # the smallest problem
    assert _C.conv_stem_plan(1 << 12, 128, 128)["rows"] == 1 << 24
    for shape in ((256, 224, 224), (128, 224, 224), (256, 224, 216),
                  (2, 32, 32)):
        p = _C.conv_stem_plan(*shape)
        assert p["eligible"] and p["native"] == (shape in NATIVE), shape
