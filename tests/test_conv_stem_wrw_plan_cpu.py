"""The launch geometry of the stem's weight gradient (csrc/conv_stem_plan.cc):
host arithmetic only."""

import pytest

from torch_cgx_amd import _C

SHAPES = [(1, 2, 16, 0), (3, 62, 32, 0), (5, 16, 16, 2), (40, 4, 16, 0),
          (2, 6, 224, 0), (256, 224, 224, 0), (256, 224, 224, 100),
          (2, 32, 752, 0), (7, 230, 400, 3)]


def test_eligibility_bounds():
    plan = _C.conv_stem_wrw_plan
    max_w = plan(1, 2, 16)["max_w"]
    assert max_w % 16 == 0
    for good in [(1, 2, 16), (1, 2, max_w), (256, 224, 224), (1, 4096, 16)]:
        assert plan(*good)["eligible"], good
    for bad in [(0, 2, 16), (1, 0, 16), (1, 3, 16), (1, 2, 8), (1, 2, 24),
                (1, 2, max_w + 16), (2 ** 20, 224, 224), (1, 2, 16, -1)]:
        assert not plan(*bad)["eligible"], bad


@pytest.mark.parametrize("shape", SHAPES)
def test_plan_fits_and_walks_every_band_once(shape):
    p = _C.conv_stem_wrw_plan(*shape)
    assert p["eligible"] and p["band_rows"] >= 1
    assert 2 * p["buf_bytes"] <= p["lds_bytes"] <= p["lds_budget"]
    assert p["dyvecs"] * p["threads"] >= p["groups"] * 64
    assert p["steps"] == (p["groups"] + 1) // 2
    assert 0 < p["last_groups"] <= p["groups"]
    assert p["bands"] == shape[0] * p["bands_per_image"]
    assert p["grid"] == p["splits"] <= (shape[3] or 256)
    walk = _C.conv_stem_wrw_walk(*shape).tolist()
    assert len(walk) == p["splits"] and walk[0][0] == 0
    assert all(a < b <= a + p["bands_per_split"] for a, b in walk)
    assert all(walk[i][1] == walk[i + 1][0] for i in range(len(walk) - 1))
    assert walk[-1][1] == p["bands"]


def test_the_flagship_problem():
    p = _C.conv_stem_wrw_plan(256, 224, 224)
    assert p["band_rows"] == 4 and p["bands"] == 256 * 28
    assert p["splits"] == 256 and p["bands_per_split"] == 28


def test_native_only_for_the_table():
    # the one measured problem (benchmarks/RESULTS.md) and its neighbours
    for s in SHAPES + [(128, 224, 224, 0), (256, 224, 240, 0)]:
        assert _C.conv_stem_wrw_plan(*s)["native"] == (s[:3] == (256, 224, 224))
