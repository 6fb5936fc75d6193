"""Geometry of conv3x3s2_wrw replayed through the functions the kernel compiles:
the fill of a stage and the tap table, over every chunk of small problems."""

import pytest

from torch_cgx_amd import _C

# (batch, H, W, C, N, max_workgroups): a 2x2 input; odd Wo != Ho; stacked 7x7
# outputs, the last group partly filled; three chunks, the last short; a cap
SHAPES = [
    (1, 2, 2, 64, 64, 0),
    (2, 4, 6, 64, 64, 0),
    (3, 14, 14, 64, 128, 0),
    (2, 14, 56, 64, 64, 0),
    (5, 24, 24, 128, 64, 2),
]


def _stage(shape, chunk, plan):
    """position -> (is_x, pixel or -1), every (position, vector) met once"""
    fill, taps = _C.conv3x3s2_wrw_fill(*shape, chunk)
    rows = fill.reshape(-1, 4).tolist()
    assert sorted((r[0], r[1]) for r in rows) == [
        (pos, v) for pos in range(plan["stage_pos"]) for v in range(8)]
    stage = {}
    for pos, _vec, is_x, pixel in rows:
        assert stage.setdefault(pos, (is_x, pixel)) == (is_x, pixel)
        assert is_x == (pos >= plan["strip_dy"])
    return stage, taps.tolist()


@pytest.mark.parametrize("shape", SHAPES)
def test_every_tap_meets_its_pixel(shape):
    batch, h, w, c, n, _cap = shape
    ho, wo = h // 2, w // 2
    plan = _C.conv3x3s2_wrw_plan(*shape)
    assert plan["eligible"]
    assert plan["lds_bytes"] <= plan["lds_budget"] == 160 * 1024
    assert plan["glds"] <= plan["max_glds"]
    assert plan["splits"] <= plan["chunks"]
    assert plan["grid"] == plan["splits"] * (c // 64) * (n // 64)
    seen_dy = []
    for chunk in range(plan["chunks"]):
        stage, taps = _stage(shape, chunk, plan)
        footprint, staged = set(), []
        for pos, (is_x, pixel) in stage.items():
            if is_x:
                assert -1 <= pixel < batch * h * w
                staged += [pixel] if pixel >= 0 else []
                continue
            assert -1 <= pixel < batch * ho * wo
            for tap, (_plane, shift) in enumerate(taps):
                # a zero of dY stays inside the stage, which this chunk wrote
                assert stage[pos + shift][0] == 1
                if pixel < 0:
                    continue
                b, oh, ow = pixel // (ho * wo), pixel // wo % ho, pixel % wo
                ih, iw = 2 * oh + tap // 3 - 1, 2 * ow + tap % 3 - 1
                inside = 0 <= ih < h and 0 <= iw < w
                want = (b * h + ih) * w + iw if inside else -1
                assert stage[pos + shift][1] == want, (chunk, pos, tap)
                footprint |= {want} if inside else set()
            seen_dy += [pixel] if pixel >= 0 else []
        assert sorted(staged) == sorted(footprint)  # each exactly once
    assert sorted(seen_dy) == list(range(batch * ho * wo))


def test_chunks_and_splits():
    multi = _C.conv3x3s2_wrw_plan(*SHAPES[3])
    assert multi["images"] == 1 and multi["chunks_per_image"] == 3
    assert multi["hr"] * 3 > 7  # the last chunk is short
    stacked = _C.conv3x3s2_wrw_plan(*SHAPES[2])
    assert stacked["images"] == 2 and stacked["chunks"] == 2
    assert stacked["stage_pos"] == 640  # two 7x7 outputs fill a stage
    assert _C.conv3x3s2_wrw_plan(*SHAPES[4])["grid"] == 2
    for shape in [(256, 56, 56, 128, 128), (256, 28, 28, 256, 256),
                  (256, 14, 14, 512, 512)]:
        plan = _C.conv3x3s2_wrw_plan(*shape)
        batch, h, w, c, n = shape
        assert plan["eligible"]
        assert plan["splits"] <= 8 or plan["splits"] % 8 == 0
        assert plan["grid"] <= 256
        # the partials stay within the bytes the workgroups read
        operands = 2 * batch * (h // 2) * (w // 2) * (n * c // 64
                                                      + 4 * c * n // 64)
        assert 4 * plan["partial_floats"] <= operands


@pytest.mark.parametrize("shape, ok", [
    ((2, 8, 8, 64, 512), True), ((2, 8, 174, 64, 64), True),
    ((2, 8, 176, 64, 64), False), ((2, 7, 8, 64, 64), False),
    ((2, 8, 6 + 1, 64, 64), False), ((2, 8, 8, 32, 64), False),
    ((2, 8, 8, 96, 64), False), ((2, 8, 8, 64, 1024), False),
    ((0, 8, 8, 64, 64), False),
])
def test_eligibility_edges(shape, ok):
    assert _C.conv3x3s2_wrw_plan(*shape)["eligible"] == ok
