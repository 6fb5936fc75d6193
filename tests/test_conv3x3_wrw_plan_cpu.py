"""The launch geometry of the 3x3 weight gradient (csrc/conv3x3_plan.cc):
the chunks of all splits cover every image row once, the strips hold what the
taps reach, and LDS and the grid stay within their limits."""

import pytest

from torch_cgx_amd import _C

# (batch, H, W, C, N, max_workgroups)
GRID = [(1, 1, 1, 64, 64, 0), (2, 3, 5, 64, 64, 0), (3, 7, 7, 64, 128, 0),
        (5, 14, 14, 256, 256, 0), (2, 11, 56, 64, 64, 0),
        (2, 12, 12, 64, 64, 3), (9, 7, 7, 512, 512, 7), (2, 40, 3, 128, 64, 0),
        (1, 2, 166, 64, 64, 0), (256, 56, 56, 64, 64, 0),
        (256, 28, 28, 128, 128, 0), (256, 14, 14, 256, 256, 0),
        (256, 7, 7, 512, 512, 0)]


@pytest.mark.parametrize("shape", GRID, ids=lambda s: "x".join(map(str, s)))
def test_chunks_cover_every_row_once(shape):
    b, h, w, c, n, wg = shape
    p = _C.conv3x3_wrw_plan(b, h, w, c, n, wg)
    assert p["eligible"] and (p["bn"], p["bk"]) == (64, 64)
    assert p["grid"] == p["splits"] * p["ntiles_n"] * p["ntiles_k"]
    assert wg == 0 or p["grid"] <= max(wg, p["ntiles_n"] * p["ntiles_k"])
    assert 1 <= p["splits"] <= p["chunks"]
    assert p["chunks_per_split"] == -(-p["chunks"] // p["splits"])
    assert p["strip_dy"] == -(-p["hr"] * (w + 1) // 16) * 16
    assert p["strip_x"] >= p["strip_dy"] + 2 * (w + 1) + 2
    assert p["strip_x"] % 4 == 0
    assert p["lds_bytes"] == 2 * (p["strip_dy"] * 64 + p["strip_x"] * 64)
    assert p["lds_bytes"] <= p["lds_budget"] == 160 * 1024
    assert p["partial_floats"] == p["splits"] * n * 9 * c
    seen = {}
    for split in range(p["splits"]):
        for chunk in range(split, p["chunks"], p["splits"]):
            group, part = divmod(chunk, p["chunks_per_image"])
            for t in range(part * p["hr"], (part + 1) * p["hr"]):
                row = _C.conv3x3_wrw_row(b, h, w, c, n, wg, group, t)
                if row >= 0:
                    assert row not in seen, (row, seen[row], chunk)
                    seen[row] = chunk
    assert sorted(seen) == list(range(b * h))


def test_the_bottleneck_problems_and_the_limits():
    for h, c in ((56, 64), (28, 128), (14, 256), (7, 512)):
        p = _C.conv3x3_wrw_plan(256, h, h, c, c)
        assert p["eligible"] and p["grid"] >= 128, p
    assert _C.conv3x3_wrw_plan(256, 7, 7, 512, 512)["images"] > 1
    for bad in ((2, 4, 4, 32, 64), (2, 4, 4, 64, 96), (2, 4, 4, 1024, 64),
                (2, 4, 4, 64, 1024), (0, 4, 4, 64, 64), (2, 0, 4, 64, 64),
                (2, 4, 0, 64, 64), (2, 4, 167, 64, 64),
                (1 << 12, 1 << 7, 1 << 6, 64, 64)):
        assert not _C.conv3x3_wrw_plan(*bad)["eligible"], bad
