"""The launch geometry of the 3x3 forward with statistics
(conv3x3_fwd_plan in csrc/conv3x3_plan.cc): the tiles of all workgroups cover
every pixel once per channel tile, every tap reads its neighbour through the
strip or is cleared, and LDS, the grid and the partials keep their limits."""

import pytest

from torch_cgx_amd import _C

# (batch, H, W, C, N, max_workgroups)
GRID = [(2, 1, 1, 64, 64, 0), (2, 3, 5, 64, 64, 0), (3, 7, 7, 128, 64, 0),
        (2, 3, 56, 64, 64, 0), (5, 12, 12, 64, 64, 2), (9, 7, 7, 512, 512, 7),
        (2, 40, 3, 128, 64, 0), (1, 2, 159, 64, 64, 0),
        (64, 14, 14, 128, 64, 7), (256, 14, 14, 256, 256, 0)]


@pytest.mark.parametrize("shape", GRID, ids=lambda s: "x".join(map(str, s)))
def test_tiles_cover_every_pixel_once_and_taps_find_their_neighbours(shape):
    b, h, w, c, n, wg = shape
    p = _C.conv3x3_fwd_plan(b, h, w, c, n, wg)
    assert p["eligible"] and p["rows"] == b * h * w
    assert p["grid"] == p["splits"] * p["ntiles"] and n == p["ntiles"] * p["bn"]
    assert wg == 0 or p["grid"] <= max(wg, p["ntiles"])
    assert 1 <= p["splits"] <= p["row_tiles"]
    assert p["tiles_per_split"] == -(-p["row_tiles"] // p["splits"])
    assert p["run"] == 32 * p["tiles_per_split"]
    assert p["strip_rows"] == p["tile_rows"] + 2 * w + 2 <= 64 * p["xvecs"]
    assert p["resident"] == (c == 64) and p["nchunks"] * p["kc"] == c
    assert p["lds_bytes"] <= p["lds_budget"] == 160 * 1024
    assert p["pstride"] == 2 * n + p["ntiles"] and n % (8 * p["ntiles"]) == 0
    assert p["partial_floats"] == p["splits"] * p["pstride"]
    walk = _C.conv3x3_fwd_walk(b, h, w, c, n, wg)
    assert tuple(walk.shape) == (p["grid"], p["tiles_per_split"], 4)
    seen, writers = {}, set()
    for wgi, tiles in enumerate(walk.tolist()):
        for n0, split, row0, row1 in tiles:
            if n0 < 0:
                continue
            writers.add((n0, split))
            for row in range(row0, row1):
                assert (n0, row) not in seen
                seen[n0, row] = wgi
    assert len(seen) == p["ntiles"] * p["rows"]
    assert len(writers) == p["grid"]           # one partial row each
    if b * h * w <= 4096:
        taps = _C.conv3x3_fwd_taps(b, h, w, c, n).tolist()
        for row, got in enumerate(taps):
            img, y, x = row // (h * w), row // w % h, row % w
            want = [(img * h + y + r - 1) * w + x + s - 1
                    if 0 <= y + r - 1 < h and 0 <= x + s - 1 < w else -1
                    for r in range(3) for s in range(3)]
            assert got == want, (row, got, want)


def test_what_is_eligible_and_what_is_native():
    for c in (64, 128, 256, 512):
        for n in (64, 128, 256, 512):
            p = _C.conv3x3_fwd_plan(4, 9, 9, c, n)
            assert p["eligible"] and n % (8 * p["ntiles"]) == 0
            assert p["lds_bytes"] <= 160 * 1024
    for bad in ((2, 4, 4, 32, 64), (2, 4, 4, 64, 96), (2, 4, 4, 1024, 64),
                (2, 4, 4, 64, 1024), (0, 4, 4, 64, 64), (2, 0, 4, 64, 64),
                (2, 4, 0, 64, 64), (1, 1, 1, 64, 64), (2, 4, 160, 64, 64),
                (1 << 12, 1 << 7, 1 << 6, 64, 64)):
        p = _C.conv3x3_fwd_plan(*bad)
        assert not p["eligible"] and not p["native"], bad
    # `native` only for the entries of the measured table: the four
    # bottleneck problems of ResNet-50 at batch 256, and nothing beside them
    for h, c in ((56, 64), (28, 128), (14, 256), (7, 512)):
        p = _C.conv3x3_fwd_plan(256, h, h, c, c)
        assert p["eligible"] and p["grid"] == 256 and p["native"], p
        for other in ((128, h, h, c, c), (256, h, h - 1, c, c),
                      (256, h, h, c, 2 * c if c < 512 else 64)):
            q = _C.conv3x3_fwd_plan(*other)
            assert q["eligible"] and not q["native"], other
