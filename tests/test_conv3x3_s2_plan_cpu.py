"""conv3x3s2_fwd_plan (csrc/conv3x3_plan.cc): every tap reads the input pixel
of its definition through a parity plane or is cleared, the tiles cover every
output pixel once per channel tile; eligibility, LDS and the table."""

import pytest

from torch_cgx_amd import _C

# (batch, H, W, C, N, max_workgroups) of the input
GRID = [(2, 2, 2, 64, 64, 0), (2, 4, 6, 64, 64, 0), (3, 14, 14, 128, 64, 0),
        (2, 6, 56, 64, 64, 0), (5, 24, 24, 64, 64, 2), (1, 2, 62, 64, 64, 0),
        (2, 80, 2, 128, 64, 0), (64, 28, 28, 128, 64, 7),
        (256, 28, 28, 256, 256, 0)]


@pytest.mark.parametrize("shape", GRID, ids=lambda s: "x".join(map(str, s)))
def test_tiles_cover_every_pixel_once_and_taps_find_their_neighbours(shape):
    b, h, w, c, n, wg = shape
    ho, wo = h // 2, w // 2
    p = _C.conv3x3s2_fwd_plan(b, h, w, c, n, wg)
    assert p["eligible"] and p["rows"] == b * ho * wo
    assert (p["ho"], p["wo"]) == (ho, wo) and n == p["ntiles"] * p["bn"]
    assert wg == 0 or p["grid"] <= max(wg, p["ntiles"])
    assert p["tiles_per_split"] == -(-p["row_tiles"] // p["splits"])
    assert p["run"] == 16 * p["tiles_per_split"]
    t = p["tile_rows"]
    assert p["plane_rows"] == [t, t + 1, t + wo, t + wo + 1]
    assert p["strip_rows"] == sum(p["plane_rows"]) <= 64 * p["xvecs"]
    walk = _C.conv3x3s2_fwd_walk(b, h, w, c, n, wg)
    seen, writers = set(), set()
    for tiles in walk.tolist():
        for n0, split, row0, row1 in tiles:
            if n0 >= 0:
                writers.add((n0, split))
                assert seen.isdisjoint((n0, r) for r in range(row0, row1))
                seen.update((n0, r) for r in range(row0, row1))
    assert len(seen) == p["ntiles"] * p["rows"] and len(writers) == p["grid"]
    if p["rows"] <= 4096:  # the seam raises where a tap leaves its plane
        taps = _C.conv3x3s2_fwd_taps(b, h, w, c, n).tolist()
        for row, got in enumerate(taps):
            img, oh, ow = row // (ho * wo), row // wo % ho, row % wo
            want = [(img * h + 2 * oh + r - 1) * w + 2 * ow + s - 1
                    if 0 <= 2 * oh + r - 1 < h and 0 <= 2 * ow + s - 1 < w
                    else -1 for r in range(3) for s in range(3)]
            assert got == want, (row, got, want)


def test_what_is_eligible_and_what_is_native():
    good = [(4, 10, 10, c, n) for c in (64, 128, 256, 512)
            for n in (64, 128, 256, 512)]
    for ok in good + [(2, 4, w, 64, 64) for w in range(2, 64, 2)]:
        p = _C.conv3x3s2_fwd_plan(*ok)
        assert p["eligible"] and p["lds_bytes"] <= 160 * 1024, ok
    for bad in ((2, 4, 4, 32, 64), (2, 4, 4, 64, 96), (2, 4, 4, 1024, 64),
                (2, 4, 4, 64, 1024), (0, 4, 4, 64, 64), (2, 0, 4, 64, 64),
                (2, 4, 0, 64, 64), (2, 5, 4, 64, 64), (2, 4, 5, 64, 64),
                (1, 2, 2, 64, 64), (2, 4, 64, 64, 64), (2, 4096, 2, 64, 64),
                (1 << 13, 1 << 7, 1 << 5, 64, 64)):
        p = _C.conv3x3s2_fwd_plan(*bad)
        assert not p["eligible"] and not p["native"], bad
    # `native` at most for the three problems of ResNet-50 at batch 256
    for h, c in ((56, 128), (28, 256), (14, 512)):
        p = _C.conv3x3s2_fwd_plan(256, h, h, c, c)
        assert p["eligible"] and p["grid"] == 256, p
        for other in ((128, h, h, c, c), (256, h, h - 2, c, c),
                      (256, h, h, c, c // 2)):
            q = _C.conv3x3s2_fwd_plan(*other)
            assert q["eligible"] and not q["native"], other
