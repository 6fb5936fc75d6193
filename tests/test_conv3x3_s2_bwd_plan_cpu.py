"""conv3x3s2_bwd_plan: dX rebuilt in fp64 from the plan's host functions alone
(strip map, validity bits, term table, output pixel) is the input gradient, each
pixel written once, each dY row walked once; eligibility and the table."""

import pytest
import torch
import torch.nn.functional as F

from torch_cgx_amd import _C

# the GPU test's shapes (batch, C, N, Ho, Wo, max_workgroups) ...
GPU = [(2, 64, 64, 1, 1, 0), (2, 64, 64, 2, 3, 0), (3, 64, 128, 7, 7, 0),
       (2, 128, 64, 7, 7, 0), (2, 64, 64, 3, 28, 0), (2, 256, 256, 5, 5, 0),
       (2, 512, 512, 3, 3, 0), (5, 64, 64, 12, 12, 2), (32, 128, 64, 14, 14, 7)]
# ... as (batch, H, W of dX, C, N, max_workgroups), the widest and a tall one
GRID = [(b, 2 * ho, 2 * wo, c, n, wg) for b, c, n, ho, wo, wg in GPU] + [
    (1, 2, 126, 64, 64, 0), (2, 80, 2, 128, 64, 0)]


@pytest.mark.parametrize("shape", GRID, ids=lambda s: "x".join(map(str, s)))
def test_the_host_functions_rebuild_the_input_gradient(shape):
    b, h, w, c, n, wg = shape
    ho, wo = h // 2, w // 2
    p = _C.conv3x3s2_bwd_plan(b, h, w, c, n, wg)
    assert p["eligible"] and p["rows"] == b * ho * wo
    assert (p["ho"], p["wo"]) == (ho, wo) and c == p["ntiles"] * p["bn"]
    assert n == p["nchunks"] * p["kc"] and p["pstride"] == 0
    assert wg == 0 or p["grid"] <= max(wg, p["ntiles"])
    assert p["tiles_per_split"] == -(-p["row_tiles"] // p["splits"])
    assert p["strip_rows"] == p["tile_rows"] + wo + 1 <= 64 * p["xvecs"]
    assert p["lds_bytes"] <= p["lds_budget"]
    seen, writers = set(), set()
    for tiles in _C.conv3x3s2_bwd_walk(b, h, w, c, n, wg).tolist():
        for c0, split, row0, row1 in tiles:
            if c0 >= 0:
                writers.add((c0, split))
                assert seen.isdisjoint((c0, r) for r in range(row0, row1))
                seen.update((c0, r) for r in range(row0, row1))
    assert len(seen) == p["ntiles"] * p["rows"] and len(writers) == p["grid"]
    if p["rows"] > 4096:
        return
    terms = _C.conv3x3s2_bwd_terms(b, h, w, c, n)  # the seam raises off-strip
    pixels = terms[:, :, 0, 2].reshape(-1)
    assert torch.equal(pixels.sort().values, torch.arange(b * h * w))
    g = torch.Generator().manual_seed(h * 31 + w)
    dy = torch.randn(b, n, ho, wo, generator=g, dtype=torch.float64)
    wt = torch.randn(n, c, 3, 3, generator=g, dtype=torch.float64)
    rows = dy.permute(0, 2, 3, 1).reshape(-1, n)
    dx = torch.zeros(b * h * w, c, dtype=torch.float64)
    counts = []
    for cls in range(4):
        for term in range(4):
            tap, src, pix = terms[:, cls, term].unbind(1)
            if int(tap[0]) < 0:
                assert bool((terms[:, cls, term] == -1).all())
                continue
            assert bool((tap == tap[0]).all())
            assert bool((pix == terms[:, cls, 0, 2]).all())
            live = src >= 0
            dx.index_add_(0, pix[live], rows[src[live]]
                          @ wt[:, :, int(tap[0]) // 3, int(tap[0]) % 3])
            counts.append(cls)
    assert [counts.count(k) for k in range(4)] == [1, 2, 2, 4]
    want = F.conv_transpose2d(dy, wt, stride=2, padding=1, output_padding=1)
    want = want.permute(0, 2, 3, 1).reshape(-1, c)
    assert float((dx - want).abs().max()) <= 1e-12 * float(want.abs().max())


def test_the_gpu_shapes_reach_the_plans_they_are_for():
    plans = [_C.conv3x3s2_bwd_plan(*s) for s in GRID[:len(GPU)]]
    assert all(p["eligible"] and p["tile_rows"] == 128 for p in plans)
    assert plans[0]["rows"] == 2  # one dY pixel an image: every shift masked
    assert (plans[1]["ho"], plans[1]["wo"]) == (2, 3)
    assert all(plans[i]["row_tiles"] == 1 for i in (0, 1, 3, 5, 6))
    # 147 rows: two tiles, the last short, the third image across the boundary
    assert plans[2]["row_tiles"] == 2 and plans[2]["rows"] == 147
    assert (plans[2]["nchunks"], plans[2]["ntiles"]) == (4, 1)
    assert (plans[3]["nchunks"], plans[3]["ntiles"]) == (2, 2)
    assert plans[4]["row_tiles"] == 2 and plans[4]["rows"] == 168  # short
    assert [(plans[i]["ntiles"], plans[i]["nchunks"]) for i in (5, 6)] == [
        (4, 8), (8, 16)]
    assert plans[7]["grid"] == 2 and plans[7]["tiles_per_split"] == 3
    assert plans[8]["ntiles"] == 2 and plans[8]["splits"] == 3
    assert plans[8]["tiles_per_split"] == 17


def test_what_is_eligible_and_what_is_native():
    good = [(4, 10, 10, c, n) for c in (64, 128, 256, 512)
            for n in (64, 128, 256, 512)]
    for ok in good + [(2, 4, w, 64, 64) for w in range(2, 128, 2)] + [
            (1, 2, 4, 64, 64), (1 << 12, 1 << 6, 1 << 6, 64, 64),
            (2, 2048, 2, 64, 64)]:
        p = _C.conv3x3s2_bwd_plan(*ok)
        assert p["eligible"] and p["lds_bytes"] <= 160 * 1024, ok
    for bad in ((2, 4, 4, 32, 64), (2, 4, 4, 64, 96), (2, 4, 4, 1024, 64),
                (2, 4, 4, 64, 1024), (0, 4, 4, 64, 64), (2, 0, 4, 64, 64),
                (2, 4, 0, 64, 64), (2, 5, 4, 64, 64), (2, 4, 5, 64, 64),
                (1, 2, 2, 64, 64), (2, 4, 128, 64, 64), (2, 4096, 2, 64, 64),
                (1 << 13, 1 << 7, 1 << 5, 64, 64)):
        p = _C.conv3x3s2_bwd_plan(*bad)
        assert not p["eligible"] and not p["native"], bad
    # kNativeBwd3x3S2 is empty: none of ResNet-50's three met the rule
    for h, c in ((56, 128), (28, 256), (14, 512)):
        for other in ((256, h, h, c, c), (128, h, h, c, c),
                      (256, h, h - 2, c, c), (256, h, h, c, c // 2)):
            q = _C.conv3x3s2_bwd_plan(*other)
            assert q["eligible"] and not q["native"], other
        assert _C.conv3x3s2_bwd_plan(256, h, h, c, c)["grid"] == 256
