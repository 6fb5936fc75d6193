"""Launch geometry of the 1x1 convolution's backward-data GEMM
(conv1x1_bwd_plan in csrc/conv1x1_plan.h): the forward geometry with k and n
exchanged.  dX is K wide and tiled, dY's N channels are contracted."""

import pytest
import torch

from torch_cgx_amd import _C

# (rows, K of dX, N of dY, with_add, max_workgroups): the twelve stride-1 1x1
# problems of the ResNet-50 benchmark at batch 256, the first eight with a
# skip gradient to add ...
FORK = [(64, 64, 56), (256, 64, 56), (256, 128, 56), (512, 128, 28),
        (512, 256, 28), (1024, 256, 14), (1024, 512, 14), (2048, 512, 7)]
PLAIN = [(64, 256, 56), (128, 512, 28), (256, 1024, 14), (512, 2048, 7)]
BENCH = ([(256 * hw * hw, k, n, True, 0) for k, n, hw in FORK]
         + [(256 * hw * hw, k, n, False, 0) for k, n, hw in PLAIN])
# ... and the shapes of tests/test_gpu_conv1x1_bwd.py, with others at the
# limits of the plan
SMALL = [(2, 64, 64, False, 0), (98, 256, 64, True, 0), (75, 64, 256, False, 0),
         (50, 128, 256, True, 0), (162, 512, 128, False, 0),
         (18, 512, 2048, True, 0), (18, 2048, 512, False, 0),
         (6272, 256, 64, True, 0), (1568, 256, 64, True, 3),
         (18, 128, 64, False, 0), (18, 64, 2048, True, 0),
         (18, 128, 2048, False, 0), (18, 256, 256, True, 0),
         (1 << 24, 64, 64, False, 0), (129, 2048, 2048, True, 0),
         (128, 64, 64, True, 0), (12544, 2048, 512, False, 5)]
SHAPES = BENCH + SMALL
LDS_LIMIT = 160 * 1024
STRIPS = 32 * 1024  # four waves x [32 rows][64 channels] of fp32


def _id(s):
    return "R{}-dx{}-dy{}-add{:d}-wg{}".format(*s)


@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_geometry(shape):
    rows, k, n, add, max_wg = shape
    p = _C.conv1x1_bwd_plan(rows, k, n, add, max_wg)
    assert p["eligible"]
    assert p["threads"] == 256 and p["tile_rows"] == 128
    assert p["tile_channels"] == 32 * p["mfma_tiles"]
    assert p["mfma_tiles"] in (2, 4, 8)
    # dX's K channels are tiled, dY's N channels are contracted in chunks
    assert p["tile_channels"] * p["ntiles"] == k
    assert p["k_chunk"] * p["k_chunks"] == n
    assert p["k_chunk"] == (64 if n == 64 else 128)
    assert p["row_tiles"] == -(-rows // 128)
    assert p["grid"] == p["ntiles"] * p["splits"]
    assert 1 <= p["splits"] <= p["row_tiles"]
    assert p["tiles_per_split"] == -(-p["row_tiles"] // p["splits"])
    if max_wg:
        assert p["grid"] <= max(max_wg, p["ntiles"])
    # W^T (whole or one chunk) and the four fp32 strips, within the LDS of a CU
    w_cols = n if p["resident"] else p["k_chunk"]
    assert p["lds_bytes"] == p["tile_channels"] * w_cols * 2 + STRIPS
    assert p["lds_bytes"] <= LDS_LIMIT
    if not p["resident"]:
        assert p["tile_channels"] * n * 2 > 128 * 1024
    # the add changes which kernel runs, not where
    q = _C.conv1x1_bwd_plan(rows, k, n, not add, max_wg)
    for key in p:
        if key != "native":
            assert p[key] == q[key], key


@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_is_the_forward_geometry_with_k_and_n_exchanged(shape):
    rows, k, n, add, max_wg = shape
    p = _C.conv1x1_bwd_plan(rows, k, n, add, max_wg)
    f = _C.conv1x1_plan(rows, n, k, max_wg)
    for key in ("mfma_tiles", "tile_channels", "ntiles", "k_chunk", "k_chunks",
                "resident", "row_tiles"):
        assert p[key] == f[key], key
    assert p["lds_bytes"] == f["lds_bytes"] + 16 * 1024


@pytest.mark.parametrize("shape", [s for s in SHAPES if s[0] <= 1 << 20],
                         ids=_id)
def test_walk_visits_every_tile_once(shape):
    rows, k, n, add, max_wg = shape
    p = _C.conv1x1_bwd_plan(rows, k, n, add, max_wg)
    walk = _C.conv1x1_bwd_walk(rows, k, n, add, max_wg)
    assert tuple(walk.shape) == (p["grid"], p["tiles_per_split"], 4)
    live = walk[..., 0] >= 0
    assert bool(live[:, 0].all())
    assert bool((live[:, 1:] <= live[:, :-1]).all())
    r0, r1, c0, c1 = walk[live].unbind(1)
    assert bool((r0 % 128 == 0).all())
    assert bool((c0 % p["tile_channels"] == 0).all())
    assert bool((c1 - c0 == p["tile_channels"]).all())
    assert bool((c1 <= k).all())
    # rows past R are excluded
    assert bool((r1 == torch.clamp(r0 + 128, max=rows)).all())
    assert bool((r1 > r0).all())
    # every row tile exactly once per channel tile
    key = (r0 // 128) * p["ntiles"] + c0 // p["tile_channels"]
    assert key.numel() == p["row_tiles"] * p["ntiles"]
    assert torch.equal(key.sort().values, torch.arange(key.numel()))
    for c in range(0, k, p["tile_channels"]):
        cover = torch.zeros(rows, dtype=torch.int64)
        for a, b in zip(r0[c0 == c].tolist(), r1[c0 == c].tolist()):
            cover[a:b] += 1
        assert bool((cover == 1).all())
    # one workgroup keeps one channel tile and walks upwards
    for wg in range(0, p["grid"], max(1, p["grid"] // 7)):
        mine = walk[wg][live[wg]]
        assert mine[:, 2].unique().numel() == 1
        assert bool((mine[1:, 0] > mine[:-1, 0]).all())


@pytest.mark.parametrize("rows,k,n", [(1, 64, 64), (98, 32, 64), (98, 64, 32),
                                      (98, 96, 64), (98, 64, 4096),
                                      (98, 4096, 64), ((1 << 24) + 1, 64, 64),
                                      (98, 0, 64)])
def test_ineligible(rows, k, n):
    for add in (False, True):
        p = _C.conv1x1_bwd_plan(rows, k, n, add)
        assert not p["eligible"] and not p["native"]
        with pytest.raises(RuntimeError):
            _C.conv1x1_bwd_walk(rows, k, n, add)


# (K of dX, N of dY, with_add) that met the rule of benchmarks/RESULTS.md: the
# slowest native run faster than the fastest stock run
NATIVE = {(64, 64, True), (256, 64, True), (256, 128, True), (512, 128, True),
          (512, 256, True), (1024, 256, True), (64, 256, False),
          (128, 512, False)}


def test_native_only_where_measured_faster():
    """The per-problem decision lives in the plan: the benchmark's problems
    that were measured faster, at the row count and with the add they were
    measured with, and nothing else."""
    for rows, k, n, add, _ in BENCH:
        for with_add in (False, True):
            want = (k, n, with_add) in NATIVE
            assert _C.conv1x1_bwd_plan(rows, k, n, with_add)["native"] == want
        assert not _C.conv1x1_bwd_plan(rows // 2, k, n, add)["native"]
    for rows, k, n, add, _ in SMALL:
        assert not _C.conv1x1_bwd_plan(rows, k, n, add)["native"]


def test_forward_plan_is_untouched():
    p = _C.conv1x1_plan(802816, 256, 64)
    assert p["native"] and p["lds_bytes"] == 64 * 256 * 2 + 16 * 1024
    assert "run" in p and "partial_floats" in p
