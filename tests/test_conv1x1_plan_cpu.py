"""Launch geometry of the 1x1 convolution with statistics (csrc/conv1x1_plan.h):
the tile walk the kernel runs, replayed on the host."""

import pytest
import torch

from torch_cgx_amd import _C

# (rows, K, N, max_workgroups): the twelve stride-1 1x1 forward problems of the
# ResNet-50 benchmark at batch 256 ...
BENCH = [(256 * hw * hw, k, n, 0) for k, n, hw in [
    (64, 64, 56), (64, 256, 56), (256, 64, 56), (256, 128, 56),
    (128, 512, 28), (512, 128, 28), (512, 256, 28),
    (256, 1024, 14), (1024, 256, 14), (1024, 512, 14),
    (512, 2048, 7), (2048, 512, 7)]]
# ... and the shapes of tests/test_gpu_conv1x1_bn.py
SMALL = [(2, 64, 64, 0), (98, 64, 256, 0), (75, 256, 64, 0),
         (162, 128, 512, 0), (18, 2048, 512, 0), (18, 512, 2048, 0),
         (6272, 64, 256, 0), (1568, 64, 256, 3), (1 << 24, 64, 64, 0),
         (129, 2048, 2048, 0), (128, 64, 64, 0), (12544, 512, 2048, 5)]
SHAPES = BENCH + SMALL
LDS_LIMIT = 160 * 1024


def _id(s):
    return "R{}-{}to{}-wg{}".format(*s)


@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_geometry(shape):
    rows, k, n, max_wg = shape
    p = _C.conv1x1_plan(rows, k, n, max_wg)
    assert p["eligible"]
    assert p["threads"] == 256 and p["tile_rows"] == 128
    assert p["tile_channels"] == 32 * p["mfma_tiles"]
    assert p["mfma_tiles"] in (2, 4, 8)
    assert p["tile_channels"] * p["ntiles"] == n
    assert p["k_chunk"] * p["k_chunks"] == k
    assert p["row_tiles"] == -(-rows // 128)
    assert p["grid"] == p["ntiles"] * p["splits"]
    assert 1 <= p["splits"] <= p["row_tiles"]
    assert p["tiles_per_split"] == -(-p["row_tiles"] // p["splits"])
    assert p["run"] == 16 * p["tiles_per_split"]
    if max_wg:
        assert p["grid"] <= max(max_wg, p["ntiles"])
    # W (whole or one K chunk) and four 4 KiB strips, within the LDS of a CU
    w_rows_k = k if p["resident"] else p["k_chunk"]
    assert p["lds_bytes"] == p["tile_channels"] * w_rows_k * 2 + 16 * 1024
    assert p["lds_bytes"] <= LDS_LIMIT
    # the final merge reuses the W area: 16 rows of tile_channels floats + 8
    assert (16 * p["tile_channels"] + 8) * 4 <= p["lds_bytes"] - 16 * 1024
    if not p["resident"]:
        assert p["tile_channels"] * k * 2 > 128 * 1024


@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_partials_stay_small(shape):
    rows, k, n, max_wg = shape
    p = _C.conv1x1_plan(rows, k, n, max_wg)
    assert p["partial_stride"] == 2 * n + p["ntiles"]
    assert p["partial_floats"] == p["splits"] * p["partial_stride"]
    if p["splits"] > 1:
        assert 4 * p["partial_floats"] <= 0.05 * 2 * rows * n


@pytest.mark.parametrize("shape", [s for s in SHAPES if s[0] <= 1 << 20],
                         ids=_id)
def test_walk_visits_every_tile_once(shape):
    rows, k, n, max_wg = shape
    p = _C.conv1x1_plan(rows, k, n, max_wg)
    walk = _C.conv1x1_walk(rows, k, n, max_wg)
    assert tuple(walk.shape) == (p["grid"], p["tiles_per_split"], 4)
    live = walk[..., 0] >= 0
    # a workgroup's tiles come first, in ascending row order, and it has one
    assert bool(live[:, 0].all())
    assert bool((live[:, 1:] <= live[:, :-1]).all())
    t = walk[live]
    r0, r1, n0, n1 = t.unbind(1)
    assert bool((r0 % 128 == 0).all()) and bool((n0 % p["tile_channels"] == 0).all())
    assert bool((n1 - n0 == p["tile_channels"]).all())
    # tail rows are excluded
    assert bool((r1 == torch.clamp(r0 + 128, max=rows)).all())
    assert bool((r1 > r0).all())
    # every (row tile, channel tile) exactly once
    key = (r0 // 128) * p["ntiles"] + n0 // p["tile_channels"]
    assert key.numel() == p["row_tiles"] * p["ntiles"]
    assert torch.equal(key.sort().values, torch.arange(key.numel()))
    # ... which covers [0, R) x [0, N)
    cover = torch.zeros(rows, dtype=torch.int64)
    for a, b in zip(r0[n0 == 0].tolist(), r1[n0 == 0].tolist()):
        cover[a:b] += 1
    assert bool((cover == 1).all())
    # one workgroup keeps one channel tile, and its run length is the plan's
    for wg in range(0, p["grid"], max(1, p["grid"] // 7)):
        mine = walk[wg][live[wg]]
        assert mine[:, 2].unique().numel() == 1
        assert bool((mine[1:, 0] > mine[:-1, 0]).all())
        assert 16 * mine.shape[0] <= p["run"]


@pytest.mark.parametrize("rows,k,n", [(1, 64, 64), (98, 32, 64), (98, 64, 32),
                                      (98, 96, 64), (98, 64, 4096),
                                      (98, 4096, 64), ((1 << 24) + 1, 64, 64),
                                      (98, 0, 64)])
def test_ineligible(rows, k, n):
    p = _C.conv1x1_plan(rows, k, n)
    assert not p["eligible"] and not p["native"]
    with pytest.raises(RuntimeError):
        _C.conv1x1_walk(rows, k, n)


NATIVE = {(64, 64), (64, 256), (256, 64), (256, 128), (128, 512), (512, 128),
          (256, 1024)}


def test_native_only_where_measured_faster():
    """The per-shape decision lives in the plan: seven of the benchmark's
    twelve shapes, at the row count they were measured at, and nothing else."""
    for rows, k, n, _ in BENCH:
        assert _C.conv1x1_plan(rows, k, n)["native"] == ((k, n) in NATIVE)
        assert not _C.conv1x1_plan(rows // 2, k, n)["native"]
    for rows, k, n, _ in SMALL:
        assert not _C.conv1x1_plan(rows, k, n)["native"]
