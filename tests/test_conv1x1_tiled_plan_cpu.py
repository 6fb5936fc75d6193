"""Launch geometry of the tiled walk of the native 1x1 convolution
(conv1x1_tiled_plan / conv1x1_tiled_bwd_plan in csrc/conv1x1_plan.h): the
tile walk the kernels run, replayed on the host."""

import pytest
import torch

from torch_cgx_amd import _C

PROBLEMS = [(64, 64, 56), (64, 256, 56), (256, 64, 56), (256, 128, 56),
            (128, 512, 28), (512, 128, 28), (512, 256, 28),
            (256, 1024, 14), (1024, 256, 14), (1024, 512, 14),
            (512, 2048, 7), (2048, 512, 7)]
# (rows, K, N, max_workgroups): the twelve stride-1 1x1 problems of the
# ResNet-50 benchmark at batch 256, free and with a capped grid ...
BENCH = [(256 * hw * hw, k, n, wg) for k, n, hw in PROBLEMS for wg in (0, 100)]
# ... and the shapes of tests/test_gpu_conv1x1_tiled.py
SMALL = [(98, 64, 128, 0), (2, 128, 128, 0), (75, 1024, 256, 0),
         (392, 1024, 256, 0), (18, 2048, 512, 0), (18, 512, 2048, 0),
         (1568, 256, 1024, 3), (18, 128, 64, 0), (257, 2048, 2048, 5)]
SHAPES = BENCH + SMALL
LDS_LIMIT = 160 * 1024

# the problems in kNativeTiled / kNativeTiledBwd (csrc/conv1x1_plan.cc)
NATIVE = {(512, 256), (1024, 256), (1024, 512), (512, 2048), (2048, 512)}
# (K, N, with_add)
NATIVE_BWD = {(64, 64, False), (64, 256, True), (256, 64, False),
              (256, 128, False), (128, 512, True), (512, 128, False),
              (512, 256, False), (256, 1024, False), (256, 1024, True),
              (1024, 256, False), (1024, 512, False), (1024, 512, True),
              (512, 2048, False), (512, 2048, True), (2048, 512, False),
              (2048, 512, True)}


def _id(s):
    return "R{}-{}to{}-wg{}".format(*s)


def _plans(shape):
    """The forward plan and the two backward-data ones with the width they
    produce and their strips' bytes."""
    rows, k, n, wg = shape
    return [(_C.conv1x1_tiled_plan(rows, k, n, wg), k, n, 16 * 1024),
            (_C.conv1x1_tiled_bwd_plan(rows, k, n, False, wg), n, k, 32 * 1024),
            (_C.conv1x1_tiled_bwd_plan(rows, k, n, True, wg), n, k, 32 * 1024)]


@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_geometry(shape):
    rows, _, _, max_wg = shape
    for p, contracted, produced, strips in _plans(shape):
        assert p["eligible"] and not p["resident"]
        assert p["threads"] == 256 and p["tile_rows"] == 256
        assert p["mfma_tiles"] in (2, 4)
        assert p["tile_channels"] == 32 * p["mfma_tiles"] == min(produced, 128)
        assert p["tile_channels"] * p["ntiles"] == produced
        # B staged per tile at most half of A streamed
        assert 2 * p["tile_channels"] <= p["tile_rows"]
        assert p["k_chunk"] == 64 and p["k_chunks"] * 64 == contracted
        assert p["row_tiles"] == -(-rows // 256)
        assert p["grid"] == p["ntiles"] * p["splits"]
        assert 1 <= p["splits"] <= p["row_tiles"]
        assert p["tiles_per_split"] == -(-p["row_tiles"] // p["splits"])
        if max_wg:
            assert p["grid"] <= max(max_wg, p["ntiles"])
        # two stages of B beside the strips, within the LDS of a CU
        assert p["lds_bytes"] == 2 * p["tile_channels"] * 64 * 2 + strips
        assert p["lds_bytes"] <= LDS_LIMIT
    p = _plans(shape)[0][0]
    assert p["run"] == 32 * p["tiles_per_split"]
    # the final merge reuses the B area: 16 rows of tile_channels floats + 8
    assert (16 * p["tile_channels"] + 8) * 4 <= p["lds_bytes"] - 16 * 1024


@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_partials_stay_small(shape):
    rows, k, n, max_wg = shape
    p = _C.conv1x1_tiled_plan(rows, k, n, max_wg)
    assert p["partial_stride"] == 2 * n + p["ntiles"]
    assert p["partial_floats"] == p["splits"] * p["partial_stride"]
    assert n % (8 * p["ntiles"]) == 0
    if p["splits"] > 1:
        assert 4 * p["partial_floats"] <= 0.05 * 2 * rows * n


def _check_walk(p, walk, rows):
    tc = p["tile_channels"]
    assert tuple(walk.shape) == (p["grid"], p["tiles_per_split"], 4)
    live = walk[..., 0] >= 0
    # a workgroup's tiles come first, and it has one
    assert bool(live[:, 0].all())
    assert bool((live[:, 1:] <= live[:, :-1]).all())
    r0, r1, n0, n1 = walk[live].unbind(1)
    assert bool((r0 % 256 == 0).all()) and bool((n0 % tc == 0).all())
    assert bool((n1 - n0 == tc).all())
    assert bool((r1 == torch.clamp(r0 + 256, max=rows)).all())
    assert bool((r1 > r0).all())
    # every (row tile, channel tile) exactly once
    key = (r0 // 256) * p["ntiles"] + n0 // tc
    assert key.numel() == p["row_tiles"] * p["ntiles"]
    assert torch.equal(key.sort().values, torch.arange(key.numel()))
    # ... which covers [0, R) x [0, N)
    for c0 in n0.unique().tolist():
        edges = torch.stack([r0[n0 == c0], r1[n0 == c0]], 1)
        edges = edges[edges[:, 0].argsort()]
        assert int(edges[0, 0]) == 0 and int(edges[-1, 1]) == rows
        assert bool((edges[1:, 0] == edges[:-1, 1]).all())
    assert n0.unique().numel() == p["ntiles"]
    # a workgroup keeps one channel tile and walks its rows upward
    for wg in range(0, p["grid"], max(1, p["grid"] // 7)):
        mine = walk[wg][live[wg]]
        assert mine[:, 2].unique().numel() == 1
        assert bool((mine[1:, 0] > mine[:-1, 0]).all())


@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_walk_visits_every_tile_once(shape):
    rows, k, n, max_wg = shape
    p = _C.conv1x1_tiled_plan(rows, k, n, max_wg)
    _check_walk(p, _C.conv1x1_tiled_walk(rows, k, n, max_wg), rows)
    assert 32 * p["tiles_per_split"] == p["run"]
    for add in (False, True):
        _check_walk(_C.conv1x1_tiled_bwd_plan(rows, k, n, add, max_wg),
                    _C.conv1x1_tiled_bwd_walk(rows, k, n, add, max_wg), rows)


def test_workgroups_that_share_rows_share_an_xcd():
    """Where the splits divide by 8, the channel tiles of a split have block
    indices 8 apart."""
    rows, k, n = 256 * 14 * 14, 1024, 512
    p = _C.conv1x1_tiled_plan(rows, k, n)
    assert p["splits"] % 8 == 0 and p["ntiles"] == 4
    walk = _C.conv1x1_tiled_walk(rows, k, n)
    for wg in (0, 5, 8 * p["ntiles"] + 3):
        same = [wg + 8 * j for j in range(p["ntiles"] - wg // 8 % p["ntiles"])]
        assert len({int(walk[w, 0, 0]) for w in same}) == 1
        assert len({int(walk[w, 0, 2]) for w in same}) == len(same)


@pytest.mark.parametrize("rows,k,n", [(1, 64, 64), (98, 32, 64), (98, 64, 32),
                                      (98, 96, 64), (98, 64, 4096),
                                      (98, 4096, 64), ((1 << 24) + 1, 64, 64),
                                      (98, 0, 64)])
def test_ineligible(rows, k, n):
    for p in (_C.conv1x1_tiled_plan(rows, k, n),
              _C.conv1x1_tiled_bwd_plan(rows, k, n, False),
              _C.conv1x1_tiled_bwd_plan(rows, k, n, True)):
        assert not p["eligible"] and not p["native"]
    with pytest.raises(RuntimeError):
        _C.conv1x1_tiled_walk(rows, k, n)
    with pytest.raises(RuntimeError):
        _C.conv1x1_tiled_bwd_walk(rows, k, n)


def test_native_only_where_measured_faster():
    for k, n, hw in PROBLEMS:
        rows = 256 * hw * hw
        assert _C.conv1x1_tiled_plan(rows, k, n)["native"] == (
            (k, n) in NATIVE)
        assert not _C.conv1x1_tiled_plan(rows // 2, k, n)["native"]
        for add in (False, True):
            assert _C.conv1x1_tiled_bwd_plan(rows, k, n, add)["native"] == (
                (k, n, add) in NATIVE_BWD)
            assert not _C.conv1x1_tiled_bwd_plan(rows // 2, k, n,
                                                 add)["native"]
    for rows, k, n, wg in SMALL:
        assert not _C.conv1x1_tiled_plan(rows, k, n, wg)["native"]
        for add in (False, True):
            assert not _C.conv1x1_tiled_bwd_plan(rows, k, n, add, wg)["native"]


KEYS = ("native", "mfma_tiles", "ntiles", "k_chunk", "resident", "splits",
        "grid", "tiles_per_split", "lds_bytes")
# rows of FORWARD and BACKWARD in test_conv1x1_wrw_plan_cpu.py, by problem:
# conv1x1_plan's KEYS and partial_floats; conv1x1_bwd_plan's `native` without
# and with the add, then the rest of KEYS
OLD_FORWARD = {
    (64, 256, 56): (True, 8, 1, 64, True, 256, 256, 25, 49152, 131328),
    (512, 256, 28): (False, 8, 1, 128, False, 256, 256, 7, 81920, 131328),
    (256, 1024, 14): (True, 8, 4, 128, True, 64, 256, 7, 147456, 131328),
    (1024, 256, 14): (False, 8, 1, 128, False, 256, 256, 2, 81920, 131328),
    (2048, 512, 7): (False, 8, 2, 128, False, 98, 196, 1, 81920, 100548),
}
OLD_BACKWARD = {
    (64, 256, 56): (True, False, 2, 1, 128, True, 512, 512, 13, 65536),
    (512, 256, 28): (False, True, 8, 2, 128, True, 128, 256, 13, 163840),
    (256, 1024, 14): (False, False, 8, 1, 128, False, 256, 256, 2, 98304),
    (1024, 512, 14): (False, False, 8, 4, 128, False, 64, 256, 7, 98304),
    (512, 2048, 7): (False, False, 8, 2, 128, False, 98, 196, 1, 98304),
}


def test_the_old_plans_are_what_they_were():
    for (k, n, hw), want in OLD_FORWARD.items():
        p = _C.conv1x1_plan(256 * hw * hw, k, n)
        assert p["tile_rows"] == 128
        assert tuple(p[key] for key in KEYS + ("partial_floats",)) == want
    for (k, n, hw), want in OLD_BACKWARD.items():
        for add in (False, True):
            q = _C.conv1x1_bwd_plan(256 * hw * hw, k, n, add)
            assert q["native"] == want[int(add)]
            assert tuple(q[key] for key in KEYS[1:]) == want[2:]
    p = _C.conv1x1_wrw_plan(256 * 7 * 7, 2048, 512)
    assert p["native"] and p["chunk_rows"] == 64
    assert not _C.conv1x1_wrw_plan(256 * 56 * 56, 64, 64)["native"]
