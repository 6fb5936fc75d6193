"""Launch geometry of the 1x1 convolution's backward-weights GEMM
(conv1x1_wrw_plan in csrc/conv1x1_plan.h): dW[N, K] in bn x bk tiles, the rows
in 64-row chunks dealt to `splits` workgroups per tile."""

import pytest
import torch

from torch_cgx_amd import _C

# (K, N, image side): the twelve stride-1 1x1 problems of the ResNet-50
# benchmark at batch 256 ...
PROBLEMS = [(64, 64, 56), (64, 256, 56), (256, 64, 56), (256, 128, 56),
            (128, 512, 28), (512, 128, 28), (512, 256, 28), (256, 1024, 14),
            (1024, 256, 14), (1024, 512, 14), (512, 2048, 7), (2048, 512, 7)]
BENCH = [(256 * hw * hw, k, n, 0) for k, n, hw in PROBLEMS]
# ... and (rows, K, N, max_workgroups) of tests/test_gpu_conv1x1_wrw.py, with
# others at the limits of the plan
SMALL = [(2, 64, 64, 0), (98, 256, 64, 0), (75, 64, 256, 0), (50, 128, 256, 0),
         (128, 512, 128, 0), (18, 512, 2048, 0), (18, 2048, 512, 0),
         (6272, 256, 64, 0), (1568, 256, 64, 3), (50, 64, 256, 0),
         (50, 256, 64, 0), (1 << 24, 64, 64, 0), (129, 2048, 2048, 0),
         (64, 64, 64, 0), (65, 64, 64, 0), (12544, 2048, 512, 5),
         (802816, 64, 64, 100), (200704, 512, 256, 1)]
SHAPES = BENCH + SMALL
LDS_LIMIT = 160 * 1024


def _id(s):
    return "R{}-k{}-n{}-wg{}".format(*s)


@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_geometry(shape):
    rows, k, n, max_wg = shape
    p = _C.conv1x1_wrw_plan(rows, k, n, max_wg)
    assert p["eligible"]
    assert p["threads"] == 256 and p["chunk_rows"] == 64
    assert p["bn"] in (64, 128, 256) and p["bk"] in (64, 128, 256)
    assert (p["bn"], p["bk"]) != (256, 256)  # not instantiated
    assert p["bn"] * p["ntiles_n"] == n
    assert p["bk"] * p["ntiles_k"] == k
    # one chunk of dY's and of X's channels of the tile
    assert p["lds_bytes"] == 64 * (p["bn"] + p["bk"]) * 2
    assert p["lds_bytes"] <= LDS_LIMIT
    assert p["row_chunks"] == -(-rows // 64)
    assert 1 <= p["splits"] <= p["row_chunks"]
    tiles = p["ntiles_n"] * p["ntiles_k"]
    assert p["grid"] == tiles * p["splits"]
    assert p["chunks_per_split"] == -(-p["row_chunks"] // p["splits"])
    assert p["partial_floats"] == p["splits"] * n * k
    # the partials, written and read back, within half of the input bytes
    # wherever there is a choice
    if p["splits"] > 1:
        assert 2 * 4 * p["partial_floats"] <= rows * (n + k)
    if max_wg:
        assert p["grid"] <= max(max_wg, tiles)
    else:
        q = _C.conv1x1_wrw_plan(rows, k, n, 1 << 30)
        assert q == p


@pytest.mark.parametrize("shape", [s for s in SHAPES if s[0] <= 1 << 20],
                         ids=_id)
def test_walk_visits_every_chunk_of_every_tile_once(shape):
    rows, k, n, max_wg = shape
    p = _C.conv1x1_wrw_plan(rows, k, n, max_wg)
    walk = _C.conv1x1_wrw_walk(rows, k, n, max_wg)
    assert tuple(walk.shape) == (p["grid"], p["chunks_per_split"], 5)
    live = walk[..., 0] >= 0
    assert bool(live[:, 0].all())  # no workgroup without rows
    assert bool((live[:, 1:] <= live[:, :-1]).all())
    n0, k0, split, r0, r1 = walk[live].unbind(1)
    assert bool((n0 % p["bn"] == 0).all()) and bool((n0 < n).all())
    assert bool((k0 % p["bk"] == 0).all()) and bool((k0 < k).all())
    assert bool((r0 % 64 == 0).all())
    # no chunk starts at or beyond R, and rows past R are excluded
    assert bool((r0 < rows).all())
    assert bool((r1 == torch.clamp(r0 + 64, max=rows)).all())
    tiles = p["ntiles_n"] * p["ntiles_k"]
    tile = (n0 // p["bn"]) * p["ntiles_k"] + k0 // p["bk"]
    key = (r0 // 64) * tiles + tile
    assert key.numel() == p["row_chunks"] * tiles
    assert torch.equal(key.sort().values, torch.arange(key.numel()))
    # a workgroup keeps one tile and one plane of the partials and walks
    # upwards; a (tile, plane) pair belongs to one workgroup
    owner = set()
    for wg in range(p["grid"]):
        mine = walk[wg][live[wg]]
        assert mine[:, :3].unique(dim=0).shape[0] == 1
        assert bool((mine[1:, 3] > mine[:-1, 3]).all())
        assert 0 <= int(mine[0, 2]) < p["splits"]
        owner.add(tuple(mine[0, :3].tolist()))
    assert len(owner) == p["grid"]


def test_workgroups_of_a_row_slice_are_eight_apart():
    """Where the splits divide by 8, the workgroups that read the same rows
    have block indices that are equal modulo 8."""
    for rows, k, n, _ in BENCH:
        p = _C.conv1x1_wrw_plan(rows, k, n)
        if p["splits"] % 8:
            continue
        walk = _C.conv1x1_wrw_walk(rows, k, n)
        split = walk[:, 0, 2]
        for s in range(0, p["splits"], max(1, p["splits"] // 5)):
            wgs = (split == s).nonzero().flatten()
            assert wgs.numel() == p["ntiles_n"] * p["ntiles_k"]
            assert (wgs % 8).unique().numel() == 1


@pytest.mark.parametrize("rows,k,n", [(1, 64, 64), (98, 32, 64), (98, 64, 32),
                                      (98, 96, 64), (98, 64, 4096),
                                      (98, 4096, 64), ((1 << 24) + 1, 64, 64),
                                      (98, 0, 64)])
def test_ineligible(rows, k, n):
    p = _C.conv1x1_wrw_plan(rows, k, n)
    assert not p["eligible"] and not p["native"]
    with pytest.raises(RuntimeError):
        _C.conv1x1_wrw_walk(rows, k, n)


# (K, N) that met the rule of benchmarks/RESULTS.md: the slowest native run
# faster than the fastest stock run
NATIVE = {(k, n) for k, n, _ in PROBLEMS} - {(64, 64)}


def test_native_only_where_measured_faster():
    for rows, k, n, _ in BENCH:
        assert _C.conv1x1_wrw_plan(rows, k, n)["native"] == ((k, n) in NATIVE)
        assert not _C.conv1x1_wrw_plan(rows // 2, k, n)["native"]
    for rows, k, n, max_wg in SMALL:
        if (rows, k, n, 0) not in BENCH:
            assert not _C.conv1x1_wrw_plan(rows, k, n, max_wg)["native"]


KEYS = ("native", "mfma_tiles", "ntiles", "k_chunk", "resident", "splits",
        "grid", "tiles_per_split", "lds_bytes")
# conv1x1_plan of the twelve problems, in the order of PROBLEMS, as the
# commit before conv1x1_wrw_plan gave them: KEYS and partial_floats
FORWARD = [
    (True, 2, 1, 64, True, 768, 768, 9, 24576, 99072),
    (True, 8, 1, 64, True, 256, 256, 25, 49152, 131328),
    (True, 2, 1, 128, True, 768, 768, 9, 49152, 99072),
    (True, 4, 1, 128, True, 512, 512, 13, 81920, 131584),
    (True, 8, 2, 128, True, 128, 256, 13, 81920, 131328),
    (True, 4, 1, 128, True, 256, 256, 7, 147456, 65792),
    (False, 8, 1, 128, False, 256, 256, 7, 81920, 131328),
    (True, 8, 4, 128, True, 64, 256, 7, 147456, 131328),
    (False, 8, 1, 128, False, 256, 256, 2, 81920, 131328),
    (False, 8, 2, 128, False, 128, 256, 4, 81920, 131328),
    (False, 8, 8, 128, False, 32, 256, 4, 81920, 131328),
    (False, 8, 2, 128, False, 98, 196, 1, 81920, 100548),
]
# conv1x1_bwd_plan likewise: `native` without and with the add, then the
# rest of KEYS, which the add does not change
BACKWARD = [
    (False, True, 2, 1, 64, True, 1024, 1024, 7, 40960),
    (True, False, 2, 1, 128, True, 512, 512, 13, 65536),
    (False, True, 8, 1, 64, True, 512, 512, 13, 65536),
    (False, True, 8, 1, 128, True, 256, 256, 25, 98304),
    (True, False, 4, 1, 128, True, 256, 256, 7, 163840),
    (False, True, 8, 2, 128, True, 128, 256, 13, 98304),
    (False, True, 8, 2, 128, True, 128, 256, 13, 163840),
    (False, False, 8, 1, 128, False, 256, 256, 2, 98304),
    (False, True, 8, 4, 128, True, 64, 256, 7, 163840),
    (False, False, 8, 4, 128, False, 64, 256, 7, 98304),
    (False, False, 8, 2, 128, False, 98, 196, 1, 98304),
    (False, False, 8, 8, 128, False, 32, 256, 4, 98304),
]


def test_the_other_two_plans_are_untouched():
    for (rows, k, n, _), fwd, bwd in zip(BENCH, FORWARD, BACKWARD):
        p = _C.conv1x1_plan(rows, k, n)
        assert tuple(p[key] for key in KEYS + ("partial_floats",)) == fwd
        assert p["eligible"] and p["tile_channels"] == 32 * p["mfma_tiles"]
        for add in (False, True):
            q = _C.conv1x1_bwd_plan(rows, k, n, add)
            assert tuple(q[key] for key in KEYS) == (bwd[add],) + bwd[2:]
            assert q["eligible"]
