"""Launch geometry and address maps of the ring backward-weights GEMM
(conv1x1_wrw_ring_plan, conv1x1_wrw_image_slot, conv1x1_wrw_ring_piece and
conv1x1_wrw_ring_lds_base in csrc/conv1x1_plan.h): a stage of the ring is
filled by loads that write LDS lane-linearly, so the permutation of the
image's cells sits on the address each lane loads from.  The kernel calls
these functions; the tests replay them."""

import pytest
import torch

from torch_cgx_amd import _C

# (K, N, image side): the twelve stride-1 1x1 problems of the ResNet-50
# benchmark at batch 256 ...
PROBLEMS = [(64, 64, 56), (64, 256, 56), (256, 64, 56), (256, 128, 56),
            (128, 512, 28), (512, 128, 28), (512, 256, 28), (256, 1024, 14),
            (1024, 256, 14), (1024, 512, 14), (512, 2048, 7), (2048, 512, 7)]
BENCH = [(256 * hw * hw, k, n, 0) for k, n, hw in PROBLEMS]
# ... capped, and (rows, K, N, max_workgroups) of
# tests/test_gpu_conv1x1_wrw_ring.py, with others at the limits of the plan
SMALL = [(2, 128, 128, 0), (192, 128, 128, 1), (800, 128, 128, 1),
         (512, 256, 128, 2), (512, 128, 256, 2), (18, 512, 2048, 0),
         (18, 2048, 512, 0), (392, 1024, 256, 0), (512, 128, 128, 2),
         (640, 128, 128, 2),
         (129, 2048, 2048, 0), (64, 128, 128, 0), (65, 128, 128, 0),
         (12544, 2048, 512, 5), (50176, 256, 1024, 100),
         (200704, 512, 256, 1), (1 << 20, 128, 128, 0)]
SHAPES = [s for s in BENCH if min(s[1], s[2]) >= 128] + SMALL
LDS_LIMIT = 160 * 1024
WAVES = 4


def _id(s):
    return "R{}-k{}-n{}-wg{}".format(*s)


def _cell(c, r, u):
    """wrw_cell<C>(r, u) of csrc/conv1x1_kernels.hip"""
    lin = r * (c // 32) + u
    swz = (r >> 1) & 1 if c == 64 else r & 3
    return 256 * (lin >> 2) + 64 * ((lin & 3) ^ swz)


@pytest.mark.parametrize("c", [64, 128, 256])
def test_the_loads_of_a_stage_fill_the_image_of_wrw_cell(c):
    # vector q (eight channels) of row r sits at wrw_cell(r, q >> 2) + 16*(q & 3)
    want = {_cell(c, r, q >> 2) + 16 * (q & 3): (r, 8 * q)
            for r in range(64) for q in range(c // 8)}
    assert sorted(want) == list(range(0, 64 * c * 2, 16))
    got = {}
    for wave in range(WAVES):
        for j in range(64 * c // 2048):
            piece = _C.conv1x1_wrw_ring_piece(wave, j)
            assert piece % 1024 == 0
            for lane in range(64):
                p = piece + 16 * lane   # where the hardware puts the lane
                assert p not in got
                got[p] = _C.conv1x1_wrw_image_slot(c, p)
    assert got == want
    # whole 128- or 256-byte pieces of a row per group of 8 or 16 lanes, and
    # every row inside the chunk
    seg = min(c * 2, 256) // 16
    for p0 in range(0, 64 * c * 2, 16 * seg):
        run = [got[p0 + 16 * i] for i in range(seg)]
        assert len({r for r, _ in run}) == 1
        chans = sorted(ch for _, ch in run)
        assert chans == list(range(chans[0], chans[0] + 8 * seg, 8))
        assert chans[0] % (8 * seg) == 0
    assert all(0 <= r < 64 and 0 <= ch < c for r, ch in got.values())


@pytest.mark.parametrize("shape", [(800, 128, 128), (50176, 1024, 512)],
                         ids=lambda s: "R{}-k{}-n{}".format(*s))
def test_the_stages_tile_lds(shape):
    rows, k, n = shape
    p = _C.conv1x1_wrw_ring_plan(rows, k, n)
    assert p["lds_bytes"] <= LDS_LIMIT
    seen = set()
    for slot in range(p["stages"]):
        fill = _C.conv1x1_wrw_ring_fill(rows, k, n, slot)
        most = 64 * max(p["bn"], p["bk"]) // 2048
        assert tuple(fill.shape) == (2, WAVES, most, 64, 3)
        for op, c in enumerate((p["bn"], p["bk"])):
            mine = fill[op, :, :64 * c // 2048].reshape(-1, 3)
            assert bool((fill[op, :, 64 * c // 2048:] == -1).all())
            lds, row, chan = mine.unbind(1)
            # the operand's image inside the stage, in the image's own order
            base = slot * p["stage_bytes"] + (64 * p["bn"] * 2 if op else 0)
            assert bool((lds >= base).all())
            assert bool((lds + 16 <= base + 64 * c * 2).all())
            for a, r, ch in mine.tolist():
                assert _C.conv1x1_wrw_image_slot(c, a - base) == (r, ch)
            assert bool((row >= 0).all()) and bool((row < 64).all())
            assert bool((chan >= 0).all()) and bool((chan + 8 <= c).all())
            seen.update(lds.tolist())
        # lane-linear from a base the wave shares
        lanes = fill[..., 0]
        live = lanes[..., 0] >= 0
        step = lanes[..., 1:] - lanes[..., :-1]
        assert bool((step[live] == 16).all())
        assert bool((lanes[..., 0][live] % 1024 == 0).all())
    assert sorted(seen) == list(range(0, p["lds_bytes"], 16))
    with pytest.raises(RuntimeError):
        _C.conv1x1_wrw_ring_fill(rows, k, n, p["stages"])


@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_geometry(shape):
    rows, k, n, max_wg = shape
    p = _C.conv1x1_wrw_ring_plan(rows, k, n, max_wg)
    assert p["eligible"]
    assert p["threads"] == 256 and p["chunk_rows"] == 64
    assert (p["bn"], p["bk"]) == (128, 128)
    assert p["bn"] * p["ntiles_n"] == n and p["bk"] * p["ntiles_k"] == k
    assert p["stage_bytes"] == 64 * (p["bn"] + p["bk"]) * 2
    assert p["stages"] == 4
    assert p["lds_bytes"] == p["stages"] * p["stage_bytes"] == 128 * 1024
    # no second workgroup fits beside one
    assert 2 * p["lds_bytes"] > LDS_LIMIT
    # the counted wait of the kernel: the loads of a wave for the younger
    # stages, within the six bits of vmcnt
    assert (p["stages"] - 1) * p["stage_bytes"] // 4096 < 64
    # a chunk staged through registers fits the ring
    assert p["lds_bytes"] >= 64 * (p["bn"] + p["bk"]) * 2
    assert p["row_chunks"] == -(-rows // 64)
    assert 1 <= p["splits"] <= p["row_chunks"]
    tiles = p["ntiles_n"] * p["ntiles_k"]
    assert p["grid"] == tiles * p["splits"]
    assert p["chunks_per_split"] == -(-p["row_chunks"] // p["splits"])
    assert p["partial_floats"] == p["splits"] * n * k
    if max_wg:
        assert p["grid"] <= max(max_wg, tiles)
    else:
        assert p["grid"] <= max(256, tiles)   # one workgroup per CU
        assert _C.conv1x1_wrw_ring_plan(rows, k, n, 1 << 30) == p


@pytest.mark.parametrize("shape", SHAPES, ids=_id)
def test_walk_visits_every_chunk_of_every_tile_once(shape):
    rows, k, n, max_wg = shape
    p = _C.conv1x1_wrw_ring_plan(rows, k, n, max_wg)
    walk = _C.conv1x1_wrw_ring_walk(rows, k, n, max_wg)
    assert tuple(walk.shape) == (p["grid"], p["chunks_per_split"], 5)
    live = walk[..., 0] >= 0
    assert bool(live[:, 0].all())  # no workgroup without rows
    assert bool((live[:, 1:] <= live[:, :-1]).all())
    n0, k0, split, r0, r1 = walk[live].unbind(1)
    assert bool((n0 % p["bn"] == 0).all()) and bool((n0 < n).all())
    assert bool((k0 % p["bk"] == 0).all()) and bool((k0 < k).all())
    assert bool((r0 % 64 == 0).all()) and bool((r0 < rows).all())
    assert bool((r1 == torch.clamp(r0 + 64, max=rows)).all())
    tiles = p["ntiles_n"] * p["ntiles_k"]
    tile = (n0 // p["bn"]) * p["ntiles_k"] + k0 // p["bk"]
    key = (r0 // 64) * tiles + tile
    assert key.numel() == p["row_chunks"] * tiles
    assert torch.equal(key.sort().values, torch.arange(key.numel()))
    # the chunk with rows past R, which the kernel stages through registers,
    # is the last of the workgroups that own it
    if rows % 64:
        short = (walk[..., 4] - walk[..., 3] < 64) & live
        assert int(short.sum()) == tiles
        last = live.sum(1) - 1
        assert bool(short[torch.arange(p["grid"]), last].sum() == tiles)
    owner = set()
    for wg in range(0, p["grid"], max(1, p["grid"] // 64)):
        mine = walk[wg][live[wg]]
        assert mine[:, :3].unique(dim=0).shape[0] == 1
        assert bool((mine[1:, 3] > mine[:-1, 3]).all())
        assert 0 <= int(mine[0, 2]) < p["splits"]
        owner.add(tuple(mine[0, :3].tolist()))
    assert len(owner) == len(range(0, p["grid"], max(1, p["grid"] // 64)))
    assert walk[:, 0, :3].unique(dim=0).shape[0] == p["grid"]


def test_workgroups_of_a_row_slice_are_eight_apart():
    checked = 0
    for rows, k, n, _ in SHAPES:
        p = _C.conv1x1_wrw_ring_plan(rows, k, n)
        if p["splits"] % 8:
            continue
        checked += 1
        split = _C.conv1x1_wrw_ring_walk(rows, k, n)[:, 0, 2]
        for s in range(0, p["splits"], max(1, p["splits"] // 5)):
            wgs = (split == s).nonzero().flatten()
            assert wgs.numel() == p["ntiles_n"] * p["ntiles_k"]
            assert (wgs % 8).unique().numel() == 1
    assert checked >= 4


@pytest.mark.parametrize("rows,k,n", [(1, 128, 128), (98, 64, 128),
                                      (98, 128, 64), (98, 96, 128),
                                      (98, 128, 4096), (98, 4096, 128),
                                      ((1 << 24) + 1, 128, 128),
                                      (98, 0, 128)])
def test_ineligible(rows, k, n):
    p = _C.conv1x1_wrw_ring_plan(rows, k, n)
    assert not p["eligible"] and not p["native"]
    with pytest.raises(RuntimeError):
        _C.conv1x1_wrw_ring_walk(rows, k, n)
    with pytest.raises(RuntimeError):
        _C.conv1x1_wrw_ring_fill(rows, k, n)


# (K, N) that met the rule of benchmarks/RESULTS.md against conv1x1_wrw: the
# slowest run of the ring faster than the fastest of conv1x1_wrw
NATIVE = {(k, n) for k, n, _ in PROBLEMS if min(k, n) >= 128}


def test_native_only_where_measured_faster():
    for rows, k, n, _ in BENCH:
        p = _C.conv1x1_wrw_ring_plan(rows, k, n)
        assert p["native"] == ((k, n) in NATIVE)
        assert p["eligible"] == (min(k, n) >= 128)
        assert not _C.conv1x1_wrw_ring_plan(rows // 2, k, n)["native"]
    for rows, k, n, max_wg in SMALL:
        if (rows, k, n, 0) not in BENCH:
            assert not _C.conv1x1_wrw_ring_plan(rows, k, n, max_wg)["native"]


# conv1x1_wrw_plan of the twelve problems, in the order of PROBLEMS, as the
# commit before conv1x1_wrw_ring_plan gave them
KEYS = ("native", "bn", "bk", "splits", "grid", "chunks_per_split",
        "lds_bytes")
TODAY = [
    (False, 64, 64, 1024, 1024, 13, 16384),
    (True, 256, 64, 512, 512, 25, 40960),
    (True, 64, 256, 512, 512, 25, 40960),
    (True, 128, 256, 256, 256, 49, 49152),
    (True, 256, 128, 128, 256, 25, 49152),
    (True, 128, 256, 128, 256, 25, 49152),
    (True, 128, 256, 64, 256, 49, 49152),
    (True, 128, 128, 24, 384, 33, 32768),
    (True, 128, 128, 24, 384, 33, 32768),
    (True, 128, 256, 16, 256, 49, 49152),
    (True, 128, 128, 3, 192, 66, 32768),
    (True, 128, 128, 3, 192, 66, 32768),
]


def test_conv1x1_wrw_plan_is_untouched():
    for (rows, k, n, _), want in zip(BENCH, TODAY):
        p = _C.conv1x1_wrw_plan(rows, k, n)
        assert tuple(p[key] for key in KEYS) == want
        assert p["eligible"] and "stages" not in p
