"""conv1x1s2_plan (csrc/conv1x1_plan.h): eligibility, the tile walk and the
addresses the kernel's loads direct to LDS read, replayed on the host."""

import numpy as np
import pytest
import torch

from torch_cgx_amd import _C

# (batch, H, W, K, N): the three downsample convolutions of ResNet-50
RESNET = [(256, 56, 56, 256, 512), (256, 28, 28, 512, 1024),
          (256, 14, 14, 1024, 2048)]


def test_eligibility_at_the_limits():
    ok = [(2, 1, 1, 64, 256), (1, 3, 2, 2048, 2048), (2, 5, 7, 64, 256),
          (1, 8192, 8192, 64, 256), (1, 4096, 4096, 512, 256)]
    bad = [(1, 1, 1, 64, 256), (2, 0, 4, 64, 256), (2, 4, 0, 64, 256),
           (2, 4, 4, 32, 256), (2, 4, 4, 96, 256), (2, 4, 4, 4096, 256),
           (2, 4, 4, 64, 128), (2, 4, 4, 64, 384), (2, 4, 4, 64, 4096),
           (1, 8194, 8192, 64, 256),    # R above 2^24
           (1, 4096, 4096, 1024, 256)]  # X's 2^31 vectors do not fit an int
    assert all(_C.conv1x1s2_plan(*s)["eligible"] for s in ok)
    for s in bad:
        assert not _C.conv1x1s2_plan(*s)["eligible"]
        assert not _C.conv1x1s2_plan(*s)["native"]
        with pytest.raises(RuntimeError):
            _C.conv1x1s2_walk(*s)
    p = _C.conv1x1s2_plan(2, 5, 7, 64, 256)
    assert (p["ho"], p["wo"], p["rows"]) == (3, 4, 24)


@pytest.mark.parametrize("shape", RESNET)
def test_resnet_problems(shape):
    b, h, w, k, n = shape
    p = _C.conv1x1s2_plan(*shape)
    assert p["eligible"] and p["rows"] == b * (h // 2) * (w // 2)
    assert (p["tile_rows"], p["tile_channels"], p["k_chunk"]) == (256, 256, 64)
    assert p["k_chunks"] == k // 64 and p["stage_bytes"] == 2 * 256 * 64 * 2
    assert p["lds_bytes"] == 2 * p["stage_bytes"] + 16384 <= 160 * 1024
    # the final merge reuses the ring: 12 rows of 256 floats and 4 counts
    assert (12 * 256 + 4) * 4 <= 2 * p["stage_bytes"]
    assert p["grid"] == p["ntiles"] * p["splits"] <= 256
    assert p["run"] == 64 * p["tiles_per_split"]
    assert p["pstride"] == 2 * n + p["ntiles"]
    assert 4 * p["partial_floats"] <= 0.05 * 2 * p["rows"] * n
    assert _C.conv1x1s2_plan(*shape, 256)["grid"] <= 256
    assert _C.conv1x1s2_plan(*shape, 100)["grid"] <= 100
    # kNativeFwd1x1S2 (csrc/conv1x1_plan.cc): measured at batch 256 only
    assert p["native"] and not _C.conv1x1s2_plan(b // 2, h, w, k, n)["native"]
    assert not _C.conv1x1s2_plan(b, h - 1, w, k, n)["native"]


@pytest.mark.parametrize("shape", RESNET + [(3, 20, 20, 256, 512),
                                            (16, 28, 28, 128, 512)])
@pytest.mark.parametrize("cap", [0, 6])
def test_walk_visits_every_tile_once(shape, cap):
    p = _C.conv1x1s2_plan(*shape, cap)
    walk = _C.conv1x1s2_walk(*shape, cap)
    assert tuple(walk.shape) == (p["grid"], p["tiles_per_split"], 4)
    live = walk[..., 0] >= 0
    assert bool(live[:, 0].all()) and bool((live[:, 1:] <= live[:, :-1]).all())
    r0, r1, n0, n1 = walk[live].unbind(1)
    assert bool((r1 == torch.clamp(r0 + 256, max=p["rows"])).all())
    assert bool((r0 % 256 == 0).all()) and bool((n1 - n0 == 256).all())
    key = (r0 // 256) * p["ntiles"] + n0 // 256
    assert torch.equal(key.sort().values,
                       torch.arange(p["row_tiles"] * p["ntiles"]))


@pytest.mark.parametrize("shape,tile", [((3, 5, 7, 64, 256), 0),
                                        ((5, 32, 32, 64, 256), 3),
                                        ((3, 20, 20, 256, 512), 1),
                                        ((256, 14, 14, 1024, 2048), 48)])
def test_loads_fill_the_image_the_operand_reads_expect(shape, tile):
    b, h, w, _, _ = shape
    ho, wo = (h + 1) // 2, (w + 1) // 2
    row, vec, pixel = _C.conv1x1s2_source(*shape, tile).numpy().T
    # every (row, vector) once, at w_slot<64>(row, vec) of the kernels
    assert sorted(zip(row, vec)) == [(r, q) for r in range(256)
                                     for q in range(8)]
    assert np.array_equal(np.arange(2048), row * 8 + (vec ^ ((row >> 1) & 7)))
    # the gathered pixel; rows past R read row R - 1
    r = np.minimum(tile * 256 + row, b * ho * wo - 1)
    img, oh, ow = r // (ho * wo), r // wo % ho, r % wo
    assert np.array_equal(pixel, (img * h + 2 * oh) * w + 2 * ow)
