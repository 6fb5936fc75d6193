"""The backward-weights GEMM of the 1x1 convolution that loads its chunks
straight into a ring of LDS stages (conv1x1_wrw_ring in
csrc/conv1x1_kernels.hip), against fp64, against conv1x1_wrw bit for bit
where both split the rows alike, and through the modules.

Operands and the error bound are those of test_gpu_conv1x1_wrw.py:
|err| <= 2^-8 |ref| + (R+1) 2^-24 sum_r |dy x|.
"""

import copy
import functools

import pytest
import torch

from torch_cgx_amd import _C
from torch_cgx_amd.models.resnet import Bottleneck
from torch_cgx_amd.ops import fused_bn

from test_gpu_conv1x1_wrw import (_bf16_cl, _bits, _bound, _in_poisoned_buffer,
                                  _operands, _rows)

# (batch, K of X, N of dY, H, W, max_workgroups)
SHAPES = [
    (2, 128, 128, 1, 1, 0),      # one chunk of two rows: no stage of the ring
    (2, 128, 128, 8, 12, 1),     # 192 rows: three chunks, fewer than stages
    (2, 128, 128, 20, 20, 1),    # 800 rows: 12 chunks wrap the ring, 32 left
    # meant for 128 x 256 and 256 x 128 tiles, which measured no faster and
    # are not built: here two 128 x 128 tiles, eight chunks in one split
    (2, 256, 128, 16, 16, 2),
    (2, 128, 256, 16, 16, 2),
    (2, 512, 2048, 3, 3, 0),     # 64 channel tiles, 18 rows
    (2, 2048, 512, 3, 3, 0),
    (2, 1024, 256, 14, 14, 0),   # 392 rows: 7 chunks, 7 splits, 8-row tail
    # as many chunks a split as the ring has stages, and one more
    (2, 128, 128, 16, 16, 2),
    (2, 128, 128, 16, 20, 2),
]
TAILS = [SHAPES[0], SHAPES[2], SHAPES[7]]
WRAPS = SHAPES[2]
# every tile the launcher instantiates
TILES = {(128, 128)}


def _ids(s):
    return "{}x{}to{}x{}x{}-wg{}".format(*s)


def _plan(shape, ring=True):
    b, k, n, h, w, wg = shape
    plan = _C.conv1x1_wrw_ring_plan if ring else _C.conv1x1_wrw_plan
    return plan(b * h * w, k, n, wg)


def _same_split(shape):
    p, q = _plan(shape), _plan(shape, ring=False)
    return all(p[key] == q[key] for key in ("bn", "bk", "splits"))


def test_shapes_reach_every_instantiation_and_every_path():
    plans = [_plan(s) for s in SHAPES]
    assert all(p["eligible"] and p["stages"] == 4 for p in plans)
    assert {(p["bn"], p["bk"]) for p in plans} == TILES
    # walks shorter than the ring, as long, one longer, and many times as long
    walks = {p["chunks_per_split"] for p in plans}
    assert {1, 3, 4, 5, 13} <= walks
    assert {p["ntiles_n"] * p["ntiles_k"] for p in plans} >= {1, 2, 16, 64}
    assert _plan(SHAPES[0])["row_chunks"] == 1
    p = _plan(WRAPS)
    assert p["splits"] == 1 and p["row_chunks"] == 13 and 800 % 64 == 32
    assert 12 >= 3 * p["stages"]
    assert all((s[0] * s[3] * s[4]) % 64 for s in TAILS)
    p = _plan(SHAPES[7])
    assert p["row_chunks"] == 7 and p["splits"] > 1
    # where the two kernels must give the same bits
    same = [s for s in SHAPES if _same_split(s)]
    assert len(same) >= 4 and WRAPS in same


@functools.lru_cache(maxsize=None)
def _run(shape):
    wg = shape[5]
    dy, x = _operands(shape)
    keep = dy.clone(), x.clone()
    got = dict(dw=_C.conv1x1_wrw_ring(dy, x, wg),
               dw2=_C.conv1x1_wrw_ring(dy, x, wg),
               old=_C.conv1x1_wrw(dy, x, wg))
    torch.cuda.synchronize()
    got["inputs_unchanged"] = (torch.equal(_bits(dy), _bits(keep[0]))
                               and torch.equal(_bits(x), _bits(keep[1])))
    dy64, x64 = _rows(dy), _rows(x)
    ref = dict(dw=dy64.t() @ x64, mag=dy64.abs().t() @ x64.abs())
    return got, ref


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_accuracy(shape):
    got, ref = _run(shape)
    b, k, n, h, w, _ = shape
    dw = got["dw"]
    assert tuple(dw.shape) == (n, k, 1, 1) and dw.dtype == torch.bfloat16
    assert dw.is_contiguous()
    assert dw.is_contiguous(memory_format=torch.channels_last)
    err = (dw.double().cpu().reshape(n, k) - ref["dw"]).abs()
    bound = _bound(ref, b * h * w)
    worst = (err / bound.clamp_min(1e-300)).max().item()
    print(f"worst error / bound {worst:.3f}")
    assert bool((err <= bound).all())


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_the_bits_of_conv1x1_wrw_where_the_splits_agree(shape):
    got, _ = _run(shape)
    if _same_split(shape):
        assert torch.equal(_bits(got["dw"]), _bits(got["old"]))
    else:  # another order of the same sum
        assert tuple(got["dw"].shape) == tuple(got["old"].shape)


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_reproducible_and_inputs_untouched(shape):
    got, _ = _run(shape)
    assert not bool(got["dw"].isnan().any())
    assert torch.equal(_bits(got["dw"]), _bits(got["dw2"]))
    assert got["inputs_unchanged"]


@pytest.mark.gpu
@pytest.mark.parametrize("shape", TAILS, ids=_ids)
def test_rows_past_the_end_are_not_read_into_the_sum(shape):
    got, _ = _run(shape)
    dy, x = _operands(shape)
    big_dy, vdy = _in_poisoned_buffer(dy)
    big_x, vx = _in_poisoned_buffer(x)
    assert _C.conv1x1_wrw_ring_eligible(vdy, vx)
    assert bool(big_dy[-1].isnan().all()) and bool(big_x[-1].isnan().all())
    dw = _C.conv1x1_wrw_ring(vdy, vx, shape[5])
    assert bool(dw.isfinite().all())
    assert torch.equal(_bits(dw), _bits(got["dw"]))


@pytest.mark.gpu
def test_rejects_what_conv1x1_wrw_rejects():
    dy = _bf16_cl(torch.randn(2, 128, 4, 4))
    x = _bf16_cl(torch.randn(2, 256, 4, 4))
    assert _C.conv1x1_wrw_eligible(dy, x)
    assert _C.conv1x1_wrw_ring_eligible(dy, x)
    bad = [(dy.float(), x), (dy, x.float()), (dy.contiguous(), x),
           (dy, x.contiguous()), (dy, x[:1]), (dy[:, :32], x),
           (dy, _bf16_cl(torch.randn(2, 256, 4, 5))),
           (dy, _bf16_cl(torch.randn(2, 32, 4, 4))),
           (dy, _bf16_cl(torch.randn(2, 96, 4, 4))),
           (_bf16_cl(torch.randn(1, 128, 1, 1)),
            _bf16_cl(torch.randn(1, 256, 1, 1))),
           (dy.cpu(), x.cpu())]
    for args in bad:
        assert not _C.conv1x1_wrw_eligible(*args)
        assert not _C.conv1x1_wrw_ring_eligible(*args)
        with pytest.raises(RuntimeError):
            _C.conv1x1_wrw_ring(*args)
    with pytest.raises(RuntimeError):
        _C.conv1x1_wrw_ring(dy, x, -1)
    # and, having no tile for them, 64 channels on either side
    narrow = _bf16_cl(torch.randn(2, 64, 4, 4))
    for args in ((narrow, x), (dy, narrow)):
        assert _C.conv1x1_wrw_eligible(*args)
        assert not _C.conv1x1_wrw_ring_eligible(*args)
        with pytest.raises(RuntimeError):
            _C.conv1x1_wrw_ring(*args)


# ---- through the modules ------------------------------------------------------


def _train_step(blk, x, dy, mode, monkeypatch):
    monkeypatch.setenv("CGX_NATIVE_CONV1X1_WRW_RING", mode)
    blk = copy.deepcopy(blk).cuda().to(memory_format=torch.channels_last)
    x = x.clone().requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out = blk(x)
    out.backward(dy)
    torch.cuda.synchronize()
    return blk


@pytest.mark.gpu
def test_bottleneck_routes_the_weight_gradients(monkeypatch):
    """CGX_NATIVE_CONV1X1_WRW_RING=all sends both 1x1 weight gradients of a
    bottleneck through the ring, =0 neither (they go to conv1x1_wrw, which
    CGX_NATIVE_CONV1X1_WRW=all opens).  In both runs the gradient is the
    kernel's output as fp32, within the bound against the fp64 product of
    that run's own operands."""
    monkeypatch.setenv("CGX_NATIVE_CONV1X1", "all")
    monkeypatch.setenv("CGX_NATIVE_CONV1X1_BWD", "all")
    monkeypatch.setenv("CGX_NATIVE_CONV1X1_WRW", "all")
    ring, old, seen = [], [], []
    real_ring, real_old = _C.conv1x1_wrw_ring, _C.conv1x1_wrw
    real_dw = fused_bn._conv1x1_dw

    def spy_ring(dy, x, max_workgroups=0):
        ring.append(tuple(dy.shape))
        return real_ring(dy, x, max_workgroups)

    def spy_old(dy, x, max_workgroups=0):
        old.append(tuple(dy.shape))
        return real_old(dy, x, max_workgroups)

    def spy_dw(dy, x, weight):
        dw = real_dw(dy, x, weight)
        seen.append((dy, x, dw))
        return dw

    monkeypatch.setattr(fused_bn._C, "conv1x1_wrw_ring", spy_ring)
    monkeypatch.setattr(fused_bn._C, "conv1x1_wrw", spy_old)
    monkeypatch.setattr(fused_bn, "_conv1x1_dw", spy_dw)
    torch.manual_seed(3)
    blk = Bottleneck(1024, 256)
    g = torch.Generator().manual_seed(17)
    x = _bf16_cl(torch.randn(2, 1024, 14, 14, generator=g))
    dy = _bf16_cl(torch.randn(2, 1024, 14, 14, generator=g))
    rows = 2 * 14 * 14
    on = _train_step(blk, x, dy, "all", monkeypatch)
    assert len(ring) == 2 and not old and len(seen) == 2
    off = _train_step(blk, x, dy, "0", monkeypatch)
    assert len(ring) == 2 and len(old) == 2 and len(seen) == 4
    for which, blk_run, ops in (("all", on, seen[:2]), ("0", off, seen[2:])):
        by_shape = {tuple(dw.shape[:2]): (cdy, cx, dw) for cdy, cx, dw in ops}
        for conv in ("conv1", "conv3"):
            grad = getattr(blk_run, conv).weight.grad
            assert grad.dtype == torch.float32
            assert grad.shape == getattr(blk_run, conv).weight.shape
            cdy, cx, dw = by_shape[tuple(grad.shape[:2])]
            n, k = dw.shape[:2]
            assert dw.dtype == torch.bfloat16
            assert torch.equal(grad, dw.float())
            dy64, x64 = _rows(cdy), _rows(cx)
            ref = dict(dw=dy64.t() @ x64, mag=dy64.abs().t() @ x64.abs())
            bound = _bound(ref, rows)
            err = (grad.double().cpu().reshape(n, k) - ref["dw"]).abs()
            worst = (err / bound.clamp_min(1e-300)).max().item()
            print(f"{conv} {which}: worst error / bound {worst:.3f}")
            assert bool((err <= bound).all()), (conv, which)


def test_the_switch(monkeypatch):
    for name in ("CGX_FUSED_BN", "CGX_NATIVE_CONV1X1", "CGX_NATIVE_CONV1X1_WRW",
                 "CGX_NATIVE_CONV1X1_WRW_RING"):
        monkeypatch.delenv(name, raising=False)
    assert fused_bn.native_conv1x1_wrw_ring_mode() == "1"
    # "all" is not inherited ...
    monkeypatch.setenv("CGX_NATIVE_CONV1X1_WRW", "all")
    assert fused_bn.native_conv1x1_wrw_ring_mode() == "1"
    monkeypatch.setenv("CGX_NATIVE_CONV1X1_WRW_RING", "all")
    assert fused_bn.native_conv1x1_wrw_ring_mode() == "all"
    # ... but "0" is, from each switch above it
    for name in ("CGX_NATIVE_CONV1X1_WRW", "CGX_NATIVE_CONV1X1"):
        monkeypatch.setenv(name, "0")
        assert fused_bn.native_conv1x1_wrw_ring_mode() == "0"
        monkeypatch.delenv(name)
    monkeypatch.setenv("CGX_FUSED_BN", "0")
    assert fused_bn.native_conv1x1_wrw_ring_mode() == "0"
