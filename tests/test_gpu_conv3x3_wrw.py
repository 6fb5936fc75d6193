"""The native weight gradient of the 3x3 / stride 1 / padding 1 convolution
(conv3x3_wrw in csrc/conv3x3_kernels.hip), against fp64 and against the stock
weight gradient.

Error budget, as in test_gpu_conv1x1_wrw.py: |err| <= 2^-8 |ref| +
(R+1) 2^-24 mag, one rounding plus R = B*H*W fp32 additions in any order, mag
the same sum over absolute values; the zero pads add exact zeros.  The native
error may be at most 1.5x that of MIOpen's weight gradient.
"""

import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from torch_cgx_amd import _C  # noqa: E402
from torch_cgx_amd.models.resnet import Bottleneck  # noqa: E402
from torch_cgx_amd.ops import fused_bn  # noqa: E402


def _short_last_chunk_height(w):
    """The smallest H cut into two or more chunks, the last one short."""
    for h in range(2, 512):
        p = _C.conv3x3_wrw_plan(2, h, w, 64, 64)
        if p["chunks_per_image"] >= 2 and h % p["hr"]:
            return h
    raise AssertionError("no such height")


# (batch, C of X, N of dY, H, W, max_workgroups)
SHAPES = [(1, 64, 64, 1, 1, 0), (2, 64, 64, 3, 5, 0), (2, 128, 64, 7, 7, 0),
          (3, 64, 128, 7, 7, 0), (2, 64, 64, _short_last_chunk_height(56), 56, 0),
          (2, 256, 256, 14, 14, 0), (2, 512, 512, 7, 7, 0),
          (2, 64, 64, 12, 12, 3),
          # several splits: a multiple of 8 over two tiles, the same capped to
          # three, and groups of images with the last one partly filled
          (64, 128, 64, 14, 14, 0), (64, 128, 64, 14, 14, 7),
          (100, 64, 64, 7, 7, 0)]
BORDERS = SHAPES[:4]
U = 2.0 ** -24


def _ids(s):
    return "{}x{}to{}x{}x{}-wg{}".format(*s)


def _bf16_cl(t):
    return t.bfloat16().cuda().contiguous(memory_format=torch.channels_last)


def _bits(t):
    return t.contiguous().view(torch.int16)


def _stock_dw(dy, x):
    w = torch.empty(dy.shape[1], x.shape[1], 3, 3, dtype=dy.dtype,
                    device=dy.device).contiguous(
                        memory_format=torch.channels_last)
    return torch.ops.aten.convolution_backward(
        dy, x, w, None, (1, 1), (1, 1), (1, 1), False, (0, 0), 1,
        (False, True, False))[1]


def _reference(dy, x):
    dy64, x64 = dy.detach().double().cpu(), x.detach().double().cpu()
    size = (dy.shape[1], x.shape[1], 3, 3)
    dw = torch.nn.grad.conv2d_weight(x64, size, dy64, padding=1)
    mag = torch.nn.grad.conv2d_weight(x64.abs(), size, dy64.abs(), padding=1)
    rows = dy.shape[0] * dy.shape[2] * dy.shape[3]
    return dict(dw=dw, bound=2.0 ** -8 * dw.abs() + (rows + 1) * U * mag)


def _operands(shape):
    b, c, n, h, w, _ = shape
    g = torch.Generator().manual_seed(c * 7 + n * 3 + h)
    dy = _bf16_cl(torch.randn(b, n, h, w, generator=g) * (
        0.5 + torch.rand(1, n, 1, 1, generator=g)))
    x = _bf16_cl(torch.randn(b, c, h, w, generator=g))
    return dy, x


@functools.lru_cache(maxsize=None)
def _run(shape):
    wg = shape[5]
    dy, x = _operands(shape)
    keep = dy.clone(), x.clone()
    got = dict(dw=_C.conv3x3_wrw(dy, x, wg), dw2=_C.conv3x3_wrw(dy, x, wg),
               stock=_stock_dw(dy, x))
    torch.cuda.synchronize()
    got["inputs_unchanged"] = (torch.equal(_bits(dy), _bits(keep[0]))
                               and torch.equal(_bits(x), _bits(keep[1])))
    return got, _reference(dy, x)


def _plan(shape):
    b, c, n, h, w, wg = shape
    return _C.conv3x3_wrw_plan(b, h, w, c, n, wg)


def test_shapes_reach_the_plans_they_are_for():
    plans = [_plan(s) for s in SHAPES]
    assert all(p["eligible"] for p in plans)
    # every pair the launcher instantiates; both LDS images are 64 wide
    assert {(p["bn"], p["bk"]) for p in plans} == {(64, 64)}
    assert plans[1]["chunks_per_image"] == 1
    assert plans[4]["chunks_per_image"] >= 2                 # short last chunk
    assert SHAPES[4][3] % plans[4]["hr"] != 0
    assert plans[2]["images"] == 2 and plans[3]["images"] == 3  # odd batch
    assert plans[5]["ntiles_n"] * plans[5]["ntiles_k"] == 16  # channel tiling
    assert plans[6]["ntiles_n"] * plans[6]["ntiles_k"] == 64
    assert plans[7]["grid"] <= 3
    assert plans[8]["splits"] == 8 and plans[8]["grid"] == 16
    assert plans[9]["splits"] == 3 and plans[9]["grid"] == 6
    assert plans[9]["chunks_per_split"] >= 8                 # long walks
    assert plans[10]["splits"] == 4 and 100 % plans[10]["images"]


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_accuracy(shape):
    got, ref = _run(shape)
    _, c, n, _, _, _ = shape
    dw = got["dw"]
    assert tuple(dw.shape) == (n, c, 3, 3) and dw.dtype == torch.bfloat16
    assert dw.is_contiguous(memory_format=torch.channels_last)
    err = (dw.double().cpu() - ref["dw"]).abs()
    worst = (err / ref["bound"].clamp_min(1e-300)).max().item()
    print(f"worst error / bound {worst:.3f}")
    assert bool((err <= ref["bound"]).all())
    # reproducible, inputs untouched
    assert not bool(dw.isnan().any())
    assert torch.equal(_bits(dw), _bits(got["dw2"]))
    assert got["inputs_unchanged"]


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_against_stock(shape):
    got, ref = _run(shape)

    def errors(t):
        d = t.double().cpu() - ref["dw"]
        return d.abs().max().item(), (d.norm() / ref["dw"].norm()).item()

    (a_abs, a_l2), (b_abs, b_l2) = errors(got["dw"]), errors(got["stock"])
    msg = (f"native max-abs {a_abs:.3e} rel-L2 {a_l2:.3e}; stock max-abs "
           f"{b_abs:.3e} rel-L2 {b_l2:.3e}")
    print(msg)
    assert a_abs <= 1.5 * b_abs, msg
    assert a_l2 <= 1.5 * b_l2, msg


def _in_poisoned_buffer(t):
    """The tensor as a view into a buffer with NaN rows before and after."""
    b, c, h, w = t.shape
    rows, pad = b * h * w, 640
    big = torch.full((rows + 2 * pad, c), float("nan"), dtype=t.dtype,
                     device=t.device)
    view = big[pad:pad + rows].view(b, h, w, c).permute(0, 3, 1, 2)
    view.copy_(t)
    return big, view


@pytest.mark.parametrize("shape", BORDERS, ids=_ids)
def test_nothing_outside_the_images_reaches_the_sum(shape):
    got, _ = _run(shape)
    dy, x = _operands(shape)
    big_dy, vdy = _in_poisoned_buffer(dy)
    big_x, vx = _in_poisoned_buffer(x)
    assert _C.conv3x3_wrw_eligible(vdy, vx)
    for big in (big_dy, big_x):
        assert bool(big[0].isnan().all()) and bool(big[-1].isnan().all())
    dw = _C.conv3x3_wrw(vdy, vx, shape[5])
    assert bool(dw.isfinite().all())
    assert torch.equal(_bits(dw), _bits(got["dw"]))


def test_rejects_what_it_cannot_take():
    dy = _bf16_cl(torch.randn(2, 64, 4, 4))
    x = _bf16_cl(torch.randn(2, 128, 4, 4))
    assert _C.conv3x3_wrw_eligible(dy, x)
    bad = [(dy.float(), x), (dy, x.float()), (dy.contiguous(), x),
           (dy, x.contiguous()), (dy, x[:1]),
           (dy, _bf16_cl(torch.randn(2, 128, 4, 5))),
           (dy, _bf16_cl(torch.randn(2, 128, 5, 4))),
           (dy, _bf16_cl(torch.randn(2, 32, 4, 4))),
           (dy, _bf16_cl(torch.randn(2, 96, 4, 4))),
           (dy, _bf16_cl(torch.randn(2, 1024, 4, 4))),
           (_bf16_cl(torch.randn(2, 1024, 4, 4)), x),
           (dy.cpu(), x.cpu())]
    for args in bad:
        assert not _C.conv3x3_wrw_eligible(*args)
        with pytest.raises(RuntimeError):
            _C.conv3x3_wrw(*args)
    with pytest.raises(RuntimeError):
        _C.conv3x3_wrw(dy, x, -1)


def _train_step(mode, monkeypatch):
    """One step of a Bottleneck(256, 64) under bf16 autocast -> (block, the
    (dy, x, dw) of every call of the kernel)."""
    monkeypatch.setenv("CGX_NATIVE_CONV3X3_WRW", mode)
    calls, real = [], _C.conv3x3_wrw

    def spy(dy, x, max_workgroups=0):
        calls.append((dy, x, real(dy, x, max_workgroups)))
        return calls[-1][2]

    monkeypatch.setattr(fused_bn._C, "conv3x3_wrw", spy)
    torch.manual_seed(3)
    blk = Bottleneck(256, 64).cuda().to(memory_format=torch.channels_last)
    g = torch.Generator().manual_seed(17)
    x = _bf16_cl(torch.randn(4, 256, 12, 12, generator=g)).requires_grad_(True)
    dy = _bf16_cl(torch.randn(4, 256, 12, 12, generator=g))
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out = blk(x)
    out.backward(dy)
    torch.cuda.synchronize()
    return blk, calls


def test_bottleneck_routes_the_weight_gradient(monkeypatch):
    blk, calls = _train_step("all", monkeypatch)
    assert len(calls) == 1
    cdy, cx, dw = calls[0]
    grad = blk.conv2.weight.grad
    assert grad.dtype == torch.float32 and grad.shape == blk.conv2.weight.shape
    assert dw.dtype == torch.bfloat16 and torch.equal(grad, dw.float())
    ref = _reference(cdy, cx)
    assert bool(((grad.double().cpu() - ref["dw"]).abs() <= ref["bound"]).all())


def test_switched_off(monkeypatch):
    blk, calls = _train_step("0", monkeypatch)
    assert not calls and blk.conv2.weight.grad is not None
    monkeypatch.setenv("CGX_NATIVE_CONV3X3_WRW", "all")
    monkeypatch.setenv("CGX_NATIVE_CONV1X1", "0")
    assert fused_bn.native_conv3x3_wrw_mode() == "all"
    monkeypatch.setenv("CGX_FUSED_BN", "0")
    assert fused_bn.native_conv3x3_wrw_mode() == "0"
    monkeypatch.delenv("CGX_FUSED_BN")
    monkeypatch.setenv("CGX_NATIVE_CONV3X3_WRW", "1")
    monkeypatch.setenv("CGX_NATIVE_CONV1X1", "all")
    assert fused_bn.native_conv3x3_wrw_mode() == "1"
