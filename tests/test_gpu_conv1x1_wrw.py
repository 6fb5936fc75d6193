"""The native backward-weights GEMM of the 1x1 convolution (conv1x1_wrw and
conv1x1_wrw_finalize in csrc/conv1x1_kernels.hip), against fp64 and against
the stock weight gradient.

Error budget.  dW[n, k] is bf16 of an fp32-accumulated sum of R products:
|err| <= 2^-8 |ref| + (R+1) 2^-24 sum_r |dy x|, the first term the one
rounding, the second R fp32 additions in any order.  MIOpen's weight gradient
is the yardstick as in test_gpu_conv1x1_bwd.py: the native error may be at
most 1.5x its error.
"""

import copy
import functools

import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

from torch_cgx_amd import _C  # noqa: E402
from torch_cgx_amd.models.resnet import Bottleneck  # noqa: E402
from torch_cgx_amd.ops import fused_bn  # noqa: E402

# (batch, K of X, N of dY, H, W, max_workgroups)
SHAPES = [(2, 64, 64, 1, 1, 0), (2, 256, 64, 7, 7, 0), (3, 64, 256, 5, 5, 0),
          (2, 128, 256, 5, 5, 0), (2, 512, 128, 8, 8, 0),
          (2, 512, 2048, 3, 3, 0), (2, 2048, 512, 3, 3, 0),
          (2, 256, 64, 56, 56, 0), (2, 256, 64, 28, 28, 3),
          # the tiles the shapes above leave out
          (2, 64, 256, 5, 5, 0), (2, 256, 64, 5, 5, 0)]
TAILS = SHAPES[:4]
U = 2.0 ** -24


def _ids(s):
    return "{}x{}to{}x{}x{}-wg{}".format(*s)


def _bf16_cl(t):
    return t.bfloat16().cuda().contiguous(memory_format=torch.channels_last)


def _rows(t):
    """[N,C,H,W] -> fp64 CPU [R, C]"""
    return t.detach().double().cpu().permute(0, 2, 3, 1).reshape(
        -1, t.shape[1])


def _errors(got, want):
    d = got - want
    return d.abs().max().item(), (d.norm() / want.norm().clamp_min(1e-300)).item()


def _stock_dw(dy, x):
    w = torch.empty(dy.shape[1], x.shape[1], 1, 1, dtype=dy.dtype,
                    device=dy.device)
    return torch.ops.aten.convolution_backward(
        dy, x, w, None, (1, 1), (0, 0), (1, 1), False, (0, 0), 1,
        (False, True, False))[1]


def _bits(t):
    return t.contiguous().view(torch.int16)


def _operands(shape):
    b, k, n, h, w, _ = shape
    g = torch.Generator().manual_seed(k * 7 + n * 3 + h)
    dy = _bf16_cl(torch.randn(b, n, h, w, generator=g) * (
        0.5 + torch.rand(1, n, 1, 1, generator=g)))
    x = _bf16_cl(torch.randn(b, k, h, w, generator=g))
    return dy, x


@functools.lru_cache(maxsize=None)
def _run(shape):
    wg = shape[5]
    dy, x = _operands(shape)
    keep = dy.clone(), x.clone()
    got = dict(dw=_C.conv1x1_wrw(dy, x, wg), dw2=_C.conv1x1_wrw(dy, x, wg),
               stock=_stock_dw(dy, x))
    torch.cuda.synchronize()
    got["inputs_unchanged"] = (torch.equal(_bits(dy), _bits(keep[0]))
                               and torch.equal(_bits(x), _bits(keep[1])))
    dy64, x64 = _rows(dy), _rows(x)
    ref = dict(dw=dy64.t() @ x64, mag=dy64.abs().t() @ x64.abs())
    return got, ref


def _plan(shape):
    b, k, n, h, w, wg = shape
    return _C.conv1x1_wrw_plan(b * h * w, k, n, wg)


def _bound(ref, rows):
    return 2.0 ** -8 * ref["dw"].abs() + (rows + 1) * U * ref["mag"]


def test_shapes_reach_every_instantiation():
    seen = set()
    for s in SHAPES:
        p = _plan(s)
        assert p["eligible"]
        seen.add((p["bn"], p["bk"]))
    # every pair the launcher instantiates: all of {64, 128, 256}^2 but 256x256
    assert seen == {(bn, bk) for bn in (64, 128, 256) for bk in (64, 128, 256)
                    } - {(256, 256)}
    assert _plan(SHAPES[0])["row_chunks"] == 1               # two rows
    assert _plan(SHAPES[1])["row_chunks"] == 2               # 64 + 34 rows
    assert _plan(SHAPES[2])["row_chunks"] == 2               # 64 + 11 rows
    assert _plan(SHAPES[4])["row_chunks"] == 2               # 128 rows, no tail
    for s in SHAPES[5:7]:
        p = _plan(s)
        assert p["ntiles_n"] * p["ntiles_k"] >= 32           # channel tiling
    assert _plan(SHAPES[7])["splits"] >= 8                   # many splits
    p = _plan(SHAPES[8])
    assert p["grid"] <= 3 and p["chunks_per_split"] >= 4


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_accuracy(shape):
    got, ref = _run(shape)
    b, k, n, h, w, _ = shape
    dw = got["dw"]
    assert tuple(dw.shape) == (n, k, 1, 1) and dw.dtype == torch.bfloat16
    # dense as the stock weight gradient is: AccumulateGrad takes it as it is
    assert tuple(got["stock"].shape) == (n, k, 1, 1)
    assert dw.is_contiguous() and got["stock"].is_contiguous()
    assert dw.is_contiguous(memory_format=torch.channels_last)
    err = (dw.double().cpu().reshape(n, k) - ref["dw"]).abs()
    bound = _bound(ref, b * h * w)
    worst = (err / bound.clamp_min(1e-300)).max().item()
    print(f"worst error / bound {worst:.3f}")
    assert bool((err <= bound).all())


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_against_stock(shape):
    got, ref = _run(shape)
    n, k = ref["dw"].shape
    a_abs, a_l2 = _errors(got["dw"].double().cpu().reshape(n, k), ref["dw"])
    b_abs, b_l2 = _errors(got["stock"].double().cpu().reshape(n, k), ref["dw"])
    msg = (f"native max-abs {a_abs:.3e} rel-L2 {a_l2:.3e}; stock max-abs "
           f"{b_abs:.3e} rel-L2 {b_l2:.3e}")
    print(msg)
    assert a_abs <= 1.5 * b_abs, msg
    assert a_l2 <= 1.5 * b_l2, msg


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_reproducible_and_inputs_untouched(shape):
    got, _ = _run(shape)
    assert not bool(got["dw"].isnan().any())
    assert torch.equal(_bits(got["dw"]), _bits(got["dw2"]))
    assert got["inputs_unchanged"]


def _in_poisoned_buffer(t):
    """The same tensor as a view into a buffer whose following rows, more
    than two chunks of them, are NaN."""
    b, c, h, w = t.shape
    rows = b * h * w
    big = torch.full((rows + 160, c), float("nan"), dtype=t.dtype,
                     device=t.device)
    view = big[:rows].view(b, h, w, c).permute(0, 3, 1, 2)
    view.copy_(t)
    return big, view


@pytest.mark.parametrize("shape", TAILS, ids=_ids)
def test_rows_past_the_end_are_not_read_into_the_sum(shape):
    got, _ = _run(shape)
    dy, x = _operands(shape)
    big_dy, vdy = _in_poisoned_buffer(dy)
    big_x, vx = _in_poisoned_buffer(x)
    assert _C.conv1x1_wrw_eligible(vdy, vx)
    assert bool(big_dy[-1].isnan().all()) and bool(big_x[-1].isnan().all())
    dw = _C.conv1x1_wrw(vdy, vx, shape[5])
    assert bool(dw.isfinite().all())
    assert torch.equal(_bits(dw), _bits(got["dw"]))


def test_rejects_what_it_cannot_take():
    dy = _bf16_cl(torch.randn(2, 64, 4, 4))
    x = _bf16_cl(torch.randn(2, 128, 4, 4))
    assert _C.conv1x1_wrw_eligible(dy, x)
    bad = [(dy.float(), x), (dy, x.float()), (dy.contiguous(), x),
           (dy, x.contiguous()), (dy, x[:1]), (dy[:, :32], x),
           (dy, _bf16_cl(torch.randn(2, 128, 4, 5))),
           (dy, _bf16_cl(torch.randn(2, 32, 4, 4))),
           (dy, _bf16_cl(torch.randn(2, 96, 4, 4))),
           (_bf16_cl(torch.randn(1, 64, 1, 1)),
            _bf16_cl(torch.randn(1, 128, 1, 1))),
           (dy.cpu(), x.cpu())]
    for args in bad:
        assert not _C.conv1x1_wrw_eligible(*args)
        with pytest.raises(RuntimeError):
            _C.conv1x1_wrw(*args)
    with pytest.raises(RuntimeError):
        _C.conv1x1_wrw(dy, x, -1)


# ---- through the modules ------------------------------------------------------


def _block():
    torch.manual_seed(3)
    blk = Bottleneck(256, 64)
    with torch.no_grad():
        for m in blk.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.weight.normal_(1.0, 0.2)
                m.bias.normal_(0.0, 0.2)
    return blk


def _train_step(blk, x, dy, mode, monkeypatch):
    monkeypatch.setenv("CGX_NATIVE_CONV1X1_WRW", mode)
    blk = copy.deepcopy(blk).cuda().to(memory_format=torch.channels_last)
    x = x.clone().requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out = blk(x)
    out.backward(dy)
    torch.cuda.synchronize()
    return blk


def test_bottleneck_routes_the_weight_gradients(monkeypatch):
    """CGX_NATIVE_CONV1X1_WRW=all sends both 1x1 weight gradients of a
    bottleneck through the kernel; =0 leaves the stock calls, whose output
    becomes the gradient bit for bit.

    Both runs go through the autograd functions of fused_bn (forward and
    backward-data native), so that the operands of every weight gradient can
    be recorded.  A weight gradient feeds nothing else in the backward, but
    MIOpen's backward-data of the 3x3 convolution between the two does not
    give the same bits every run; so each run's gradients are held against
    the fp64 product of that run's own operands; conv3's operands, which the
    backward reaches before the 3x3, are the same bits in both runs."""
    monkeypatch.setenv("CGX_NATIVE_CONV1X1", "all")
    monkeypatch.setenv("CGX_NATIVE_CONV1X1_BWD", "all")
    native, seen, stock_calls = [], [], []
    real, real_dw = _C.conv1x1_wrw, fused_bn._conv1x1_dw
    real_bw = fused_bn._conv1x1_backward

    def spy_bw(dy, x, weight, mask):
        out = real_bw(dy, x, weight, mask)
        if tuple(mask) == (False, True, False):
            stock_calls.append((dy, x, out[1]))
        return out

    def spy(dy, x, max_workgroups=0):
        native.append(tuple(dy.shape))
        return real(dy, x, max_workgroups)

    def spy_dw(dy, x, weight):
        dw = real_dw(dy, x, weight)
        seen.append((dy, x, dw))
        return dw

    monkeypatch.setattr(fused_bn._C, "conv1x1_wrw", spy)
    monkeypatch.setattr(fused_bn, "_conv1x1_dw", spy_dw)
    monkeypatch.setattr(fused_bn, "_conv1x1_backward", spy_bw)
    blk = _block()
    g = torch.Generator().manual_seed(17)
    x = _bf16_cl(torch.randn(4, 256, 12, 12, generator=g))
    dy = _bf16_cl(torch.randn(4, 256, 12, 12, generator=g))
    rows = 4 * 12 * 12
    on = _train_step(blk, x, dy, "all", monkeypatch)
    assert len(native) == 2 and len(seen) == 2 and not stock_calls
    off = _train_step(blk, x, dy, "0", monkeypatch)
    assert len(native) == 2 and len(seen) == 4 and len(stock_calls) == 2
    runs = {}
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
            runs[conv, which] = (cdy, cx, grad, bound, ref["dw"])
            if which == "0":
                # the output of the stock call on these very operands, bit
                # for bit; a second stock call sums in another order and
                # need not give the same bits, only stay within the bounds
                direct = [c for c in stock_calls if c[0] is cdy and c[1] is cx]
                assert len(direct) == 1
                assert torch.equal(grad, direct[0][2].float()), conv
                again = _stock_dw(cdy, cx).double().cpu().reshape(n, k)
                assert bool(((again - grad.double().cpu().reshape(n, k)).abs()
                             <= 2 * bound).all()), conv
    # the two runs against each other: within the two bounds, plus, where
    # the operands differ, the exact difference that makes
    for conv in ("conv1", "conv3"):
        a, b = runs[conv, "all"], runs[conv, "0"]
        same = torch.equal(_bits(a[0]), _bits(b[0])) and torch.equal(
            _bits(a[1]), _bits(b[1]))
        assert same or conv != "conv3"
        n, k = a[2].shape[:2]
        diff = (a[2] - b[2]).abs().double().cpu().reshape(n, k)
        allowed = a[3] + b[3] + (a[4] - b[4]).abs()
        print(f"{conv}: same operands {same}, worst difference / allowed "
              f"{(diff / allowed.clamp_min(1e-300)).max().item():.3f}")
        assert bool((diff <= allowed).all()), conv


def test_switched_off_with_the_forward_switch(monkeypatch):
    monkeypatch.setenv("CGX_NATIVE_CONV1X1_WRW", "all")
    assert fused_bn.native_conv1x1_wrw_mode() == "all"
    monkeypatch.setenv("CGX_NATIVE_CONV1X1", "0")
    assert fused_bn.native_conv1x1_wrw_mode() == "0"
    monkeypatch.delenv("CGX_NATIVE_CONV1X1")
    monkeypatch.setenv("CGX_FUSED_BN", "0")
    assert fused_bn.native_conv1x1_wrw_mode() == "0"
