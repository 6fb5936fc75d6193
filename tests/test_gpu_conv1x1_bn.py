"""The native 1x1 convolution that also produces the BatchNorm partials of its
output (csrc/conv1x1_kernels.hip), against fp64 and against the stock path.

Error budget.  Y is bf16 of an fp32-accumulated dot product of K terms:
|err| <= 2^-8 |ref| + (K+1) 2^-24 sum_k |x_k w_k|, the first term the final
rounding, the second K fp32 additions in any order.  MIOpen's convolution is
the yardstick as in test_gpu_fused_bn.py: the native error may be at most 1.5x
its error.  Statistics are sums of R terms, a sequential run of L terms per
lane followed by trees: |err| <= (L + log2(R/L) + 4) 2^-24 sum|terms| with L
the plan's per-lane run length, checked against fp64 statistics of the
kernel's own (rounded) output, which is what bn_apply normalises.
"""

import copy
import functools
import math

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from torch_cgx_amd import _C  # noqa: E402
from torch_cgx_amd.models.resnet import Bottleneck  # noqa: E402
from torch_cgx_amd.ops import fused_bn  # noqa: E402
from torch_cgx_amd.ops.fused_bn import bn_act, conv_bn_act  # noqa: E402

# (batch, K, N, H, W, max_workgroups)
SHAPES = [(2, 64, 64, 1, 1, 0), (2, 64, 256, 7, 7, 0), (3, 256, 64, 5, 5, 0),
          (2, 128, 512, 9, 9, 0), (2, 2048, 512, 3, 3, 0),
          (2, 512, 2048, 3, 3, 0), (2, 64, 256, 56, 56, 0),
          (2, 64, 256, 28, 28, 3)]
MOMENTUM, EPS = 0.1, 1e-5
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


def _inputs(shape, offset=False):
    b, k, n, h, w, _ = shape
    g = torch.Generator().manual_seed(k * 7 + n * 3 + h)
    if offset:
        # positive inputs and weights: every output is 100 +- about 1.3, where
        # bf16 has a spacing of 0.5
        x = 1.0 + 0.1 * torch.randn(b, k, h, w, generator=g)
        wt = (100.0 / k) * (1.0 + 0.01 * torch.randn(n, 1, 1, 1, generator=g)) \
            * torch.ones(n, k, 1, 1)
    else:
        x = torch.randn(b, k, h, w, generator=g) * (
            0.5 + torch.rand(1, k, 1, 1, generator=g)) + 0.3 * torch.randn(
                1, k, 1, 1, generator=g)
        wt = torch.randn(n, k, 1, 1, generator=g) / math.sqrt(k)
    return dict(
        x=_bf16_cl(x), w=wt.bfloat16().cuda(),
        weight=(1.0 + 0.2 * torch.randn(n, generator=g)).cuda(),
        bias=(0.2 * torch.randn(n, generator=g)).cuda(),
        running_mean=(0.1 * torch.randn(n, generator=g)).cuda(),
        running_var=(0.5 + torch.rand(n, generator=g)).cuda())


def _bn(inp, y, part, relu=True):
    rm, rv = inp["running_mean"].clone(), inp["running_var"].clone()
    out, mean, invstd, mask = _C.bn_act_forward(
        y, None, inp["weight"], inp["bias"], rm, rv, MOMENTUM, EPS, relu, part)
    return dict(out=out, mean=mean, invstd=invstd, mask=mask, running_mean=rm,
                running_var=rv)


@functools.lru_cache(maxsize=None)
def _run(shape, offset=False):
    inp = _inputs(shape, offset)
    y, part = _C.conv1x1_stats(inp["x"], inp["w"], shape[5])
    y2, part2 = _C.conv1x1_stats(inp["x"], inp["w"], shape[5])
    stock = F.conv2d(inp["x"], inp["w"])
    fused = _bn(inp, y, part)
    plain = _bn(inp, y, None)
    torch.cuda.synchronize()
    x64, w64 = _rows(inp["x"]), inp["w"].double().cpu().flatten(1)
    ref = dict(y=x64 @ w64.t(), mag=x64.abs() @ w64.abs().t())
    return inp, dict(y=y, part=part, y2=y2, part2=part2, stock=stock,
                     fused=fused, plain=plain), ref


def _plan(shape):
    b, k, n, h, w, wg = shape
    return _C.conv1x1_plan(b * h * w, k, n, wg)


def test_shapes_reach_every_path():
    seen = set()
    for s in SHAPES:
        p = _plan(s)
        assert p["eligible"]
        seen.add((p["mfma_tiles"], p["k_chunk"], p["resident"]))
    assert {(2, 64, True), (8, 64, True), (2, 128, True), (8, 128, True),
            (8, 128, False)} <= seen
    assert _plan(SHAPES[1])["row_tiles"] == 1              # a lone tail tile
    assert _plan(SHAPES[5])["ntiles"] == 8                 # N tiling
    assert _plan(SHAPES[6])["grid"] > 1                    # many workgroups
    p = _plan(SHAPES[7])
    assert p["grid"] == 3 and p["tiles_per_split"] >= 4    # moments carried on


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_output_accuracy(shape):
    inp, got, ref = _run(shape)
    k = shape[1]
    y = got["y"]
    assert y.shape == got["stock"].shape and y.dtype == torch.bfloat16
    assert y.is_contiguous(memory_format=torch.channels_last)
    err = (_rows(y) - ref["y"]).abs()
    bound = 2.0 ** -8 * ref["y"].abs() + (k + 1) * U * ref["mag"]
    n_abs, n_l2 = _errors(_rows(y), ref["y"])
    s_abs, s_l2 = _errors(_rows(got["stock"]), ref["y"])
    msg = (f"native max-abs {n_abs:.3e} rel-L2 {n_l2:.3e}; stock max-abs "
           f"{s_abs:.3e} rel-L2 {s_l2:.3e}; worst err/bound "
           f"{(err / bound.clamp_min(1e-300)).max().item():.3f}")
    print(msg)
    assert bool((err <= bound).all()), msg
    assert n_abs <= 1.5 * s_abs, msg
    assert n_l2 <= 1.5 * s_l2, msg


def _check_stat(name, got, want, bound):
    err = (got.double().cpu() - want).abs()
    worst = (err / bound.clamp_min(1e-300)).max().item()
    msg = f"{name}: max err {err.max().item():.3e}, worst err/bound {worst:.3f}"
    print(msg)
    assert bool((err <= bound).all()), msg


def _check_stats(shape, inp, y, bn):
    """The finalized statistics against fp64 statistics of y itself."""
    rows = y.numel() // y.shape[1]
    run = _plan(shape)["run"]
    k = (run + math.log2(rows / run) + 4) * U
    y64 = _rows(y)
    mean, var = y64.mean(0), y64.var(0, unbiased=False)
    invstd = 1.0 / torch.sqrt(var + EPS)
    abs_mean = y64.abs().mean(0)
    _check_stat("mean", bn["mean"], mean, k * abs_mean)
    _check_stat("invstd", bn["invstd"], invstd, 0.5 * k * invstd)
    rm0 = inp["running_mean"].double().cpu()
    rv0 = inp["running_var"].double().cpu()
    unbiased = var * rows / (rows - 1)
    _check_stat("running_mean", bn["running_mean"],
                (1 - MOMENTUM) * rm0 + MOMENTUM * mean,
                k * ((1 - MOMENTUM) * rm0.abs() + MOMENTUM * abs_mean))
    _check_stat("running_var", bn["running_var"],
                (1 - MOMENTUM) * rv0 + MOMENTUM * unbiased,
                k * ((1 - MOMENTUM) * rv0.abs() + MOMENTUM * unbiased))
    return mean, var, invstd


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_statistics(shape):
    inp, got, _ = _run(shape)
    part = got["part"]
    p = _plan(shape)
    assert tuple(part.shape) == (p["splits"], p["partial_stride"])
    # the counts: every row once per channel tile
    rows = got["y"].numel() // got["y"].shape[1]
    cnt = part[:, 2 * shape[2]:].double().sum(0).cpu()
    assert bool((cnt == rows).all())
    _check_stats(shape, inp, got["y"], got["fused"])


def test_mean_offset():
    """Outputs near 100 with unit spread: E[y^2] - E[y]^2 in fp32 loses the
    variance to cancellation, the running moments do not."""
    shape = SHAPES[6]
    inp, got, _ = _run(shape, True)
    y64 = _rows(got["y"])
    mean, var = y64.mean(0), y64.var(0, unbiased=False)
    assert float(mean.min()) > 95.0 and float(mean.max()) < 105.0
    assert float(var.min()) > 0.5
    assert float((var / mean ** 2).max()) < 1e-3
    # the case has teeth: the naive fp32 formula misses the invstd bound
    rows = y64.shape[0]
    run = _plan(shape)["run"]
    invstd = 1.0 / torch.sqrt(var + EPS)
    bound = 0.5 * (run + math.log2(rows / run) + 4) * U * invstd
    y32 = y64.float()
    naive = 1.0 / torch.sqrt((y32 * y32).mean(0) - y32.mean(0) ** 2 + EPS)
    assert bool(((naive.double() - invstd).abs() > bound).all())
    _check_stats(shape, inp, got["y"], got["fused"])


def _mask_bits(mask, rows, channels):
    bits = (mask.view(-1, 1) >> torch.arange(8, device="cuda")) & 1
    return bits.view(rows, channels).bool()


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_apply_with_partials_matches_own_statistics_pass(shape):
    """bn_act_forward(y, part) against bn_act_forward(y): the same kernels on
    the same y from statistics that may differ in their last bits."""
    inp, got, _ = _run(shape)
    a, b = got["fused"], got["plain"]
    y = got["y"]
    rows, channels = y.numel() // y.shape[1], y.shape[1]
    mean, var, invstd = _check_stats(shape, inp, y, b)
    # the budget of test_gpu_fused_bn.py for `out`: 1.5x the error of the
    # path that makes its own statistics pass
    ref = ((_rows(y) - mean) * invstd * inp["weight"].double().cpu()
           + inp["bias"].double().cpu()).clamp_min(0.0)
    a_abs, a_l2 = _errors(_rows(a["out"]), ref)
    b_abs, b_l2 = _errors(_rows(b["out"]), ref)
    msg = (f"with part max-abs {a_abs:.3e} rel-L2 {a_l2:.3e}; own pass "
           f"max-abs {b_abs:.3e} rel-L2 {b_l2:.3e}")
    print(msg)
    assert a_abs <= 1.5 * b_abs, msg
    assert a_l2 <= 1.5 * b_l2, msg
    # downstream of equal statistics everything is bitwise
    same = ((a["mean"] == b["mean"]) & (a["invstd"] == b["invstd"]))
    print(f"channels with equal statistics: {int(same.sum())}/{channels}")
    oa = a["out"].permute(0, 2, 3, 1).reshape(rows, channels)
    ob = b["out"].permute(0, 2, 3, 1).reshape(rows, channels)
    assert torch.equal(oa[:, same].view(torch.int16),
                       ob[:, same].view(torch.int16))
    ma = _mask_bits(a["mask"], rows, channels)
    mb = _mask_bits(b["mask"], rows, channels)
    assert torch.equal(ma[:, same], mb[:, same])
    assert torch.equal(ma, oa > 0)


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_reproducible(shape):
    _, got, _ = _run(shape)
    assert not bool(got["y"].isnan().any())
    assert not bool(got["part"].isnan().any())
    assert torch.equal(got["y"].view(torch.int16), got["y2"].view(torch.int16))
    assert torch.equal(got["part"], got["part2"])


# ---- through the modules ------------------------------------------------------


def _block(downsample):
    torch.manual_seed(3)
    if downsample:
        down = nn.Sequential(nn.Conv2d(64, 256, 1, bias=False),
                             nn.BatchNorm2d(256))
        blk = Bottleneck(64, 64, 1, down)
    else:
        blk = Bottleneck(256, 64)
    with torch.no_grad():
        for m in blk.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.weight.normal_(1.0, 0.2)
                m.bias.normal_(0.0, 0.2)
    return blk


def _train_step(blk, x, dy, mode, monkeypatch):
    monkeypatch.setenv("CGX_NATIVE_CONV1X1", mode)
    blk = copy.deepcopy(blk).cuda().to(memory_format=torch.channels_last)
    x = x.clone().requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out = blk(x)
    out.backward(dy)
    torch.cuda.synchronize()
    return blk, out.detach(), x.grad


@pytest.mark.parametrize("downsample", [False, True], ids=["plain", "down"])
def test_bottleneck_matches_the_stock_convolutions(downsample, monkeypatch):
    """Switch on (every eligible shape) against CGX_NATIVE_CONV1X1=0, both
    against the block evaluated in fp64: the budgets of test_gpu_fused_bn.py,
    1.5x the error of the path with the stock convolutions."""
    calls = []
    real = _C.conv1x1_stats
    monkeypatch.setattr(fused_bn._C, "conv1x1_stats",
                        lambda *a: calls.append(1) or real(*a))
    blk = _block(downsample)
    g = torch.Generator().manual_seed(17)
    cin = 64 if downsample else 256
    x = _bf16_cl(torch.randn(4, cin, 12, 12, generator=g))
    dy = _bf16_cl(torch.randn(4, 256, 12, 12, generator=g))
    on, out_on, dx_on = _train_step(blk, x, dy, "all", monkeypatch)
    assert len(calls) == (3 if downsample else 2)
    off, out_off, dx_off = _train_step(blk, x, dy, "0", monkeypatch)
    assert len(calls) == (3 if downsample else 2)

    ref = copy.deepcopy(blk).double()
    x64 = x.detach().double().cpu().requires_grad_(True)
    out64 = ref(x64)
    out64.backward(dy.double().cpu())
    out64 = out64.detach()

    def check(name, a, b, want):
        a_abs, a_l2 = _errors(a.double().cpu(), want)
        b_abs, b_l2 = _errors(b.double().cpu(), want)
        msg = (f"{name}: on max-abs {a_abs:.3e} rel-L2 {a_l2:.3e}; off "
               f"max-abs {b_abs:.3e} rel-L2 {b_l2:.3e}")
        print(msg)
        assert a_abs <= 1.5 * b_abs, msg
        assert a_l2 <= 1.5 * b_l2, msg

    check("out", out_on, out_off, out64)
    check("dx", dx_on, dx_off, x64.grad)
    pon, poff, pref = (dict(m.named_parameters()) for m in (on, off, ref))
    for name, want in pref.items():
        check(name, pon[name].grad, poff[name].grad, want.grad)
    # the modules' buffers advance alike: one step everywhere, and running
    # statistics within the same budget
    bon, boff, bref = (dict(m.named_buffers()) for m in (on, off, ref))
    for name, want in bref.items():
        if name.endswith("num_batches_tracked"):
            assert int(bon[name]) == int(boff[name]) == int(want) == 1, name
        else:
            check(name, bon[name], boff[name], want)


def _stock(conv, bn, x, identity, identity_conv, identity_bn):
    y = conv(x)
    if identity_conv is not None:
        return bn_act(bn, y, identity_conv(identity), identity_bn=identity_bn)
    return bn_act(bn, y, identity)


@pytest.mark.parametrize("kind", ["stride2", "fp32", "nchw", "eval", "3x3",
                                  "bias", "env0", "bn_off"])
def test_ineligible_runs_the_stock_convolution(kind, monkeypatch):
    def boom(*a, **k):
        raise AssertionError("native convolution called on a fallback case")

    monkeypatch.setattr(fused_bn._C, "conv1x1_stats", boom)
    monkeypatch.setenv("CGX_NATIVE_CONV1X1", "0" if kind == "env0" else "all")
    if kind == "bn_off":
        monkeypatch.setenv("CGX_FUSED_BN", "0")
    g = torch.Generator().manual_seed(23)
    conv = nn.Conv2d(64, 64, 3 if kind == "3x3" else 1,
                     stride=2 if kind == "stride2" else 1,
                     padding=1 if kind == "3x3" else 0,
                     bias=kind == "bias").cuda()
    bn = nn.BatchNorm2d(64).cuda()
    x = torch.randn(2, 64, 8, 8, generator=g).cuda()
    if kind != "fp32":
        x = x.bfloat16()
        conv = conv.bfloat16()
    if kind != "nchw":
        x = x.contiguous(memory_format=torch.channels_last)
        conv = conv.to(memory_format=torch.channels_last)
    if kind == "eval":
        bn.eval()
    conv2, bn2 = copy.deepcopy(conv), copy.deepcopy(bn)
    xa, xb = (x.clone().requires_grad_(True) for _ in range(2))
    with torch.backends.cudnn.flags(enabled=kind not in ("fp32", "nchw",
                                                         "eval", "bn_off")):
        got = conv_bn_act(conv, bn, xa, xa if kind not in ("stride2",) else None)
        want = _stock(conv2, bn2, xb, xb if kind not in ("stride2",) else None,
                      None, None)
        dy = torch.randn(got.shape, generator=g).to(got.dtype).cuda()
        got.backward(dy)
        want.backward(dy)
    assert torch.equal(got, want)
    assert torch.equal(bn.weight.grad, bn2.weight.grad)
    assert torch.equal(bn.bias.grad, bn2.bias.grad)
    # Both sides ran the same MIOpen backward kernels, which may add in a
    # different order from call to call: a bf16 ulp of the element plus the
    # reordering of an fp32 sum with cancellation, not bits.
    for a, b in [(xa.grad, xb.grad), (conv.weight.grad, conv2.weight.grad)]:
        a, b = a.double(), b.double()
        tol = 2.0 ** -7 * b.abs() + 2.0 ** -9 * b.abs().max()
        assert bool(((a - b).abs() <= tol).all())
    assert torch.equal(bn.running_mean, bn2.running_mean)
    assert torch.equal(bn.running_var, bn2.running_var)
    assert int(bn.num_batches_tracked) == int(bn2.num_batches_tracked)


def test_autograd_function_is_the_convolution():
    """_Conv1x1 under autocast: fp32 master weight in, bf16 kernel, and
    the stock convolution's backward.  MIOpen's backward kernels may add in a
    different order from call to call, so the gradients are held to the
    budget above (1.5x the stock path's error against fp64), not to bits."""
    g = torch.Generator().manual_seed(29)
    x = _bf16_cl(torch.randn(2, 128, 9, 9, generator=g))
    w = (torch.randn(512, 128, 1, 1, generator=g) / 11.0).cuda()
    dy = _bf16_cl(torch.randn(2, 512, 9, 9, generator=g))
    xa, xb = (x.clone().requires_grad_(True) for _ in range(2))
    wa, wb = (w.clone().requires_grad_(True) for _ in range(2))
    with torch.autocast("cuda", dtype=torch.bfloat16):
        ya, part, _ = fused_bn._Conv1x1.apply(xa, wa, True, False)
        yb = F.conv2d(xb, wb)
    assert not part.requires_grad and ya.dtype == yb.dtype == torch.bfloat16
    ya.backward(dy)
    yb.backward(dy)
    assert wa.grad.dtype == torch.float32 and wa.grad.shape == w.shape
    assert xa.grad.is_contiguous(memory_format=torch.channels_last)
    dy64, x64 = _rows(dy), _rows(x)
    w64 = w.bfloat16().double().cpu().flatten(1)
    for name, a, b, want in [
            ("dx", _rows(xa.grad), _rows(xb.grad), dy64 @ w64),
            ("dw", wa.grad.double().cpu().flatten(1),
             wb.grad.double().cpu().flatten(1), dy64.t() @ x64)]:
        a_abs, a_l2 = _errors(a, want)
        b_abs, b_l2 = _errors(b, want)
        msg = (f"{name}: native max-abs {a_abs:.3e} rel-L2 {a_l2:.3e}; stock "
               f"max-abs {b_abs:.3e} rel-L2 {b_l2:.3e}")
        print(msg)
        assert a_abs <= 1.5 * b_abs, msg
        assert a_l2 <= 1.5 * b_l2, msg
