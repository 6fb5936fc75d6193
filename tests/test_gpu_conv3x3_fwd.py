"""The native 3x3 / stride 1 / padding 1 convolution that also produces the
BatchNorm partials of its output (conv3x3_stats in csrc/conv3x3_kernels.hip),
against fp64 on the CPU and against the stock convolution.

Error budgets, those of test_gpu_conv1x1_bn.py with 9C terms.  Y is bf16 of an
fp32-accumulated sum of 9C products: |err| <= 2^-8 |ref| + (9C+1) 2^-24
sum|x w|.  The statistics are a sequential run of L = plan["run"] terms per
lane followed by trees: |err| <= (L + log2(R/L) + 4) 2^-24 sum|terms|, against
fp64 statistics of the kernel's own rounded output.  MIOpen's convolution is
the yardstick: the native error may be at most 1.5x its error.
"""

import functools
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from torch_cgx_amd import _C  # noqa: E402
from torch_cgx_amd.models.resnet import Bottleneck  # noqa: E402
from torch_cgx_amd.ops import fused_bn  # noqa: E402


# (batch, C, N, H, W, max_workgroups).  A tile is 256 pixels in memory order,
# so batch 2 of single pixels (one pixel alone has no statistics) puts the
# other image right beside each pixel; 2 x 3 x 56 is the smallest height at
# that width with two tiles, the last one short; 5 x 12 x 12 under a cap of
# two workgroups is the smallest walk of more than one tile per workgroup.
SHAPES = [(2, 64, 64, 1, 1, 0), (2, 64, 64, 3, 5, 0), (3, 128, 64, 7, 7, 0),
          (2, 64, 128, 7, 7, 0), (2, 64, 64, 3, 56, 0),
          (2, 256, 256, 5, 5, 0), (2, 512, 512, 3, 3, 0),
          (5, 64, 64, 12, 12, 2), (64, 128, 64, 14, 14, 7)]
BORDERS = SHAPES[:4]
MOMENTUM, EPS = 0.1, 1e-5
U = 2.0 ** -24


def _ids(s):
    return "{}x{}to{}x{}x{}-wg{}".format(*s)


def _bf16_cl(t):
    return t.bfloat16().cuda().contiguous(memory_format=torch.channels_last)


def _bits(t):
    return t.contiguous().view(torch.int16)


def _rows(t):
    """[B,C,H,W] -> fp64 CPU [R, C]"""
    return t.detach().double().cpu().permute(0, 2, 3, 1).reshape(
        -1, t.shape[1])


def _plan(shape):
    b, c, n, h, w, wg = shape
    return _C.conv3x3_fwd_plan(b, h, w, c, n, wg)


def _inputs(shape, offset=False):
    b, c, n, h, w, _ = shape
    g = torch.Generator().manual_seed(c * 7 + n * 3 + h)
    if offset:
        # the centre tap carries 100, the other eight about +-0.5: every
        # output is near 100, where bf16 has a spacing of 0.5
        x = 1.0 + 0.1 * torch.randn(b, c, h, w, generator=g)
        wt = 0.5 * torch.randn(n, c, 3, 3, generator=g) / math.sqrt(9 * c)
        wt[:, :, 1, 1] += (100.0 / c) * (1.0 + 0.01 * torch.randn(
            n, 1, generator=g))
    else:
        x = torch.randn(b, c, h, w, generator=g) * (
            0.5 + torch.rand(1, c, 1, 1, generator=g)) + 0.3 * torch.randn(
                1, c, 1, 1, generator=g)
        wt = torch.randn(n, c, 3, 3, generator=g) / math.sqrt(9 * c)
    return dict(
        x=_bf16_cl(x), w=_bf16_cl(wt),
        weight=(1.0 + 0.2 * torch.randn(n, generator=g)).cuda(),
        bias=(0.2 * torch.randn(n, generator=g)).cuda(),
        running_mean=(0.1 * torch.randn(n, generator=g)).cuda(),
        running_var=(0.5 + torch.rand(n, generator=g)).cuda())


def _bn(inp, y, part):
    rm, rv = inp["running_mean"].clone(), inp["running_var"].clone()
    _, mean, invstd, _ = _C.bn_act_forward(
        y, None, inp["weight"], inp["bias"], rm, rv, MOMENTUM, EPS, True, part)
    return dict(mean=mean, invstd=invstd)


@functools.lru_cache(maxsize=None)
def _run(shape, offset=False):
    inp = _inputs(shape, offset)
    keep = inp["x"].clone(), inp["w"].clone()
    y, part = _C.conv3x3_stats(inp["x"], inp["w"], shape[5])
    y2, part2 = _C.conv3x3_stats(inp["x"], inp["w"], shape[5])
    got = dict(y=y, part=part, y2=y2, part2=part2,
               stock=F.conv2d(inp["x"], inp["w"], padding=1),
               fused=_bn(inp, y, part), plain=_bn(inp, y, None))
    torch.cuda.synchronize()
    got["inputs_unchanged"] = (torch.equal(_bits(inp["x"]), _bits(keep[0]))
                               and torch.equal(_bits(inp["w"]), _bits(keep[1])))
    x64, w64 = inp["x"].double().cpu(), inp["w"].double().cpu()
    ref = dict(y=_rows(F.conv2d(x64, w64, padding=1)),
               mag=_rows(F.conv2d(x64.abs(), w64.abs(), padding=1)))
    return inp, got, ref


def test_shapes_reach_the_plans_they_are_for():
    plans = [_plan(s) for s in SHAPES]
    assert all(p["eligible"] for p in plans)
    # both instantiations the launcher has: the weight resident and streamed
    assert {p["resident"] for p in plans} == {True, False}
    assert all(p["row_tiles"] == 1 for p in plans[:4])   # images share a tile
    assert plans[4]["row_tiles"] == 2                    # a short last tile
    assert plans[4]["rows"] % plans[4]["tile_rows"] != 0
    assert _C.conv3x3_fwd_plan(2, 2, 56, 64, 64)["row_tiles"] == 1
    assert plans[5]["ntiles"] == 4 and plans[5]["nchunks"] == 8
    assert plans[6]["ntiles"] == 8 and plans[6]["nchunks"] == 16
    assert plans[7]["grid"] == 2 and plans[7]["tiles_per_split"] == 2
    assert plans[8]["splits"] == 7 and plans[8]["tiles_per_split"] == 7


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_accuracy_and_against_stock(shape):
    _, got, ref = _run(shape)
    b, c, n, h, w, _ = shape
    y = got["y"]
    assert tuple(y.shape) == (b, n, h, w) and y.dtype == torch.bfloat16
    assert y.is_contiguous(memory_format=torch.channels_last)
    assert not bool(y.isnan().any())
    assert torch.equal(_bits(y), _bits(got["y2"]))
    assert torch.equal(got["part"], got["part2"])
    assert got["inputs_unchanged"]
    err = (_rows(y) - ref["y"]).abs()
    bound = 2.0 ** -8 * ref["y"].abs() + (9 * c + 1) * U * ref["mag"]

    def errors(t):
        d = _rows(t) - ref["y"]
        return d.abs().max().item(), (d.norm() / ref["y"].norm()).item()

    (a_abs, a_l2), (b_abs, b_l2) = errors(y), errors(got["stock"])
    msg = (f"native max-abs {a_abs:.3e} rel-L2 {a_l2:.3e}; stock max-abs "
           f"{b_abs:.3e} rel-L2 {b_l2:.3e}; worst err/bound "
           f"{(err / bound.clamp_min(1e-300)).max().item():.3f}")
    print(msg)
    assert bool((err <= bound).all()), msg
    assert a_abs <= 1.5 * b_abs, msg
    assert a_l2 <= 1.5 * b_l2, msg


def _within(name, got, want, bound):
    err = (got.double().cpu() - want).abs()
    msg = (f"{name}: max err {err.max().item():.3e}, worst err/bound "
           f"{(err / bound.clamp_min(1e-300)).max().item():.3f}")
    print(msg)
    assert bool((err <= bound).all()), msg


@pytest.mark.parametrize(
    "shape,offset", [(s, False) for s in SHAPES] + [(SHAPES[i], True)
                                                    for i in (4, 7, 8)],
    ids=lambda v: _ids(v) if isinstance(v, tuple) else f"offset{int(v)}")
def test_statistics(shape, offset):
    _, got, _ = _run(shape, offset)
    p, n = _plan(shape), shape[2]
    part = got["part"].double().cpu()
    assert tuple(part.shape) == (p["splits"], p["pstride"])
    y64 = _rows(got["y"])
    rows = y64.shape[0]
    if offset:
        assert 95.0 < float(y64.mean(0).min()) and float(y64.std(0).max()) < 2.0
    # no pad was counted: every pixel once per channel tile
    cnt = part[:, 2 * n:]
    assert bool((cnt.sum(0) == rows).all()) and rows == p["rows"]
    # the partial rows merged in fp64 (Chan et al.)
    per = cnt.repeat_interleave(n // p["ntiles"], dim=1)
    mean = (part[:, :n] * per).sum(0) / rows
    m2 = (part[:, n:2 * n] + per * (part[:, :n] - mean) ** 2).sum(0)
    k = (p["run"] + math.log2(rows / p["run"]) + 4) * U
    want_mean, want_var = y64.mean(0), y64.var(0, unbiased=False)
    abs_mean = y64.abs().mean(0)
    _within("mean", mean, want_mean, k * abs_mean)
    _within("M2", m2, want_var * rows, k * want_var * rows)
    invstd = 1.0 / torch.sqrt(want_var + EPS)
    for name in ("fused", "plain"):
        _within(name + " mean", got[name]["mean"], want_mean, k * abs_mean)
        _within(name + " invstd", got[name]["invstd"], invstd, 0.5 * k * invstd)
    _within("fused - plain mean", got["fused"]["mean"],
            got["plain"]["mean"].double().cpu(), k * abs_mean)
    _within("fused - plain invstd", got["fused"]["invstd"],
            got["plain"]["invstd"].double().cpu(), 0.5 * k * invstd)


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
def test_nothing_outside_the_images_reaches_a_result(shape):
    inp, got, _ = _run(shape)
    big_x, vx = _in_poisoned_buffer(inp["x"])
    big_w, vw = _in_poisoned_buffer(inp["w"])
    assert _C.conv3x3_fwd_eligible(vx, vw)
    for big in (big_x, big_w):
        assert bool(big[0].isnan().all()) and bool(big[-1].isnan().all())
    y, part = _C.conv3x3_stats(vx, vw, shape[5])
    assert bool(y.isfinite().all()) and bool(part.isfinite().all())
    assert torch.equal(_bits(y), _bits(got["y"]))
    assert torch.equal(part, got["part"])


def test_rejects_what_it_cannot_take():
    x = _bf16_cl(torch.randn(2, 128, 4, 4))
    w = _bf16_cl(torch.randn(64, 128, 3, 3))
    assert _C.conv3x3_fwd_eligible(x, w)
    xs = lambda c: _bf16_cl(torch.randn(2, c, 4, 4))  # noqa: E731
    ws = lambda n, c: _bf16_cl(torch.randn(n, c, 3, 3))  # noqa: E731
    bad = [(x.float(), w), (x, w.float()), (x.contiguous(), w),
           (x, w.contiguous()), (x.cpu(), w.cpu()), (x, ws(64, 64)),
           (xs(32), ws(64, 32)), (xs(96), ws(64, 96)), (xs(1024), ws(64, 1024)),
           (x, ws(32, 128)), (x, ws(96, 128)), (x, ws(1024, 128)),
           (x, _bf16_cl(torch.randn(64, 128, 1, 1)))]
    for args in bad:
        assert not _C.conv3x3_fwd_eligible(*args)
        with pytest.raises(RuntimeError):
            _C.conv3x3_stats(*args)
    with pytest.raises(RuntimeError):
        _C.conv3x3_stats(x, w, -1)


_REAL = _C.conv3x3_stats, _C.bn_act_forward


def _train_step(mode, monkeypatch, wrw="0"):
    """One step of a Bottleneck(256, 64) under bf16 autocast -> (output, the
    gradients, the (y, part) of every call of the kernel, the `part` bn2
    received)."""
    monkeypatch.setenv("CGX_NATIVE_CONV3X3", mode)
    monkeypatch.setenv("CGX_NATIVE_CONV3X3_WRW", wrw)
    calls, parts = [], []
    real, real_bn = _REAL

    def spy(x, w, max_workgroups=0):
        calls.append(real(x, w, max_workgroups))
        return calls[-1]

    def spy_bn(x, *args):
        if x.shape[1] == 64 and calls and x is calls[-1][0]:
            parts.append(args[-1])
        return real_bn(x, *args)

    monkeypatch.setattr(fused_bn._C, "conv3x3_stats", spy)
    monkeypatch.setattr(fused_bn._C, "bn_act_forward", spy_bn)
    torch.manual_seed(3)
    blk = Bottleneck(256, 64).cuda().to(memory_format=torch.channels_last)
    g = torch.Generator().manual_seed(17)
    x = _bf16_cl(torch.randn(4, 256, 12, 12, generator=g)).requires_grad_(True)
    dy = _bf16_cl(torch.randn(4, 256, 12, 12, generator=g))
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out = blk(x)
    out.backward(dy)
    torch.cuda.synchronize()
    grads = [x.grad] + [q.grad for q in blk.parameters()]
    return out.detach(), grads, calls, parts


def test_bottleneck_routes_the_forward(monkeypatch):
    out, grads, calls, parts = _train_step("all", monkeypatch)
    assert len(calls) == 1 and len(parts) == 1 and parts[0] is calls[0][1]
    out0, grads0, calls0, _ = _train_step("0", monkeypatch)
    assert not calls0
    # Both blocks round to bf16 at the four tensors from conv2's output to the
    # block's: four half-ulps of 2^-8 each way on an element, and where a sum
    # cancels the same against the largest element.
    a, b = out.double(), out0.double()
    tol = 2.0 ** -6 * b.abs() + 2.0 ** -7 * b.abs().max()
    assert a.shape == b.shape and bool(((a - b).abs() <= tol).all())
    # A gradient has no such bound: where an input of a ReLU is within a
    # rounding of zero its mask differs between the two blocks and the
    # element's whole gradient comes or goes.  So the gradients get the
    # yardstick of test_accuracy_and_against_stock: against the same block in
    # fp64 on the CPU the native block's error is at most 1.5x the stock one's.
    torch.manual_seed(3)
    ref = Bottleneck(256, 64).double()
    g = torch.Generator().manual_seed(17)
    x = torch.randn(4, 256, 12, 12, generator=g).bfloat16().double()
    dy = torch.randn(4, 256, 12, 12, generator=g).bfloat16().double()
    ref(x.requires_grad_(True)).backward(dy)
    for a, b, r in zip(grads, grads0, [x.grad] + [q.grad
                                                  for q in ref.parameters()]):
        ea, eb = ((t.double().cpu() - r).norm().item() / r.norm().item()
                  for t in (a, b))
        print(f"gradient {tuple(r.shape)}: rel-L2 error native {ea:.3e} "
              f"stock {eb:.3e}")
        assert a.shape == r.shape and ea <= 1.5 * eb
    # the weight-gradient switch does not reach the forward, CGX_FUSED_BN does
    assert len(_train_step("all", monkeypatch, wrw="all")[2]) == 1
    assert fused_bn.native_conv3x3_mode() == "all"
    monkeypatch.setenv("CGX_FUSED_BN", "0")
    assert fused_bn.native_conv3x3_mode() == "0"
    assert not _train_step("all", monkeypatch)[2]
