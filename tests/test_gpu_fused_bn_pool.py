"""Stem: BatchNorm + ReLU + 3x3/2/1 max-pool in one forward kernel and two
backward sweeps, against F.max_pool2d(native bn_act(x), 3, 2, 1) with autograd.

The fused path computes relu(bf16(bn(x))) with bn_apply<relu>'s arithmetic,
picks max_pool2d's maximum, and its backward sweeps visit the rows in the
order of bn_bwd_reduce / bn_bwd_dx: the pooled output, dx, the statistics AND
dgamma / dbeta are required bit for bit (the sweep order is kept).
"""

import copy
import functools

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from torch_cgx_amd import _C  # noqa: E402
from torch_cgx_amd.ops import fused_bn  # noqa: E402
from torch_cgx_amd.ops.fused_bn import bn_act, bn_act_pool  # noqa: E402

CASES = [((2, 64, 8, 8), "randn"), ((3, 64, 7, 9), "randn"),
         ((2, 8, 2, 2), "randn"), ((2, 64, 30, 30), "randn"),
         ((2, 64, 112, 112), "randn"), ((2, 64, 30, 30), "ties"),
         ((3, 64, 7, 9), "ties"), ((2, 64, 30, 30), "dead")]
MOMENTUM, EPS = 0.1, 1e-5


def _ids(case):
    (n, c, h, w), kind = case
    return f"{n}x{c}x{h}x{w}-{kind}"


def _bf16_cl(t):
    return t.bfloat16().cuda().contiguous(memory_format=torch.channels_last)


def _make_bn(c, g, dead=False):
    bn = nn.BatchNorm2d(c, eps=EPS, momentum=MOMENTUM)
    with torch.no_grad():
        bn.weight.copy_(1.0 + 0.2 * torch.randn(c, generator=g))
        bn.bias.copy_(0.2 * torch.randn(c, generator=g))
        bn.running_mean.copy_(0.1 * torch.randn(c, generator=g))
        bn.running_var.copy_(0.5 + torch.rand(c, generator=g))
        if dead:
            # channel 3: a zero scale and a negative shift, so the BatchNorm
            # output is negative everywhere
            bn.weight[3] = 0.0
            bn.bias[3] = -1.0
    return bn.cuda()


def _make_inputs(shape, kind, seed):
    g = torch.Generator().manual_seed(seed)
    n, c, h, w = shape
    if kind == "ties":
        # four distinct values: most windows hold their maximum several times
        x = torch.tensor([-1.5, -0.25, 0.5, 2.0])[
            torch.randint(0, 4, shape, generator=g)]
    else:
        x = torch.randn(shape, generator=g) * (
            0.5 + torch.rand(1, c, 1, 1, generator=g)) + torch.randn(
                1, c, 1, 1, generator=g)
    oh, ow = (h - 1) // 2 + 1, (w - 1) // 2 + 1
    return (_bf16_cl(x), _bf16_cl(torch.randn(n, c, oh, ow, generator=g)),
            _make_bn(c, g, dead=kind == "dead"))


def _step(fn, bn, x, dy):
    bn = copy.deepcopy(bn)
    x = x.clone().requires_grad_(True)
    out = fn(bn, x)
    out.backward(dy)
    return dict(out=out.detach(), dx=x.grad, dgamma=bn.weight.grad,
                dbeta=bn.bias.grad, running_mean=bn.running_mean,
                running_var=bn.running_var,
                tracked=bn.num_batches_tracked.clone())


def _composed(bn, x):
    return F.max_pool2d(bn_act(bn, x), 3, 2, 1)


def _fused(bn, x):
    return bn_act_pool(bn, x, nn.MaxPool2d(3, 2, 1))


@functools.lru_cache(maxsize=None)
def _run(shape, kind):
    x, dy, bn = _make_inputs(shape, kind, seed=hash(shape) % 9973)
    want = _step(_composed, bn, x, dy)
    got = _step(_fused, bn, x, dy)
    again = _step(_fused, bn, x, dy)
    torch.cuda.synchronize()
    return x, dy, bn, want, got, again


def _same(a, b, key):
    assert not bool(a.isnan().any()), key
    if a.dtype == torch.bfloat16:  # -0 and +0 are different bits
        a, b = a.view(torch.int16), b.view(torch.int16)
    assert torch.equal(a, b), key


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_bitwise_the_composition(case):
    (n, c, h, w), kind = case
    x, dy, bn, want, got, _ = _run(*case)
    assert got["out"].shape == want["out"].shape
    assert got["out"].is_contiguous(memory_format=torch.channels_last)
    assert got["dx"].is_contiguous(memory_format=torch.channels_last)
    for key in want:
        _same(got[key], want[key], key)
    if kind == "ties" and h == 30:
        # most windows tie: count the windows whose maximum occurs twice
        # (few of them touch the border at this size)
        y = bn_act(copy.deepcopy(bn), x).float()
        cols = F.unfold(y, 3, padding=1, stride=2).view(n, c, 9, -1)
        ties = (cols == cols.max(2, keepdim=True).values).sum(2) > 1
        assert float(ties.float().mean()) > 0.5
    if kind == "dead":
        assert not bool(got["out"][:, 3].any())
        assert not bool(got["dx"][:, 3].any())
        assert float(got["dgamma"][3]) == 0 and float(got["dbeta"][3]) == 0
        assert bool(got["out"][:, 2].any()) and bool(got["dx"][:, 2].any())


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_reproducible(case):
    _, _, _, _, got, again = _run(*case)
    for key in got:
        _same(got[key], again[key], key)


def test_direct_call_and_arg_bytes():
    """The argmax byte names a window position that holds the maximum, or the
    reserved value exactly where the pooled value is zero."""
    shape = (3, 64, 7, 9)
    x, dy, bn = _make_inputs(shape, "ties", seed=4)
    y = bn_act(copy.deepcopy(bn), x)
    out, mean, invstd, arg = _C.bn_act_pool_forward(
        x, bn.weight, bn.bias, bn.running_mean.clone(),
        bn.running_var.clone(), MOMENTUM, EPS)
    assert arg.dtype == torch.uint8 and arg.shape == out.shape
    n, c, h, w = shape
    cols = F.unfold(F.pad(y.float(), (1, 1, 1, 1), value=-1.0), 3,
                    stride=2).view(n, c, 9, -1)
    flat_arg = arg.reshape(n, c, -1).long()
    flat_out = out.float().reshape(n, c, -1)
    none = flat_arg == 9
    assert torch.equal(none, flat_out <= 0)
    assert bool(none.any()) and bool((~none).any())
    picked = cols.gather(2, flat_arg.clamp_max(8).unsqueeze(2)).squeeze(2)
    assert torch.equal(picked[~none], flat_out[~none])
    # the first of equal values: nothing before the named position is as large
    before = torch.arange(9, device="cuda").view(1, 1, 9, 1) < \
        flat_arg.unsqueeze(2)
    earlier = torch.where(before, cols, torch.full_like(cols, -1.0)).max(
        2).values
    assert bool((earlier[~none] < flat_out[~none]).all())


@pytest.mark.parametrize("kind", ["kernel", "stride", "padding", "ceil",
                                  "eval", "env0", "indices"])
def test_fallback_is_the_stock_path(kind, monkeypatch):
    def boom(*a, **k):
        raise AssertionError("fused stem kernel called on a fallback case")

    monkeypatch.setattr(fused_bn._C, "bn_act_pool_forward", boom)
    if kind == "env0":
        monkeypatch.setenv("CGX_FUSED_BN", "0")
    pool = {"kernel": nn.MaxPool2d(2, 2, 1), "stride": nn.MaxPool2d(3, 1, 1),
            "padding": nn.MaxPool2d(3, 2, 0),
            "ceil": nn.MaxPool2d(3, 2, 1, ceil_mode=True),
            "indices": nn.MaxPool2d(3, 2, 1, return_indices=True),
            }.get(kind, nn.MaxPool2d(3, 2, 1))
    x, _, bn = _make_inputs((2, 64, 8, 8), "randn", seed=9)
    if kind == "eval":
        bn.eval()
    ref = copy.deepcopy(bn)
    xa, xb = (x.clone().requires_grad_(True) for _ in range(2))
    with torch.backends.cudnn.flags(enabled=False):
        got = bn_act_pool(bn, xa, pool)
        want = pool(bn_act(ref, xb))
        if kind == "indices":
            assert torch.equal(got[1], want[1])
            got, want = got[0], want[0]
        dy = torch.ones_like(want)
        got.backward(dy)
        want.backward(dy)
    assert torch.equal(got, want)
    assert torch.equal(xa.grad, xb.grad)
    assert torch.equal(bn.weight.grad, ref.weight.grad)
    assert torch.equal(bn.bias.grad, ref.bias.grad)
    assert torch.equal(bn.running_mean, ref.running_mean)
    assert torch.equal(bn.running_var, ref.running_var)
    assert int(bn.num_batches_tracked) == int(ref.num_batches_tracked)
