"""Fused NHWC bf16 BatchNorm (+ residual add, + ReLU) against an fp64
evaluation of the same formula, with the stock GPU path as the yardstick.

Error budget.  Outputs and input gradients are bf16, so both paths' errors are
dominated by the final rounding; the native path may be at most 1.5x the stock
path's error (ties may break differently).  fp32 statistics and parameter
gradients are sums of R terms computed as a sequential run of L terms per
thread followed by a tree: |error| <= (L + log2(R/L) + 4) * 2^-24 * sum|terms|,
with L the plan's per-thread run length and the 4 covering the roundings of
each term and of the final combination.  For invstd = (var + eps)^-1/2 the
terms are those of var + eps, and the bound is carried through the derivative.

The stock path runs with the cuDNN/MIOpen switch off, i.e. on ATen's own
batch-norm kernels: at these test-sized channels_last shapes MIOpen's
batch-norm backward crashed the host process (a segmentation fault inside the
autograd thread at (2,64,7,7), before any result came back).  At the
benchmark's shapes the model keeps using MIOpen wherever bn_act falls back.
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
from torch_cgx_amd.ops import fused_bn  # noqa: E402
from torch_cgx_amd.ops.fused_bn import bn_act  # noqa: E402

SHAPES = [(2, 64, 1, 1), (2, 64, 7, 7), (3, 256, 5, 5), (4, 2048, 7, 7),
          (2, 64, 56, 56)]
CASES = [(s, relu, idn) for s in SHAPES for relu in (False, True)
         for idn in (False, True)]
MOMENTUM, EPS = 0.1, 1e-5
U = 2.0 ** -24


def _aten_batch_norm():
    """Context in which F.batch_norm / nn.BatchNorm2d run ATen's kernels."""
    return torch.backends.cudnn.flags(enabled=False)


def _ids(case):
    (n, c, h, w), relu, idn = case
    return f"{n}x{c}x{h}x{w}-relu{int(relu)}-id{int(idn)}"


def _bf16_cl(t):
    return t.bfloat16().cuda().contiguous(memory_format=torch.channels_last)


def _rows(t):
    """[N,C,H,W] -> fp64 CPU [R, C]"""
    return t.detach().double().cpu().permute(0, 2, 3, 1).reshape(
        -1, t.shape[1])


def _sum_factor(rows, channels):
    run = _C.bn_plan(rows, channels)["rows_per_thread"]
    return (run + math.log2(rows / run) + 4) * U


def _make_inputs(shape, seed, offset=False):
    g = torch.Generator().manual_seed(seed)
    n, c, h, w = shape
    x = torch.randn(shape, generator=g)
    if offset:
        # bf16 has a spacing of 0.5 at 100, so a spread of 0.01 would round
        # away; std 1 leaves some twenty distinct values on that grid
        x = 100.0 + x
    else:
        # per-channel scale and shift, so that mean and variance matter
        x = x * (0.5 + torch.rand(1, c, 1, 1, generator=g)) + torch.randn(
            1, c, 1, 1, generator=g)
    return dict(
        x=_bf16_cl(x),
        identity=_bf16_cl(torch.randn(shape, generator=g)),
        dy=_bf16_cl(torch.randn(shape, generator=g)),
        weight=(1.0 + 0.2 * torch.randn(c, generator=g)).cuda(),
        bias=(0.2 * torch.randn(c, generator=g)).cuda(),
        running_mean=(0.1 * torch.randn(c, generator=g)).cuda(),
        running_var=(0.5 + torch.rand(c, generator=g)).cuda(),
    )


def _native(inp, relu, with_identity):
    rm, rv = inp["running_mean"].clone(), inp["running_var"].clone()
    idn = inp["identity"] if with_identity else None
    out, mean, invstd, mask = _C.bn_act_forward(
        inp["x"], idn, inp["weight"], inp["bias"], rm, rv, MOMENTUM, EPS, relu)
    dx, dgamma, dbeta, didn = _C.bn_act_backward(
        inp["dy"], inp["x"], mean, invstd, inp["weight"], mask, with_identity)
    return dict(out=out, mean=mean, invstd=invstd, mask=mask, dx=dx,
                dgamma=dgamma, dbeta=dbeta, didentity=didn, running_mean=rm,
                running_var=rv)


def _stock(inp, relu, with_identity):
    rm, rv = inp["running_mean"].clone(), inp["running_var"].clone()
    x = inp["x"].clone().requires_grad_(True)
    idn = inp["identity"].clone().requires_grad_(True)
    w = inp["weight"].clone().requires_grad_(True)
    b = inp["bias"].clone().requires_grad_(True)
    with _aten_batch_norm():
        out = F.batch_norm(x, rm, rv, w, b, True, MOMENTUM, EPS)
        if with_identity:
            out = out + idn
        if relu:
            out = torch.relu(out)
        out.backward(inp["dy"])
    return dict(out=out.detach(), dx=x.grad, dgamma=w.grad, dbeta=b.grad,
                didentity=idn.grad if with_identity else None,
                running_mean=rm, running_var=rv)


def _reference_forward(inp, relu, with_identity):
    x = _rows(inp["x"])
    mean = x.mean(0)
    var = x.var(0, unbiased=False)
    invstd = 1.0 / torch.sqrt(var + EPS)
    y = (x - mean) * invstd * inp["weight"].double().cpu() \
        + inp["bias"].double().cpu()
    if with_identity:
        y = y + _rows(inp["identity"])
    if relu:
        y = y.clamp_min(0.0)
    return dict(x=x, mean=mean, var=var, invstd=invstd, out=y)


def _reference_dx(inp, ref, out_rows, relu):
    """fp64 dx, with the ReLU mask taken from the forward output `out_rows`
    of the path under test."""
    g = _rows(inp["dy"])
    if relu:
        g = g * (out_rows > 0)
    xhat = (ref["x"] - ref["mean"]) * ref["invstd"]
    w = inp["weight"].double().cpu()
    dx = w * ref["invstd"] * (g - g.mean(0) - xhat * (g * xhat).mean(0))
    return g, dx


def _errors(got, want):
    d = _rows(got) - want
    return d.abs().max().item(), (d.norm() / want.norm().clamp_min(1e-300)).item()


@functools.lru_cache(maxsize=None)
def _run(shape, relu, with_identity, offset=False):
    inp = _make_inputs(shape, seed=hash((shape, relu, with_identity)) % 9973,
                       offset=offset)
    nat = _native(inp, relu, with_identity)
    nat2 = _native(inp, relu, with_identity)
    stk = _stock(inp, relu, with_identity)
    ref = _reference_forward(inp, relu, with_identity)
    torch.cuda.synchronize()
    return inp, nat, nat2, stk, ref


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_forward_accuracy(case):
    inp, nat, _, stk, ref = _run(*case)
    n_abs, n_l2 = _errors(nat["out"], ref["out"])
    s_abs, s_l2 = _errors(stk["out"], ref["out"])
    msg = (f"native max-abs {n_abs:.3e} rel-L2 {n_l2:.3e}; "
           f"stock max-abs {s_abs:.3e} rel-L2 {s_l2:.3e}")
    print(msg)
    assert nat["out"].is_contiguous(memory_format=torch.channels_last)
    assert n_abs <= 1.5 * s_abs, msg
    assert n_l2 <= 1.5 * s_l2, msg


def _check_stat(name, got, want, bound):
    err = (got.double().cpu() - want).abs()
    worst = (err / bound.clamp_min(1e-300)).max().item()
    msg = (f"{name}: max err {err.max().item():.3e}, "
           f"worst err/bound {worst:.3f}")
    print(msg)
    assert bool((err <= bound).all()), msg


def _check_forward_stats(inp, nat, ref, shape):
    rows, channels = ref["x"].shape
    k = _sum_factor(rows, channels)
    x = ref["x"]
    abs_mean = x.abs().mean(0)
    _check_stat("mean", nat["mean"], ref["mean"], k * abs_mean)
    # d invstd = -1/2 (var+eps)^-3/2 d(var+eps), |d(var+eps)| <= k (var+eps)
    _check_stat("invstd", nat["invstd"], ref["invstd"],
                0.5 * k * ref["invstd"])
    rm0 = inp["running_mean"].double().cpu()
    rv0 = inp["running_var"].double().cpu()
    unbiased = ref["var"] * rows / (rows - 1)
    _check_stat("running_mean", nat["running_mean"],
                (1 - MOMENTUM) * rm0 + MOMENTUM * ref["mean"],
                k * ((1 - MOMENTUM) * rm0.abs() + MOMENTUM * abs_mean))
    _check_stat("running_var", nat["running_var"],
                (1 - MOMENTUM) * rv0 + MOMENTUM * unbiased,
                k * ((1 - MOMENTUM) * rv0.abs() + MOMENTUM * unbiased))


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_statistics(case):
    shape, relu, with_identity = case
    inp, nat, _, _, ref = _run(*case)
    _check_forward_stats(inp, nat, ref, shape)
    rows, channels = ref["x"].shape
    k = _sum_factor(rows, channels)
    # the backward's own inputs: the native fp32 mean and invstd
    g = _rows(inp["dy"])
    if relu:
        g = g * (_rows(nat["out"]) > 0)
    xhat = (ref["x"] - nat["mean"].double().cpu()) \
        * nat["invstd"].double().cpu()
    _check_stat("dbeta", nat["dbeta"], g.sum(0), k * g.abs().sum(0))
    _check_stat("dgamma", nat["dgamma"], (g * xhat).sum(0),
                k * (g * xhat).abs().sum(0))


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_input_gradients(case):
    shape, relu, with_identity = case
    inp, nat, _, stk, ref = _run(*case)
    g_nat, dx_nat = _reference_dx(inp, ref, _rows(nat["out"]), relu)
    g_stk, dx_stk = _reference_dx(inp, ref, _rows(stk["out"]), relu)
    n_abs, n_l2 = _errors(nat["dx"], dx_nat)
    s_abs, s_l2 = _errors(stk["dx"], dx_stk)
    msg = (f"dx: native max-abs {n_abs:.3e} rel-L2 {n_l2:.3e}; "
           f"stock max-abs {s_abs:.3e} rel-L2 {s_l2:.3e}")
    print(msg)
    assert n_abs <= 1.5 * s_abs, msg
    assert n_l2 <= 1.5 * s_l2, msg
    if with_identity:
        n_abs, n_l2 = _errors(nat["didentity"], g_nat)
        s_abs, s_l2 = _errors(stk["didentity"], g_stk)
        msg = (f"didentity: native max-abs {n_abs:.3e} rel-L2 {n_l2:.3e}; "
               f"stock max-abs {s_abs:.3e} rel-L2 {s_l2:.3e}")
        print(msg)
        assert n_abs <= 1.5 * s_abs, msg
        assert n_l2 <= 1.5 * s_l2, msg
    else:
        assert nat["didentity"] is None


@pytest.mark.parametrize("case", [c for c in CASES if c[2]], ids=_ids)
def test_mask_exact(case):
    shape, relu, _ = case
    inp, nat, _, _, _ = _run(*case)
    did = nat["didentity"].view(torch.int16)
    dy = inp["dy"].view(torch.int16)
    if not relu:
        assert nat["mask"] is None
        assert torch.equal(did, dy)
        return
    out = nat["out"]
    assert not bool((out < 0).any())
    zero, pos = out == 0, out > 0
    assert bool(zero.any()) and bool(pos.any())
    assert bool((did[zero] == 0).all())
    assert torch.equal(did[pos], dy[pos])
    # one bit per element, in memory order
    bits = (nat["mask"].view(-1, 1) >> torch.arange(8, device="cuda")) & 1
    assert torch.equal(bits.view(-1).bool(),
                       pos.permute(0, 2, 3, 1).reshape(-1))


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_reproducible(case):
    _, nat, nat2, _, _ = _run(*case)
    for key, a in nat.items():
        b = nat2[key]
        if a is None:
            assert b is None, key
        else:
            assert not bool(a.isnan().any()), key
            assert torch.equal(a, b), key


def test_mean_offset():
    """A common offset 100 standard deviations wide: E[x^2] - E[x]^2 in fp32
    loses the variance to cancellation, a shifted or Welford sum does not."""
    shape = (2, 64, 56, 56)
    inp, nat, _, _, ref = _run(shape, True, False, True)
    assert float(ref["mean"].min()) > 99.0
    # the spread survived the cast to bf16 and is tiny against the offset
    assert float(ref["var"].min()) > 0.5
    assert float((ref["var"] / ref["mean"] ** 2).max()) < 1e-3
    # the case has teeth: the naive formula in fp32 (with torch's pairwise
    # sums, kinder than any kernel's) misses the invstd bound in every channel
    rows, channels = ref["x"].shape
    bound = 0.5 * _sum_factor(rows, channels) * ref["invstd"]
    x32 = ref["x"].float()
    naive_var = (x32 * x32).mean(0) - x32.mean(0) ** 2
    naive = 1.0 / torch.sqrt(naive_var + EPS)
    assert bool(((naive.double() - ref["invstd"]).abs() > bound).all())
    _check_forward_stats(inp, nat, ref, shape)


def _stock_composition(bn, x, identity, relu):
    out = bn(x)
    if identity is not None:
        out = out + identity
    if relu:
        out = F.relu(out, inplace=True)
    return out


def _fallback_inputs(kind):
    g = torch.Generator().manual_seed(11)
    if kind == "c12":
        x = _bf16_cl(torch.randn(2, 12, 7, 7, generator=g))
    elif kind == "nchw":
        x = torch.randn(2, 64, 7, 7, generator=g).bfloat16().cuda()
    elif kind == "fp32":
        x = torch.randn(2, 64, 7, 7, generator=g).cuda().contiguous(
            memory_format=torch.channels_last)
    else:
        x = _bf16_cl(torch.randn(2, 64, 7, 7, generator=g))
    idn = torch.randn(x.shape, generator=g).to(x.dtype).cuda().contiguous(
        memory_format=torch.channels_last if kind != "nchw"
        else torch.contiguous_format)
    dy = torch.randn(x.shape, generator=g).to(x.dtype).cuda()
    return x, idn, dy


@pytest.mark.parametrize("kind", ["c12", "nchw", "fp32", "eval", "env0"])
def test_fallback_is_the_stock_path(kind, monkeypatch):
    def boom(*a, **k):
        raise AssertionError("native kernel called on a fallback case")

    monkeypatch.setattr(fused_bn._C, "bn_act_forward", boom)
    if kind == "env0":
        monkeypatch.setenv("CGX_FUSED_BN", "0")
    x, idn, dy = _fallback_inputs(kind)
    bn = nn.BatchNorm2d(x.shape[1]).cuda()
    with torch.no_grad():
        bn.weight.normal_(1.0, 0.2)
        bn.bias.normal_(0.0, 0.2)
    if kind == "eval":
        bn.eval()
    ref = copy.deepcopy(bn)
    xa, xb = (x.clone().requires_grad_(True) for _ in range(2))
    ia, ib = (idn.clone().requires_grad_(True) for _ in range(2))
    with _aten_batch_norm():
        got = bn_act(bn, xa, ia, relu=True)
        want = _stock_composition(ref, xb, ib, True)
        got.backward(dy)
        want.backward(dy)
    assert torch.equal(got, want)
    assert torch.equal(xa.grad, xb.grad) and torch.equal(ia.grad, ib.grad)
    assert torch.equal(bn.weight.grad, ref.weight.grad)
    assert torch.equal(bn.bias.grad, ref.bias.grad)
    assert torch.equal(bn.running_mean, ref.running_mean)
    assert torch.equal(bn.running_var, ref.running_var)
    assert int(bn.num_batches_tracked) == int(ref.num_batches_tracked)


def test_bn_act_runs_the_native_kernels(monkeypatch):
    """Through the module and autograd: same bits as the direct calls."""
    calls = []
    real = _C.bn_act_forward
    monkeypatch.setattr(fused_bn._C, "bn_act_forward",
                        lambda *a: calls.append(1) or real(*a))
    shape = (2, 64, 7, 7)
    inp = _make_inputs(shape, seed=5)
    direct = _native(inp, True, True)
    bn = nn.BatchNorm2d(64).cuda()
    with torch.no_grad():
        bn.weight.copy_(inp["weight"])
        bn.bias.copy_(inp["bias"])
        bn.running_mean.copy_(inp["running_mean"])
        bn.running_var.copy_(inp["running_var"])
    x = inp["x"].clone().requires_grad_(True)
    idn = inp["identity"].clone().requires_grad_(True)
    out = bn_act(bn, x, idn, relu=True)
    out.backward(inp["dy"])
    assert calls == [1, 1]  # _native() above, and this one
    assert torch.equal(out, direct["out"])
    assert torch.equal(x.grad, direct["dx"])
    assert torch.equal(idn.grad, direct["didentity"])
    assert torch.equal(bn.weight.grad, direct["dgamma"])
    assert torch.equal(bn.bias.grad, direct["dbeta"])
    assert torch.equal(bn.running_mean, direct["running_mean"])
    assert torch.equal(bn.running_var, direct["running_var"])
    assert int(bn.num_batches_tracked) == 1


def test_module_semantics_over_three_steps():
    shape = (2, 64, 7, 7)
    rows = 2 * 7 * 7
    k = _sum_factor(rows, 64)
    nat = nn.BatchNorm2d(64).cuda()
    stk = copy.deepcopy(nat)
    rm = nat.running_mean.double().cpu()
    rv = nat.running_var.double().cpu()
    rm_bound = torch.zeros_like(rm)
    rv_bound = torch.zeros_like(rv)
    for step in range(3):
        x = _make_inputs(shape, seed=100 + step)["x"]
        bn_act(nat, x, relu=True)
        with _aten_batch_norm():
            stk(x)
        x64 = _rows(x)
        mean, var = x64.mean(0), x64.var(0, unbiased=True)
        rm_bound = (1 - MOMENTUM) * rm_bound + k * (
            (1 - MOMENTUM) * rm.abs() + MOMENTUM * x64.abs().mean(0))
        rv_bound = (1 - MOMENTUM) * rv_bound + k * (
            (1 - MOMENTUM) * rv.abs() + MOMENTUM * var)
        rm = (1 - MOMENTUM) * rm + MOMENTUM * mean
        rv = (1 - MOMENTUM) * rv + MOMENTUM * var
    assert int(nat.num_batches_tracked) == int(stk.num_batches_tracked) == 3
    _check_stat("running_mean", nat.running_mean, rm, rm_bound)
    _check_stat("running_var", nat.running_var, rv, rv_bound)
    # the stock module meets the same bound, so the two are within twice it
    _check_stat("running_mean vs stock", nat.running_mean,
                stk.running_mean.double().cpu(), 2 * rm_bound)
    _check_stat("running_var vs stock", nat.running_var,
                stk.running_var.double().cpu(), 2 * rv_bound)
