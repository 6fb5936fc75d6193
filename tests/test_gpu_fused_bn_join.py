"""The residual join of two BatchNorms, relu(bn3(x3) + bn_d(xd)), against the
existing native ops composed: bn_act_forward(xd, relu=False) for the identity,
bn_act_forward(x3, identity), bn_act_backward on bn3 and then on the downsample
BatchNorm with dy = didentity.  The fused kernels keep every rounding and the
order of every sum, so everything is required bit for bit.

Stock BatchNorm calls run with the cuDNN/MIOpen switch off, as in
test_gpu_fused_bn.py.
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
from torch_cgx_amd.ops.fused_bn import bn_act  # noqa: E402

SHAPES = [(2, 64, 1, 1), (2, 64, 7, 7), (3, 256, 5, 5), (4, 2048, 7, 7),
          (2, 64, 56, 56)]
CASES = [(s, relu) for s in SHAPES for relu in (False, True)]
# the two BatchNorms differ in these too
MOM3, EPS3, MOMD, EPSD = 0.1, 1e-5, 0.2, 1e-3


def _aten_batch_norm():
    return torch.backends.cudnn.flags(enabled=False)


def _ids(case):
    (n, c, h, w), relu = case
    return f"{n}x{c}x{h}x{w}-relu{int(relu)}"


def _bf16_cl(t):
    return t.bfloat16().cuda().contiguous(memory_format=torch.channels_last)


def _operand(shape, g):
    c = shape[1]
    x = torch.randn(shape, generator=g)
    # per-channel scale and shift, so that mean and variance matter
    x = x * (0.5 + torch.rand(1, c, 1, 1, generator=g)) + torch.randn(
        1, c, 1, 1, generator=g)
    return dict(x=_bf16_cl(x),
                weight=(1.0 + 0.2 * torch.randn(c, generator=g)).cuda(),
                bias=(0.2 * torch.randn(c, generator=g)).cuda(),
                running_mean=(0.1 * torch.randn(c, generator=g)).cuda(),
                running_var=(0.5 + torch.rand(c, generator=g)).cuda())


def _make_inputs(shape, seed):
    g = torch.Generator().manual_seed(seed)
    return dict(a=_operand(shape, g), b=_operand(shape, g),
                dy=_bf16_cl(torch.randn(shape, generator=g)))


def _composed(inp, relu):
    a, b = inp["a"], inp["b"]
    rm3, rv3 = a["running_mean"].clone(), a["running_var"].clone()
    rmd, rvd = b["running_mean"].clone(), b["running_var"].clone()
    identity, meand, invstdd, _ = _C.bn_act_forward(
        b["x"], None, b["weight"], b["bias"], rmd, rvd, MOMD, EPSD, False)
    out, mean3, invstd3, mask = _C.bn_act_forward(
        a["x"], identity, a["weight"], a["bias"], rm3, rv3, MOM3, EPS3, relu)
    dx3, dgamma3, dbeta3, didentity = _C.bn_act_backward(
        inp["dy"], a["x"], mean3, invstd3, a["weight"], mask, True)
    dxd, dgammad, dbetad, _ = _C.bn_act_backward(
        didentity, b["x"], meand, invstdd, b["weight"], None, False)
    return dict(out=out, mask=mask, dx3=dx3, dxd=dxd, mean3=mean3,
                invstd3=invstd3, meand=meand, invstdd=invstdd, rm3=rm3,
                rv3=rv3, rmd=rmd, rvd=rvd, dgamma3=dgamma3, dbeta3=dbeta3,
                dgammad=dgammad, dbetad=dbetad)


def _fused(inp, relu):
    a, b = inp["a"], inp["b"]
    rm3, rv3 = a["running_mean"].clone(), a["running_var"].clone()
    rmd, rvd = b["running_mean"].clone(), b["running_var"].clone()
    out, mean3, invstd3, meand, invstdd, mask = _C.bn_act2_forward(
        a["x"], b["x"], a["weight"], a["bias"], rm3, rv3, MOM3, EPS3,
        b["weight"], b["bias"], rmd, rvd, MOMD, EPSD, relu)
    dx3, dxd, dgamma3, dbeta3, dgammad, dbetad = _C.bn_act2_backward(
        inp["dy"], a["x"], b["x"], mean3, invstd3, a["weight"], meand,
        invstdd, b["weight"], mask)
    return dict(out=out, mask=mask, dx3=dx3, dxd=dxd, mean3=mean3,
                invstd3=invstd3, meand=meand, invstdd=invstdd, rm3=rm3,
                rv3=rv3, rmd=rmd, rvd=rvd, dgamma3=dgamma3, dbeta3=dbeta3,
                dgammad=dgammad, dbetad=dbetad)


@functools.lru_cache(maxsize=None)
def _run(shape, relu):
    inp = _make_inputs(shape, seed=hash((shape, relu)) % 9973)
    want = _composed(inp, relu)
    got = _fused(inp, relu)
    again = _fused(inp, relu)
    torch.cuda.synchronize()
    return inp, want, got, again


def _same(a, b, key):
    if a is None or b is None:
        assert a is None and b is None, key
        return
    assert not bool(a.isnan().any()), key
    if a.dtype == torch.bfloat16:  # -0 and +0 are different bits
        a, b = a.view(torch.int16), b.view(torch.int16)
    assert torch.equal(a, b), key


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_bitwise_the_composed_native_ops(case):
    inp, want, got, _ = _run(*case)
    assert got["out"].is_contiguous(memory_format=torch.channels_last)
    assert got["dxd"].is_contiguous(memory_format=torch.channels_last)
    for key in want:
        _same(got[key], want[key], key)
    if case[1] and inp["dy"].numel() > 1000:
        # the case has teeth: the ReLU cuts, and the operands differ
        assert 0.1 < float((got["out"] > 0).float().mean()) < 0.9
        assert not torch.equal(got["dx3"], got["dxd"])


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_reproducible(case):
    _, _, got, again = _run(*case)
    for key in got:
        _same(got[key], again[key], key)


def _block(channels, seed):
    """(bn3, bn_d) with distinct parameters"""
    torch.manual_seed(seed)
    bns = []
    for mom, eps in ((MOM3, EPS3), (MOMD, EPSD)):
        bn = nn.BatchNorm2d(channels, eps=eps, momentum=mom).cuda()
        with torch.no_grad():
            bn.weight.normal_(1.0, 0.2)
            bn.bias.normal_(0.0, 0.2)
        bns.append(bn)
    return bns


def _stock_composition(bn, x, idn, bn_d, relu=True):
    out = bn(x) + bn_d(idn)
    return F.relu(out, inplace=True) if relu else out


def _rel_l2(a, b):
    a, b = a.detach().double(), b.detach().double()
    return float((a - b).norm() / b.norm())


def test_module_path_over_three_steps(monkeypatch):
    """Through bn_act(..., identity_bn=) and autograd: the same bits as the
    module-level composition of the native single-BatchNorm path, and the
    stock modules' results up to bf16 rounding.

    Against the stock path both sides round the same quantities to bf16, so
    elements differ only where fp32 results straddle a rounding boundary, by
    an ulp (2^-8 relative): relative L2 <= 2^-8 for the output.  In dx a ReLU
    bit may flip where the sum straddles zero, which moves one of the 6272
    elements by O(1), 1/sqrt(6272) = 0.013 each: 0.05 allows a few."""
    shape = (2, 64, 7, 7)
    calls = []
    bn3, bnd = _block(64, 1)
    ref3, refd = copy.deepcopy(bn3), copy.deepcopy(bnd)
    stk3, stkd = copy.deepcopy(bn3), copy.deepcopy(bnd)
    real = _C.bn_act2_forward
    monkeypatch.setattr(fused_bn._C, "bn_act2_forward",
                        lambda *a: calls.append(1) or real(*a))
    for step in range(3):
        inp = _make_inputs(shape, seed=200 + step)
        xs = [inp["a"]["x"].clone().requires_grad_(True) for _ in range(3)]
        ds = [inp["b"]["x"].clone().requires_grad_(True) for _ in range(3)]
        got = bn_act(bn3, xs[0], ds[0], relu=True, identity_bn=bnd)
        want = bn_act(ref3, xs[1], bn_act(refd, ds[1], relu=False))
        with _aten_batch_norm():
            stock = _stock_composition(stk3, xs[2], ds[2], stkd)
            got.backward(inp["dy"])
            want.backward(inp["dy"])
            stock.backward(inp["dy"])
        _same(got, want, "out")
        _same(xs[0].grad, xs[1].grad, "dx3")
        _same(ds[0].grad, ds[1].grad, "dxd")
        figures = (_rel_l2(got, stock), _rel_l2(xs[0].grad, xs[2].grad),
                   _rel_l2(ds[0].grad, ds[2].grad))
        print("rel L2 vs stock: out %.2e dx3 %.2e dxd %.2e" % figures)
        assert figures[0] <= 2.0 ** -8
        assert figures[1] <= 0.05 and figures[2] <= 0.05
    assert calls == [1, 1, 1]
    for new, ref, stk in ((bn3, ref3, stk3), (bnd, refd, stkd)):
        assert torch.equal(new.weight.grad, ref.weight.grad)
        assert torch.equal(new.bias.grad, ref.bias.grad)
        assert torch.equal(new.running_mean, ref.running_mean)
        assert torch.equal(new.running_var, ref.running_var)
        assert int(new.num_batches_tracked) == 3
        assert int(stk.num_batches_tracked) == 3
        # fp32 sums of 98 terms, two implementations
        torch.testing.assert_close(new.running_mean, stk.running_mean,
                                   rtol=1e-5, atol=1e-6)
        torch.testing.assert_close(new.running_var, stk.running_var,
                                   rtol=1e-5, atol=1e-6)


def _fallback_inputs(kind):
    g = torch.Generator().manual_seed(13)
    if kind == "c12":
        x = _bf16_cl(torch.randn(2, 12, 7, 7, generator=g))
    elif kind == "nchw":
        x = torch.randn(2, 64, 7, 7, generator=g).bfloat16().cuda()
    elif kind == "fp32":
        x = torch.randn(2, 64, 7, 7, generator=g).cuda().contiguous(
            memory_format=torch.channels_last)
    else:
        x = _bf16_cl(torch.randn(2, 64, 7, 7, generator=g))
    ishape = (2, 64, 1, 1) if kind == "shape" else x.shape
    idn = torch.randn(ishape, generator=g).to(x.dtype).cuda().contiguous(
        memory_format=torch.channels_last if kind != "nchw"
        else torch.contiguous_format)
    dy = torch.randn(x.shape, generator=g).to(x.dtype).cuda()
    return x, idn, dy


@pytest.mark.parametrize("kind", ["c12", "nchw", "fp32", "eval", "eval_d",
                                  "env0", "shape"])
def test_fallback_is_the_stock_path(kind, monkeypatch):
    def boom(*a, **k):
        raise AssertionError("native kernel called on a fallback case")

    monkeypatch.setattr(fused_bn._C, "bn_act_forward", boom)
    monkeypatch.setattr(fused_bn._C, "bn_act2_forward", boom)
    if kind == "env0":
        monkeypatch.setenv("CGX_FUSED_BN", "0")
    x, idn, dy = _fallback_inputs(kind)
    bn, bnd = _block(x.shape[1], 3)
    if kind == "eval":
        bn.eval()
    if kind == "eval_d":
        bnd.eval()
    ref, refd = copy.deepcopy(bn), copy.deepcopy(bnd)
    xa, xb = (x.clone().requires_grad_(True) for _ in range(2))
    ia, ib = (idn.clone().requires_grad_(True) for _ in range(2))
    with _aten_batch_norm():
        got = bn_act(bn, xa, ia, relu=True, identity_bn=bnd)
        want = _stock_composition(ref, xb, ib, refd)
        got.backward(dy)
        want.backward(dy)
    assert torch.equal(got, want)
    assert torch.equal(xa.grad, xb.grad) and torch.equal(ia.grad, ib.grad)
    for new, old in ((bn, ref), (bnd, refd)):
        assert torch.equal(new.weight.grad, old.weight.grad)
        assert torch.equal(new.bias.grad, old.bias.grad)
        assert torch.equal(new.running_mean, old.running_mean)
        assert torch.equal(new.running_var, old.running_var)
        assert int(new.num_batches_tracked) == int(old.num_batches_tracked)
