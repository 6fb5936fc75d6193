"""The native backward-data GEMM of the 1x1 convolution, which can add the
skip gradient of a residual fork in its epilogue (conv1x1_bwd_data in
csrc/conv1x1_kernels.hip), against fp64 and against the stock path.

Error budget.  dX is bf16 of an fp32-accumulated sum of N products and, with a
skip gradient, one more term: |err| <= 2^-8 |ref| + (N+2) 2^-24 (sum_n |dy_n
w_n| + |skip|), the first term the one rounding, the second N+1 fp32 additions
in any order.  MIOpen's backward-data followed by a bf16 add is the yardstick
as in test_gpu_conv1x1_bn.py: the native error may be at most 1.5x its error.
"""

import copy
import functools
import math

import pytest
import torch
import torch.nn as nn

pytestmark = pytest.mark.gpu

from torch_cgx_amd import _C  # noqa: E402
from torch_cgx_amd.models.resnet import Bottleneck  # noqa: E402
from torch_cgx_amd.ops import fused_bn  # noqa: E402

# (batch, K of dX, N of dY, H, W, max_workgroups)
SHAPES = [(2, 64, 64, 1, 1, 0), (2, 256, 64, 7, 7, 0), (3, 64, 256, 5, 5, 0),
          (2, 128, 256, 5, 5, 0), (2, 512, 128, 9, 9, 0),
          (2, 512, 2048, 3, 3, 0), (2, 2048, 512, 3, 3, 0),
          (2, 256, 64, 56, 56, 0), (2, 256, 64, 28, 28, 3),
          # the instantiations the shapes above leave out, and a W^T tile that
          # fills the LDS to its last byte
          (2, 128, 64, 3, 3, 0), (2, 64, 2048, 3, 3, 0),
          (2, 128, 2048, 3, 3, 0), (2, 256, 256, 3, 3, 0)]
U = 2.0 ** -24


def _ids(s):
    return "{}x{}from{}x{}x{}-wg{}".format(*s)


def _bf16_cl(t):
    return t.bfloat16().cuda().contiguous(memory_format=torch.channels_last)


def _rows(t):
    """[N,C,H,W] -> fp64 CPU [R, C]"""
    return t.detach().double().cpu().permute(0, 2, 3, 1).reshape(
        -1, t.shape[1])


def _errors(got, want):
    d = got - want
    return d.abs().max().item(), (d.norm() / want.norm().clamp_min(1e-300)).item()


def _stock_dx(dy, w, x_like):
    return torch.ops.aten.convolution_backward(
        dy, x_like, w, None, (1, 1), (0, 0), (1, 1), False, (0, 0), 1,
        (True, False, False))[0]


@functools.lru_cache(maxsize=None)
def _run(shape):
    b, k, n, h, w, wg = shape
    g = torch.Generator().manual_seed(k * 7 + n * 3 + h)
    dy = _bf16_cl(torch.randn(b, n, h, w, generator=g) * (
        0.5 + torch.rand(1, n, 1, 1, generator=g)))
    wt = (torch.randn(n, k, 1, 1, generator=g) / math.sqrt(n)).bfloat16().cuda()
    skip = _bf16_cl(torch.randn(b, k, h, w, generator=g))
    keep = skip.clone()
    got = {}
    for name, s in (("plain", None), ("add", skip)):
        got[name] = _C.conv1x1_bwd_data(dy, wt, s, wg)
        got[name + "2"] = _C.conv1x1_bwd_data(dy, wt, s, wg)
    stock = _stock_dx(dy, wt, skip)
    got["stock_plain"], got["stock_add"] = stock, stock + skip
    torch.cuda.synchronize()
    got["skip_unchanged"] = torch.equal(skip.view(torch.int16),
                                        keep.view(torch.int16))
    dy64, w64, s64 = _rows(dy), wt.double().cpu().flatten(1), _rows(skip)
    ref = dict(plain=dy64 @ w64, mag_plain=dy64.abs() @ w64.abs())
    ref["add"] = ref["plain"] + s64
    ref["mag_add"] = ref["mag_plain"] + s64.abs()
    return got, ref


def _plan(shape, add=False):
    b, k, n, h, w, wg = shape
    return _C.conv1x1_bwd_plan(b * h * w, k, n, add, wg)


def test_shapes_reach_every_instantiation():
    seen = set()
    for s in SHAPES:
        p = _plan(s)
        assert p["eligible"]
        seen.add((p["mfma_tiles"], p["k_chunk"], p["resident"]))
    # with and without the add, each of them
    assert seen == {(nt, 64, True) for nt in (2, 4, 8)} | {
        (nt, 128, res) for nt in (2, 4, 8) for res in (True, False)}
    assert _plan(SHAPES[0])["row_tiles"] == 1               # two rows
    assert _plan(SHAPES[1])["row_tiles"] == 1               # a lone tail tile
    assert _plan(SHAPES[6])["ntiles"] == 8                  # channel tiling
    assert not _plan(SHAPES[6])["resident"]
    assert _plan(SHAPES[7])["grid"] > 1                     # many workgroups
    p = _plan(SHAPES[8])
    assert p["grid"] == 3 and p["tiles_per_split"] >= 4
    assert _plan(SHAPES[12])["lds_bytes"] == 160 * 1024


@pytest.mark.parametrize("add", ["plain", "add"])
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_accuracy(shape, add):
    got, ref = _run(shape)
    b, k, n, h, w, _ = shape
    dx = got[add]
    assert tuple(dx.shape) == (b, k, h, w) and dx.dtype == torch.bfloat16
    assert dx.is_contiguous(memory_format=torch.channels_last)
    err = (_rows(dx) - ref[add]).abs()
    bound = 2.0 ** -8 * ref[add].abs() + (n + 2) * U * ref["mag_" + add]
    worst = (err / bound.clamp_min(1e-300)).max().item()
    print(f"worst error / bound {worst:.3f}")
    assert bool((err <= bound).all())


@pytest.mark.parametrize("add", ["plain", "add"])
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_against_stock(shape, add):
    got, ref = _run(shape)
    a_abs, a_l2 = _errors(_rows(got[add]), ref[add])
    b_abs, b_l2 = _errors(_rows(got["stock_" + add]), ref[add])
    msg = (f"native max-abs {a_abs:.3e} rel-L2 {a_l2:.3e}; stock max-abs "
           f"{b_abs:.3e} rel-L2 {b_l2:.3e}")
    print(msg)
    assert a_abs <= 1.5 * b_abs, msg
    assert a_l2 <= 1.5 * b_l2, msg


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_reproducible_and_skip_untouched(shape):
    got, _ = _run(shape)
    for add in ("plain", "add"):
        assert not bool(got[add].isnan().any())
        assert torch.equal(got[add].view(torch.int16),
                           got[add + "2"].view(torch.int16))
    assert got["skip_unchanged"]


def test_rejects_what_it_cannot_take():
    dy = _bf16_cl(torch.randn(2, 64, 4, 4))
    w = torch.randn(64, 128, 1, 1).bfloat16().cuda()
    skip = _bf16_cl(torch.randn(2, 128, 4, 4))
    assert _C.conv1x1_bwd_eligible(dy, w, skip)
    assert _C.conv1x1_bwd_eligible(dy, w)
    bad = [(dy.float(), w, None), (dy.contiguous(), w, None),
           (dy, w.float(), None), (dy, w, skip.float()),
           (dy, w, skip.contiguous()), (dy, w, skip[:, :64]),
           (dy, w, _bf16_cl(torch.randn(2, 128, 4, 5))),
           (dy, torch.randn(32, 128, 1, 1).bfloat16().cuda(), None)]
    for args in bad:
        assert not _C.conv1x1_bwd_eligible(*args)
        with pytest.raises(RuntimeError):
            _C.conv1x1_bwd_data(*args)


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


@pytest.fixture
def bwd_calls(monkeypatch):
    """The skip argument of every _C.conv1x1_bwd_data call."""
    calls = []
    real = _C.conv1x1_bwd_data

    def spy(dy, weight, skip=None, max_workgroups=0):
        calls.append(skip)
        return real(dy, weight, skip, max_workgroups)

    monkeypatch.setattr(fused_bn._C, "conv1x1_bwd_data", spy)
    return calls


def _train_step(blk, x, dy, mode, monkeypatch):
    monkeypatch.setenv("CGX_NATIVE_CONV1X1_BWD", mode)
    blk = copy.deepcopy(blk).cuda().to(memory_format=torch.channels_last)
    x = x.clone().requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out = blk(x)
    out.backward(dy)
    torch.cuda.synchronize()
    return blk, out.detach(), x.grad


@pytest.mark.parametrize("forward", ["1", "all"])
@pytest.mark.parametrize("downsample", [False, True], ids=["plain", "down"])
def test_bottleneck_matches_the_stock_backward(downsample, forward, bwd_calls,
                                               monkeypatch):
    """One training step with every eligible backward-data native against
    CGX_NATIVE_CONV1X1_BWD=0, both against the block in fp64: 1.5x the error
    of the stock path, with the forward convolutions stock ("1": none of
    these shapes is in the plan's table) or native ("all")."""
    monkeypatch.setenv("CGX_NATIVE_CONV1X1", forward)
    blk = _block(downsample)
    g = torch.Generator().manual_seed(17)
    cin = 64 if downsample else 256
    x = _bf16_cl(torch.randn(4, cin, 12, 12, generator=g))
    dy = _bf16_cl(torch.randn(4, 256, 12, 12, generator=g))
    on, out_on, dx_on = _train_step(blk, x, dy, "all", monkeypatch)
    assert len(bwd_calls) == (3 if downsample else 2)
    assert sum(s is not None for s in bwd_calls) == 1
    off, out_off, dx_off = _train_step(blk, x, dy, "0", monkeypatch)
    assert len(bwd_calls) == (3 if downsample else 2)

    ref = copy.deepcopy(blk).double()
    x64 = x.detach().double().cpu().requires_grad_(True)
    out64 = ref(x64)
    out64.backward(dy.double().cpu())
    out64 = out64.detach()

    def check(name, a, b, want):
        a_abs, a_l2 = _errors(a.double().cpu(), want)
        b_abs, b_l2 = _errors(b.double().cpu(), want)
        msg = (f"{name}: all max-abs {a_abs:.3e} rel-L2 {a_l2:.3e}; 0 "
               f"max-abs {b_abs:.3e} rel-L2 {b_l2:.3e}")
        print(msg)
        assert a_abs <= 1.5 * b_abs, msg
        assert a_l2 <= 1.5 * b_l2, msg

    check("out", out_on, out_off, out64)
    check("dx", dx_on, dx_off, x64.grad)
    pon, poff, pref = (dict(m.named_parameters()) for m in (on, off, ref))
    for name, want in pref.items():
        check(name, pon[name].grad, poff[name].grad, want.grad)
    bon, boff, bref = (dict(m.named_buffers()) for m in (on, off, ref))
    for name, want in bref.items():
        if name.endswith("num_batches_tracked"):
            assert int(bon[name]) == int(boff[name]) == int(want) == 1, name
        else:
            check(name, bon[name], boff[name], want)


def _conv_bn(k, n):
    torch.manual_seed(5)
    conv = nn.Conv2d(k, n, 1, bias=False).cuda().to(
        memory_format=torch.channels_last)
    return conv, nn.BatchNorm2d(n).cuda()


def test_fork_with_its_second_output_unused(bwd_calls, monkeypatch):
    monkeypatch.setenv("CGX_NATIVE_CONV1X1_BWD", "all")
    conv, bn = _conv_bn(128, 64)
    g = torch.Generator().manual_seed(31)
    x = _bf16_cl(torch.randn(2, 128, 6, 6, generator=g)).requires_grad_(True)
    dy = _bf16_cl(torch.randn(2, 64, 6, 6, generator=g))
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out, skip = fused_bn.conv_bn_act_fork(conv, bn, x)
    assert skip is not x and torch.equal(skip, x)
    out.backward(dy)
    assert bwd_calls == [None]
    assert x.grad.shape == x.shape and not bool(x.grad.isnan().any())
    assert conv.weight.grad.dtype == torch.float32


def _close(a, b):
    """A bf16 ulp of the element plus 2^-9 of the tensor's maximum: the
    tolerance of test_ineligible_runs_the_stock_convolution."""
    assert a.dtype == b.dtype and a.shape == b.shape
    a, b = a.double(), b.double()
    tol = 2.0 ** -7 * b.abs() + 2.0 ** -9 * b.abs().max()
    return bool(((a - b).abs() <= tol).all())


def test_fork_with_a_skip_gradient_that_is_not_channels_last(bwd_calls,
                                                             monkeypatch):
    """The stock backward-data plus `+`, against the graph without the fork."""
    conv, bn = _conv_bn(128, 64)
    conv2, bn2 = copy.deepcopy(conv), copy.deepcopy(bn)
    g = torch.Generator().manual_seed(37)
    x = _bf16_cl(torch.randn(2, 128, 6, 6, generator=g))
    dy = _bf16_cl(torch.randn(2, 64, 6, 6, generator=g))
    ds = torch.randn(2, 128, 6, 6, generator=g).bfloat16().cuda()
    seen = []

    def loss(out, skip):
        # a skip path whose gradient arrives as `ds`, in ds's NCHW layout
        skip.register_hook(lambda grad: seen.append(grad))
        return (out * dy).sum().float() + (skip * ds).sum().float()

    xa, xb = (x.clone().requires_grad_(True) for _ in range(2))
    with torch.autocast("cuda", dtype=torch.bfloat16):
        monkeypatch.setenv("CGX_NATIVE_CONV1X1_BWD", "all")
        out, skip = fused_bn.conv_bn_act_fork(conv, bn, xa)
        assert skip is not xa
        loss(out, skip).backward()
        assert not seen[0].is_contiguous(memory_format=torch.channels_last)
        monkeypatch.setenv("CGX_NATIVE_CONV1X1_BWD", "0")
        out2, skip2 = fused_bn.conv_bn_act_fork(conv2, bn2, xb)
        assert skip2 is xb
        loss(out2, skip2).backward()
    assert bwd_calls == []
    assert torch.equal(out, out2)
    assert _close(xa.grad, xb.grad)
    assert _close(conv.weight.grad, conv2.weight.grad)


def test_an_fp32_skip_gradient_is_added_by_the_stock_path(bwd_calls,
                                                          monkeypatch):
    """Autograd hands a bf16 tensor a bf16 gradient, so this one goes to the
    backward's own decision directly."""
    monkeypatch.setenv("CGX_NATIVE_CONV1X1_BWD", "all")
    g = torch.Generator().manual_seed(41)
    x = _bf16_cl(torch.randn(2, 128, 6, 6, generator=g))
    dy = _bf16_cl(torch.randn(2, 64, 6, 6, generator=g))
    w = (torch.randn(64, 128, 1, 1, generator=g) / 8.0).bfloat16().cuda()
    ds = _bf16_cl(torch.randn(2, 128, 6, 6, generator=g)).float()
    got = fused_bn._conv1x1_dx(dy, x, w, ds)
    assert bwd_calls == []
    assert _close(got, _stock_dx(dy, w, x) + ds)
    # ... and the same call with a gradient the kernel takes does reach it
    fused_bn._conv1x1_dx(dy, x, w, ds.bfloat16())
    assert len(bwd_calls) == 1 and bwd_calls[0] is not None


@pytest.mark.parametrize("kind", ["eval", "no_grad", "env0", "fwd0", "bn_off"])
def test_no_fork(kind, bwd_calls, monkeypatch):
    monkeypatch.setenv("CGX_NATIVE_CONV1X1_BWD", "0" if kind == "env0" else "all")
    if kind == "fwd0":
        monkeypatch.setenv("CGX_NATIVE_CONV1X1", "0")
    if kind == "bn_off":
        monkeypatch.setenv("CGX_FUSED_BN", "0")
    conv, bn = _conv_bn(128, 64)
    if kind == "eval":
        bn.eval()
    x = _bf16_cl(torch.randn(2, 128, 6, 6)).requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        if kind == "no_grad":
            with torch.no_grad():
                out, skip = fused_bn.conv_bn_act_fork(conv, bn, x)
        else:
            out, skip = fused_bn.conv_bn_act_fork(conv, bn, x)
            (out.float().sum() + skip.float().sum()).backward()
    assert skip is x
    assert bwd_calls == []
