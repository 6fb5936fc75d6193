"""conv3x3s2_bwd_data against fp64 on the CPU and the stock gradient.  A pixel of
dX is bf16 of an fp32 sum of at most four taps of N products: |err| <= 2^-8 |ref|
+ (4N+1) 2^-24 sum|dy w|, and at most 1.5x the error of MIOpen's kernel."""

import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from torch_cgx_amd import _C  # noqa: E402
from torch_cgx_amd.models.resnet import Bottleneck  # noqa: E402
from torch_cgx_amd.ops import fused_bn  # noqa: E402
from test_gpu_conv3x3_fwd import (_bf16_cl, _bits,  # noqa: E402
                                  _in_poisoned_buffer)

# (batch, C, N, Ho, Wo, max_workgroups); why: test_conv3x3_s2_bwd_plan_cpu.py
SHAPES = [(2, 64, 64, 1, 1, 0), (2, 64, 64, 2, 3, 0), (3, 64, 128, 7, 7, 0),
          (2, 128, 64, 7, 7, 0), (2, 64, 64, 3, 28, 0),
          (2, 256, 256, 5, 5, 0), (2, 512, 512, 3, 3, 0),
          (5, 64, 64, 12, 12, 2), (32, 128, 64, 14, 14, 7)]
_ids = lambda s: "{}x{}from{}x{}x{}-wg{}".format(*s)  # noqa: E731
_REAL = _C.conv3x3s2_bwd_data


def _dx(dy, w):  # the stock input gradient, in the dtype and on the device
    (b, _, ho, wo), c = dy.shape, w.shape[1]
    x = dy.new_zeros(b, c, 2 * ho, 2 * wo).contiguous(
        memory_format=torch.channels_last)
    return torch.ops.aten.convolution_backward(
        dy, x, w, None, (2, 2), (1, 1), (1, 1), False, (0, 0), 1,
        (True, False, False))[0]


@functools.lru_cache(maxsize=None)
def _run(shape):
    b, c, n, ho, wo, wg = shape
    g = torch.Generator().manual_seed(c * 7 + n * 3 + ho)
    dy = _bf16_cl(torch.randn(b, n, ho, wo, generator=g) * (
        0.5 + torch.rand(1, n, 1, 1, generator=g)))
    wt = _bf16_cl(torch.randn(n, c, 3, 3, generator=g) * (9 * n) ** -0.5)
    keep = dy.clone(), wt.clone()
    got = dict(dx=_C.conv3x3s2_bwd_data(dy, wt, wg),
               dx2=_C.conv3x3s2_bwd_data(dy, wt, wg), stock=_dx(dy, wt))
    got["inputs_unchanged"] = (torch.equal(_bits(dy), _bits(keep[0]))
                               and torch.equal(_bits(wt), _bits(keep[1])))
    dy64, w64 = dy.double().cpu(), wt.double().cpu()
    return (dy, wt), got, _dx(dy64, w64), _dx(dy64.abs(), w64.abs())


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_accuracy_and_against_stock(shape):
    _, got, ref, mag = _run(shape)
    (b, c, n, ho, wo, _), dx = shape, got["dx"]
    assert tuple(dx.shape) == (b, c, 2 * ho, 2 * wo)
    assert dx.is_contiguous(memory_format=torch.channels_last)
    assert dx.dtype == torch.bfloat16 and got["inputs_unchanged"]
    assert not bool(dx.isnan().any())
    assert torch.equal(_bits(dx), _bits(got["dx2"]))
    err = (dx.double().cpu() - ref).abs()
    bound = 2.0 ** -8 * ref.abs() + (4 * n + 1) * 2.0 ** -24 * mag
    (a_abs, a_l2), (b_abs, b_l2) = (
        (d.abs().max().item(), (d.norm() / ref.norm()).item())
        for d in (t.double().cpu() - ref for t in (dx, got["stock"])))
    msg = (f"native max-abs {a_abs:.3e} rel-L2 {a_l2:.3e}; stock max-abs "
           f"{b_abs:.3e} rel-L2 {b_l2:.3e}; worst err/bound "
           f"{(err / bound.clamp_min(1e-300)).max().item():.3f}")
    print(msg)
    assert bool((err <= bound).all()), msg
    assert a_abs <= 1.5 * b_abs and a_l2 <= 1.5 * b_l2, msg


@pytest.mark.parametrize("shape", SHAPES[:4], ids=_ids)
def test_nothing_outside_the_tensors_reaches_a_result(shape):
    (dy, wt), got, _, _ = _run(shape)
    (big_dy, vdy), (big_w, vw) = (_in_poisoned_buffer(t) for t in (dy, wt))
    assert _C.conv3x3s2_bwd_eligible(vdy, vw)
    for big in (big_dy, big_w):
        assert bool(big[0].isnan().all()) and bool(big[-1].isnan().all())
    dx = _C.conv3x3s2_bwd_data(vdy, vw, shape[5])
    assert bool(dx.isfinite().all())
    assert torch.equal(_bits(dx), _bits(got["dx"]))


def test_rejects_what_it_cannot_take():
    dy = _bf16_cl(torch.randn(2, 64, 4, 4))
    w = _bf16_cl(torch.randn(64, 128, 3, 3))
    assert _C.conv3x3s2_bwd_eligible(dy, w)
    dys = lambda n: _bf16_cl(torch.randn(2, n, 4, 4))  # noqa: E731
    ws = lambda n, c: _bf16_cl(torch.randn(n, c, 3, 3))  # noqa: E731
    bad = [(dy.float(), w), (dy, w.float()), (dy.contiguous(), w),
           (dy, w.contiguous()), (dy.cpu(), w.cpu()), (dy, ws(128, 128)),
           (dys(32), ws(32, 128)), (dys(96), ws(96, 128)),
           (dys(1024), ws(1024, 128)), (dy, ws(64, 32)), (dy, ws(64, 96)),
           (dy, ws(64, 1024)), (dy, _bf16_cl(torch.randn(64, 128, 1, 1)))]
    for args in bad:
        assert not _C.conv3x3s2_bwd_eligible(*args)
        with pytest.raises(RuntimeError):
            _C.conv3x3s2_bwd_data(*args)
    with pytest.raises(RuntimeError):
        _C.conv3x3s2_bwd_data(dy, w, -1)


def _block():
    torch.manual_seed(3)
    nn = torch.nn
    return Bottleneck(256, 64, stride=2, downsample=nn.Sequential(
        nn.Conv2d(256, 256, 1, stride=2, bias=False), nn.BatchNorm2d(256)))


def _train_step(monkeypatch, bwd, fwd="0", stride1="1"):
    """One bf16 autocast step of the strided block -> (output, gradients, calls
    of the kernel); native 1x1 convolutions, as in test_gpu_conv3x3_bwd.py."""
    for name, mode in (("1X1", "all"), ("3X3_S2", fwd), ("3X3_BWD", stride1)):
        monkeypatch.setenv("CGX_NATIVE_CONV" + name, mode)
    if bwd is None:
        monkeypatch.delenv("CGX_NATIVE_CONV3X3_S2_BWD", raising=False)
    else:
        monkeypatch.setenv("CGX_NATIVE_CONV3X3_S2_BWD", bwd)
    calls = []
    monkeypatch.setattr(fused_bn._C, "conv3x3s2_bwd_data",
                        lambda *a: calls.append(_REAL(*a)) or calls[-1])
    blk = _block().cuda().to(memory_format=torch.channels_last)
    g = torch.Generator().manual_seed(17)
    x = _bf16_cl(torch.randn(4, 256, 12, 12, generator=g)).requires_grad_(True)
    dy = _bf16_cl(torch.randn(4, 256, 6, 6, generator=g))
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out = blk(x)
    out.backward(dy)
    torch.cuda.synchronize()
    grads = [x.grad] + [q.grad for q in blk.parameters()]
    return out.detach(), grads, len(calls)


def test_bottleneck_routes_the_input_gradient(monkeypatch):
    out, grads, calls = _train_step(monkeypatch, "all")
    out0, grads0, calls0 = _train_step(monkeypatch, "0")
    assert calls == 1 and calls0 == 0
    assert torch.equal(_bits(out), _bits(out0))  # the forward is untouched
    ref = _block().double()
    g = torch.Generator().manual_seed(17)
    x = torch.randn(4, 256, 12, 12, generator=g).bfloat16().double()
    dy = torch.randn(4, 256, 6, 6, generator=g).bfloat16().double()
    ref(x.requires_grad_(True)).backward(dy)
    for a, b, r in zip(grads, grads0, [x.grad] + [q.grad
                                                  for q in ref.parameters()]):
        ea, eb = ((t.double().cpu() - r).norm().item() / r.norm().item()
                  for t in (a, b))
        print(f"gradient {tuple(r.shape)}: rel-L2 error native {ea:.3e} "
              f"stock {eb:.3e}")
        assert a.shape == r.shape and ea <= 1.5 * eb
    # batch 4 is in no table; only its own switch and CGX_FUSED_BN reach it
    for bwd, fwd, stride1, want in (
            (None, "0", "1", 0), ("1", "0", "1", 0), ("all", "all", "1", 1),
            ("0", "all", "1", 0), ("0", "0", "all", 0), ("all", "0", "0", 1)):
        assert _train_step(monkeypatch, bwd, fwd, stride1)[2] == want
    assert fused_bn.native_conv3x3_s2_bwd_mode() == "all"
    monkeypatch.setenv("CGX_FUSED_BN", "0")
    assert fused_bn.native_conv3x3_s2_bwd_mode() == "0"
    assert _train_step(monkeypatch, "all")[2] == 0
