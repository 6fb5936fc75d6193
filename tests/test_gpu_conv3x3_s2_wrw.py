"""conv3x3s2_wrw against fp64 on the CPU and the stock stride-2 weight gradient.
As in test_gpu_conv3x3_wrw.py: |err| <= 2^-8 |ref| + (R+1) 2^-24 mag, one
rounding plus R = B*Ho*Wo fp32 additions in any order, mag the same sum over
absolute values, and at most 1.5x the error of MIOpen's kernel."""

import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from torch_cgx_amd import _C  # noqa: E402
from torch_cgx_amd.ops import fused_bn  # noqa: E402
from test_gpu_conv3x3_fwd import (_bf16_cl, _bits,  # noqa: E402
                                  _in_poisoned_buffer)
from test_gpu_conv3x3_s2_bwd import _block  # noqa: E402

# (batch, C, N, Ho, Wo, max_workgroups)
SHAPES = [(1, 64, 64, 1, 1, 0), (2, 64, 64, 2, 3, 0), (3, 64, 128, 7, 7, 0),
          (2, 128, 64, 7, 7, 0), (2, 64, 64, 7, 28, 0),
          (2, 256, 256, 5, 5, 0), (2, 512, 512, 3, 3, 0),
          (5, 64, 64, 12, 12, 2), (32, 128, 64, 14, 14, 0),
          (32, 128, 64, 14, 14, 7)]
_ids = lambda s: "{}x{}to{}x{}x{}-wg{}".format(*s)  # noqa: E731
_REAL = _C.conv3x3s2_wrw


def _dw(dy, x):  # the stock weight gradient, in the dtype and on the device
    w = dy.new_empty(dy.shape[1], x.shape[1], 3, 3).contiguous(
        memory_format=torch.channels_last)
    return torch.ops.aten.convolution_backward(
        dy, x, w, None, (2, 2), (1, 1), (1, 1), False, (0, 0), 1,
        (False, True, False))[1]


def _bound(dy, x):
    dy64, x64 = dy.detach().double().cpu(), x.detach().double().cpu()
    size = (dy.shape[1], x.shape[1], 3, 3)
    ref, mag = (torch.nn.grad.conv2d_weight(a, size, b, stride=2, padding=1)
                for a, b in ((x64, dy64), (x64.abs(), dy64.abs())))
    rows = dy.shape[0] * dy.shape[2] * dy.shape[3]
    return ref, 2.0 ** -8 * ref.abs() + (rows + 1) * 2.0 ** -24 * mag


@functools.lru_cache(maxsize=None)
def _run(shape):
    b, c, n, ho, wo, wg = shape
    g = torch.Generator().manual_seed(c * 7 + n * 3 + ho)
    dy = _bf16_cl(torch.randn(b, n, ho, wo, generator=g) * (
        0.5 + torch.rand(1, n, 1, 1, generator=g)))
    x = _bf16_cl(torch.randn(b, c, 2 * ho, 2 * wo, generator=g))
    keep = dy.clone(), x.clone()
    got = dict(dw=_C.conv3x3s2_wrw(dy, x, wg), dw2=_C.conv3x3s2_wrw(dy, x, wg),
               stock=_dw(dy, x))
    got["inputs_unchanged"] = (torch.equal(_bits(dy), _bits(keep[0]))
                               and torch.equal(_bits(x), _bits(keep[1])))
    return (dy, x), got, _bound(dy, x)


def test_shapes_reach_the_plans_they_are_for():
    plans = [_C.conv3x3s2_wrw_plan(b, 2 * ho, 2 * wo, c, n, wg)
             for b, c, n, ho, wo, wg in SHAPES]
    assert all(p["eligible"] for p in plans)
    assert plans[2]["images"] == 2 and plans[3]["images"] == 2  # odd batch
    assert plans[2]["chunks"] == 2
    assert plans[4]["chunks_per_image"] >= 2 and 7 % plans[4]["hr"]
    assert plans[5]["ntiles_n"] * plans[5]["ntiles_k"] == 16
    assert plans[6]["ntiles_n"] * plans[6]["ntiles_k"] == 64
    assert plans[7]["grid"] <= 2 and plans[7]["chunks_per_split"] >= 5
    assert plans[8]["splits"] == 8 and plans[8]["grid"] == 16
    assert plans[9]["splits"] == 3 and plans[9]["grid"] == 6


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_accuracy_and_against_stock(shape):
    _, got, (ref, bound) = _run(shape)
    (_, c, n, ho, wo, _), dw = shape, got["dw"]
    assert tuple(dw.shape) == (n, c, 3, 3) and dw.dtype == torch.bfloat16
    assert dw.is_contiguous(memory_format=torch.channels_last)
    assert got["inputs_unchanged"] and not bool(dw.isnan().any())
    assert torch.equal(_bits(dw), _bits(got["dw2"]))
    if (ho, wo) == (1, 1):  # the taps that only meet the padding
        assert not bool(dw[:, :, 0].any()) and not bool(dw[:, :, :, 0].any())
    err = (dw.double().cpu() - ref).abs()
    (a_abs, a_l2), (b_abs, b_l2) = (
        (d.abs().max().item(), (d.norm() / ref.norm()).item())
        for d in (t.double().cpu() - ref for t in (dw, got["stock"])))
    msg = (f"native max-abs {a_abs:.3e} rel-L2 {a_l2:.3e}; stock max-abs "
           f"{b_abs:.3e} rel-L2 {b_l2:.3e}; worst err/bound "
           f"{(err / bound.clamp_min(1e-300)).max().item():.3f}")
    print(msg)
    assert bool((err <= bound).all()), msg
    assert a_abs <= 1.5 * b_abs and a_l2 <= 1.5 * b_l2, msg


@pytest.mark.parametrize("shape", SHAPES[:4], ids=_ids)
def test_nothing_outside_the_tensors_reaches_a_result(shape):
    (dy, x), got, _ = _run(shape)
    (big_dy, vdy), (big_x, vx) = (_in_poisoned_buffer(t) for t in (dy, x))
    assert _C.conv3x3s2_wrw_eligible(vdy, vx)
    for big in (big_dy, big_x):
        assert bool(big[0].isnan().all()) and bool(big[-1].isnan().all())
    dw = _C.conv3x3s2_wrw(vdy, vx, shape[5])
    assert bool(dw.isfinite().all())
    assert torch.equal(_bits(dw), _bits(got["dw"]))


def test_rejects_what_it_cannot_take():
    dys = lambda n, b=2, s=4: _bf16_cl(torch.randn(b, n, s, s))  # noqa: E731
    xs = lambda c, h=8, w=8: _bf16_cl(torch.randn(2, c, h, w))  # noqa: E731
    dy, x = dys(64), xs(128)
    assert _C.conv3x3s2_wrw_eligible(dy, x)
    bad = [(dy.float(), x.float()), (dy.contiguous(), x), (dy, x.contiguous()),
           (dy.cpu(), x.cpu()), (dys(64, b=3), x), (dy, xs(128, 7, 8)),
           (dy, xs(128, 8, 7)), (dy, xs(128, 10, 8)), (dy, xs(128, 4, 4)),
           (dys(32), x), (dys(96), x), (dys(1024), x), (dy, xs(32)),
           (dy, xs(96)), (dy, xs(1024))]
    for args in bad:
        assert not _C.conv3x3s2_wrw_eligible(*args)
        with pytest.raises(RuntimeError):
            _C.conv3x3s2_wrw(*args)
    with pytest.raises(RuntimeError):
        _C.conv3x3s2_wrw(dy, x, -1)


def _train_step(monkeypatch, wrw, others="0"):
    """One bf16 autocast step of the strided block -> (output, block, gradients,
    (arguments, result) of the kernel's calls); `others`: the other switches."""
    for name in ("3X3_S2", "3X3_S2_BWD", "3X3_WRW", "3X3_BWD"):
        monkeypatch.setenv("CGX_NATIVE_CONV" + name, others)
    monkeypatch.setenv("CGX_NATIVE_CONV1X1", "all")
    if wrw is None:
        monkeypatch.delenv("CGX_NATIVE_CONV3X3_S2_WRW", raising=False)
    else:
        monkeypatch.setenv("CGX_NATIVE_CONV3X3_S2_WRW", wrw)
    calls = []
    monkeypatch.setattr(
        fused_bn._C, "conv3x3s2_wrw",
        lambda *a: calls.append((a, _REAL(*a))) or calls[-1][1])
    blk = _block().cuda().to(memory_format=torch.channels_last)
    g = torch.Generator().manual_seed(17)
    x = _bf16_cl(torch.randn(4, 256, 12, 12, generator=g)).requires_grad_(True)
    dy = _bf16_cl(torch.randn(4, 256, 6, 6, generator=g))
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out = blk(x)
    out.backward(dy)
    torch.cuda.synchronize()
    grads = [x.grad] + [q.grad for q in blk.parameters()]
    return out.detach(), blk, grads, calls


def test_bottleneck_routes_the_weight_gradient(monkeypatch):
    out, blk, grads, calls = _train_step(monkeypatch, "all")
    out0, _, grads0, calls0 = _train_step(monkeypatch, "0")
    assert len(calls) == 1 and not calls0
    assert torch.equal(_bits(out), _bits(out0))  # the forward is untouched
    grad = blk.conv2.weight.grad
    args, dw = calls[0]
    assert grad.dtype == torch.float32 and torch.equal(grad, dw.float())
    want, bound = _bound(*args)
    assert bool(((dw.double().cpu() - want).abs() <= bound).all())
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
    for wrw, others, want in ((None, "0", 0), ("1", "0", 0), ("0", "all", 0),
                              (None, "all", 0), ("all", "all", 1)):
        _, blk, _, calls = _train_step(monkeypatch, wrw, others)
        assert len(calls) == want and blk.conv2.weight.grad is not None
    monkeypatch.setenv("CGX_FUSED_BN", "0")
    assert fused_bn.native_conv3x3_s2_wrw_mode() == "0"
    _, blk, _, calls = _train_step(monkeypatch, "all")
    assert not calls and blk.conv2.weight.grad is not None
