"""The native weight gradient of the stem, Conv2d(3, 64, 7, stride 2, padding
3) (conv_stem_wrw in csrc/conv_stem_kernels.hip), against fp64.

Error budget, as in test_gpu_conv3x3_wrw.py: |err| <= 2^-8 |ref| +
(R+1) 2^-24 mag, one rounding plus R = B*OH*OW fp32 additions in any order, mag
the same sum over absolute values; the zero pads add exact zeros, so an entry
whose window never meets the image has bound 0.
"""

import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from torch_cgx_amd import _C  # noqa: E402
from torch_cgx_amd.ops import fused_bn  # noqa: E402


def _short_last_band_height(w):
    """The smallest H cut into two or more bands, the last one short."""
    for h in range(2, 512, 2):
        p = _C.conv_stem_wrw_plan(3, h, w)
        if p["bands_per_image"] >= 2 and p["last_groups"] < p["groups"]:
            return h
    raise AssertionError("no such height")


# (batch, H, W, max_workgroups)
SHAPES = [(1, 2, 16, 0), (2, 4, 16, 0), (1, 6, 48, 0), (2, 6, 224, 0),
          (3, _short_last_band_height(32), 32, 0), (5, 16, 16, 2),
          (40, 4, 16, 0)]
SIZE = (64, 3, 7, 7)
U = 2.0 ** -24


def _ids(s):
    return "{}x{}x{}-wg{}".format(*s)


def _bf16_cl(t):
    return t.bfloat16().cuda().contiguous(memory_format=torch.channels_last)


def _bits(t):
    return t.contiguous().view(torch.int16)


def _fp64(dy, x):
    return torch.nn.grad.conv2d_weight(x.double().cpu(), SIZE,
                                       dy.double().cpu(), stride=2, padding=3)


def _reference(dy, x):
    dw, mag = _fp64(dy, x), _fp64(dy.abs(), x.abs())
    rows = dy.shape[0] * dy.shape[2] * dy.shape[3]
    return dict(dw=dw, bound=2.0 ** -8 * dw.abs() + (rows + 1) * U * mag)


def _operands(shape):
    b, h, w, _ = shape
    g = torch.Generator().manual_seed(b * 7 + h * 3 + w)
    dy = _bf16_cl(torch.randn(b, 64, h // 2, w // 2, generator=g) * (
        0.5 + torch.rand(1, 64, 1, 1, generator=g)))
    return dy, _bf16_cl(torch.randn(b, 3, h, w, generator=g))


def _stock_dw(dy, x):
    w = torch.empty(SIZE, dtype=dy.dtype, device=dy.device).contiguous(
        memory_format=torch.channels_last)
    return torch.ops.aten.convolution_backward(
        dy, x, w, None, (2, 2), (3, 3), (1, 1), False, (0, 0), 1,
        (False, True, False))[1]


@functools.lru_cache(maxsize=None)
def _run(shape):
    dy, x = _operands(shape)
    keep = dy.clone(), x.clone()
    got = dict(dw=_C.conv_stem_wrw(dy, x, shape[3]),
               dw2=_C.conv_stem_wrw(dy, x, shape[3]), stock=_stock_dw(dy, x))
    torch.cuda.synchronize()
    got["inputs_unchanged"] = (torch.equal(_bits(dy), _bits(keep[0]))
                               and torch.equal(_bits(x), _bits(keep[1])))
    return got, _reference(dy, x)


def test_shapes_reach_the_plans_they_are_for():
    plans = [_C.conv_stem_wrw_plan(*s) for s in SHAPES]
    assert all(p["eligible"] and p["lds_bytes"] <= p["lds_budget"]
               for p in plans)
    assert plans[0]["groups"] == 1 and plans[0]["steps"] == 1  # half a step
    assert plans[1]["band_rows"] == 2 and plans[1]["groups"] == 2
    assert plans[2]["groups"] % 2 == 1 and plans[2]["steps"] > 1
    assert plans[3]["groups"] == 3 * 14 and plans[3]["steps"] > 4
    assert plans[4]["bands_per_image"] >= 2                   # short last band
    assert 0 < plans[4]["last_groups"] < plans[4]["groups"]
    assert plans[5]["splits"] == 2 and plans[5]["bands"] == 5
    assert plans[5]["bands_per_split"] == 3
    assert plans[6]["splits"] == 40 and plans[6]["bands_per_split"] == 1


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_accuracy(shape):
    got, ref = _run(shape)
    dw = got["dw"]
    assert tuple(dw.shape) == SIZE and dw.dtype == torch.bfloat16
    assert dw.is_contiguous(memory_format=torch.channels_last)
    assert bool(dw.isfinite().all())
    err, stock = ((t.double().cpu() - ref["dw"]).abs()
                  for t in (dw, got["stock"]))
    worst = [(e / ref["bound"].clamp_min(1e-300)).max().item()
             for e in (err, stock)]
    print(f"worst error / bound: native {worst[0]:.3f} stock {worst[1]:.3f}")
    assert bool((err <= ref["bound"]).all())
    assert bool((dw.cpu()[ref["bound"] == 0] == 0).all())
    # reproducible, inputs untouched
    assert torch.equal(_bits(dw), _bits(got["dw2"]))
    assert got["inputs_unchanged"]


@pytest.mark.parametrize("which", ["x", "dy"])
def test_non_finite_inputs_reach_exactly_their_sums(which):
    shape = SHAPES[0]
    dy, x = _operands(shape)
    if which == "x":
        x[0, 1, -1, -1] = float("inf")
    else:
        dy[0, 5, 0, -1] = float("inf")
    bad = ~_C.conv_stem_wrw(dy, x).cpu().isfinite()
    assert torch.equal(bad, ~_fp64(dy, x).isfinite()) and bool(bad.any())
    if which == "x":
        where = torch.zeros(SIZE, dtype=torch.bool)
        where[:, 1, 4, 4] = where[:, 1, 4, 6] = True
        assert torch.equal(bad, where)


def test_no_stale_factor_after_a_poisoned_call():
    shape, big = SHAPES[2], SHAPES[3]
    got, _ = _run(shape)
    for fill in (float("nan"), float("inf")):
        _C.conv_stem_wrw(
            _bf16_cl(torch.full((big[0], 64, big[1] // 2, big[2] // 2), fill)),
            _bf16_cl(torch.full((big[0], 3, big[1], big[2]), fill)))
        dw = _C.conv_stem_wrw(*_operands(shape))
        assert bool(dw.isfinite().all())
        assert torch.equal(_bits(dw), _bits(got["dw"]))


def test_rejects_what_it_cannot_take():
    dy, x = _operands((2, 4, 16, 0))
    assert _C.conv_stem_wrw_eligible(dy, x)
    w24 = _bf16_cl(torch.randn(2, 64, 2, 12)), _bf16_cl(torch.randn(2, 3, 4, 24))
    for args in [(dy.float(), x), (dy, x.float()), (dy.contiguous(), x),
                 (dy, x.contiguous()), (dy[:1], x), (dy.cpu(), x.cpu()), w24]:
        assert not _C.conv_stem_wrw_eligible(*args)
        with pytest.raises(RuntimeError):
            _C.conv_stem_wrw(*args)
    with pytest.raises(RuntimeError):
        _C.conv_stem_wrw(dy, x, -1)


_REAL = _C.conv_stem_wrw


def _train_step(monkeypatch, wrw, fwd=None, fused=None):
    """One step of a fresh stem at 2 x 32 x 32 under bf16 autocast ->
    (conv.weight.grad, the (dy, x) of every call of the kernel)."""
    for name, value in (("CGX_NATIVE_CONV_STEM_WRW", wrw),
                        ("CGX_NATIVE_CONV_STEM", fwd), ("CGX_FUSED_BN", fused)):
        monkeypatch.setenv(name, value or "")
        if value is None:
            monkeypatch.delenv(name)
    calls = []

    def spy(dy, x, max_workgroups=0):
        calls.append((dy, x))
        return _REAL(dy, x, max_workgroups)

    monkeypatch.setattr(fused_bn._C, "conv_stem_wrw", spy)
    torch.manual_seed(5)
    conv = torch.nn.Conv2d(3, 64, 7, stride=2, padding=3, bias=False).cuda().to(
        memory_format=torch.channels_last)
    bn, pool = torch.nn.BatchNorm2d(64).cuda(), torch.nn.MaxPool2d(3, 2, 1)
    x = _bf16_cl(torch.randn(2, 3, 32, 32)).float()
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out = fused_bn.conv_stem_bn_act_pool(conv, bn, x, pool)
    out.backward(torch.randn_like(out))
    torch.cuda.synchronize()
    return conv.weight.grad, calls


def test_stem_routes_the_weight_gradient(monkeypatch):
    assert not _C.conv_stem_wrw_plan(2, 32, 32)["native"]
    for fwd in (None, "0"):  # the forward's switch does not reach it
        grad, calls = _train_step(monkeypatch, "all", fwd)
        assert len(calls) == 1
        ref = _reference(*calls[0])
        err = (grad.double().cpu() - ref["dw"]).abs()
        assert grad.shape == SIZE and bool((err <= ref["bound"]).all())
    assert not _train_step(monkeypatch, "0")[1]
    assert not _train_step(monkeypatch, None)[1]
    assert fused_bn.native_conv_stem_wrw_mode() == "1"
    assert not _train_step(monkeypatch, "all", fused="0")[1]
    assert fused_bn.native_conv_stem_wrw_mode() == "0"
