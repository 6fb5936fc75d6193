"""The native stem convolution with the BatchNorm partials of its output
(conv_stem_stats in csrc/conv_stem_kernels.hip) against fp64 on the CPU and
against the stock convolution.

Error budgets, those of test_gpu_conv3x3_fwd.py.  Y is bf16 of an fp32 sum of
147 products: |err| <= 2^-8 |ref| + 148 2^-24 sum|x w|.  The statistics are a
run of L = plan["run"] terms per lane followed by trees: |err| <= (L +
log2(R/L) + 4) 2^-24 sum|terms|, against fp64 statistics of the kernel's own
output.  The native error may be at most 1.5x that of MIOpen's convolution.
"""

import functools
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

from torch_cgx_amd import _C  # noqa: E402
from torch_cgx_amd.ops import fused_bn  # noqa: E402

# (B, H, W, max_workgroups); bands of up to 8 output rows, tiles of 32 pixels
SHAPES = [
    (2, 2, 8, 0),     # one output row: every window leaves on all four sides
    (1, 8, 8, 0),     # the smallest square image
    (2, 16, 24, 0),   # OW = 12: tiles cross output rows, inner pixels exist
    (2, 6, 224, 0),   # the real width, zero rows above and below, 10.5 tiles
    (3, 36, 24, 0),   # 18 output rows: bands of 8, 8 and 2, a short tile
    (5, 16, 16, 2),   # a band an image: workgroups of three and two bands
]
MOMENTUM, EPS, U = 0.1, 1e-5, 2.0 ** -24


def _ids(s):
    return "{}x{}x{}-wg{}".format(*s)


def _bf16_cl(t):
    return t.bfloat16().cuda().contiguous(memory_format=torch.channels_last)


def _bits(t):
    return t.contiguous().view(torch.int16)


def _rows(t):  # [B,C,H,W] -> fp64 CPU [R, C]
    return t.detach().double().cpu().permute(0, 2, 3, 1).reshape(
        -1, t.shape[1])


def _inputs(shape, offset=False):
    b, h, w, _ = shape
    g = torch.Generator().manual_seed(7 * h + w)
    if offset:
        # the centre tap carries 100, the other 48 about +-0.5: every output
        # is near 100, where bf16 has a spacing of 0.5
        x = 1.0 + 0.02 * torch.randn(b, 3, h, w, generator=g)
        wt = 0.5 * torch.randn(64, 3, 7, 7, generator=g) / math.sqrt(147)
        wt[:, :, 3, 3] += (100.0 / 3) * (1.0 + 0.01 * torch.randn(
            64, 1, generator=g))
    else:
        x = torch.randn(b, 3, h, w, generator=g) * (
            0.5 + torch.rand(1, 3, 1, 1, generator=g)) + 0.3 * torch.randn(
                1, 3, 1, 1, generator=g)
        wt = torch.randn(64, 3, 7, 7, generator=g) / math.sqrt(147)
    vec = lambda a, s: (a + s * torch.randn(64, generator=g)).cuda()  # noqa
    return dict(x=_bf16_cl(x), w=_bf16_cl(wt), weight=vec(1.0, 0.2),
                bias=vec(0.0, 0.2), running_mean=vec(0.0, 0.1),
                running_var=(0.5 + torch.rand(64, generator=g)).cuda())


def _bn_pool(inp, y, part):
    rm, rv = inp["running_mean"].clone(), inp["running_var"].clone()
    out, mean, invstd, _ = _C.bn_act_pool_forward(
        y, inp["weight"], inp["bias"], rm, rv, MOMENTUM, EPS, part)
    return dict(out=out, mean=mean, invstd=invstd)


def _ref(x, w):
    x64, w64 = x.double().cpu(), w.double().cpu()
    return dict(y=_rows(F.conv2d(x64, w64, None, 2, 3)),
                mag=_rows(F.conv2d(x64.abs(), w64.abs(), None, 2, 3)))


@functools.lru_cache(maxsize=None)
def _run(shape, offset=False):
    inp = _inputs(shape, offset)
    keep = inp["x"].clone(), inp["w"].clone()
    y, part = _C.conv_stem_stats(inp["x"], inp["w"], shape[3])
    y2, part2 = _C.conv_stem_stats(inp["x"], inp["w"], shape[3])
    got = dict(y=y, part=part, y2=y2, part2=part2,
               stock=F.conv2d(inp["x"], inp["w"], None, 2, 3),
               fused=_bn_pool(inp, y, part), plain=_bn_pool(inp, y, None))
    torch.cuda.synchronize()
    got["inputs_unchanged"] = (torch.equal(_bits(inp["x"]), _bits(keep[0]))
                               and torch.equal(_bits(inp["w"]), _bits(keep[1])))
    return inp, got, _ref(inp["x"], inp["w"])


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_accuracy_and_against_stock(shape):
    _, got, ref = _run(shape)
    b, h, w, _ = shape
    y = got["y"]
    assert (*y.shape, y.dtype) == (b, 64, h // 2, w // 2, torch.bfloat16)
    assert y.is_contiguous(memory_format=torch.channels_last)
    assert not bool(y.isnan().any()) and got["inputs_unchanged"]
    assert torch.equal(_bits(y), _bits(got["y2"])) and torch.equal(
        got["part"], got["part2"])
    err = (_rows(y) - ref["y"]).abs()
    bound = 2.0 ** -8 * ref["y"].abs() + 148 * U * ref["mag"]

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
    "shape,offset", [(s, False) for s in SHAPES] + [(s, True)
                                                    for s in SHAPES[-2:]],
    ids=lambda v: _ids(v) if isinstance(v, tuple) else f"offset{int(v)}")
def test_statistics(shape, offset):
    inp, got, _ = _run(shape, offset)
    p = _C.conv_stem_plan(*shape)
    part = got["part"].double().cpu()
    assert tuple(part.shape) == (p["splits"], p["pstride"])
    y64, rows = _rows(got["y"]), p["rows"]
    if offset:
        assert 95.0 < float(y64.mean(0).min()) and float(y64.std(0).max()) < 2.0
    cnt = part[:, 128:]
    assert float(cnt.sum()) == rows == y64.shape[0]
    # the partial rows merged in fp64 (Chan et al.)
    mean = (part[:, :64] * cnt).sum(0) / rows
    m2 = (part[:, 64:128] + cnt * (part[:, :64] - mean) ** 2).sum(0)
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
    # The pooled outputs round one affine map whose coefficients differ by k:
    # a rounding may flip, one bf16 ulp (2^-7), and the fp32 values move by k
    # of the terms' magnitude (|y| + |mean|) invstd |gamma|.
    a, b = (got[n]["out"].double().cpu() for n in ("fused", "plain"))
    scale = (invstd * inp["weight"].double().cpu().abs()).max()
    moved = 2 * k * (y64.abs().max() + want_mean.abs().max()) * scale
    assert a.shape == b.shape and bool(
        ((a - b).abs() <= 2.0 ** -7 * b.abs() + moved).all())


def _in_poisoned_buffer(t):
    b, c, h, w = t.shape
    rows, pad = b * h * w, 640
    big = torch.full((rows + 2 * pad, c), float("nan"), dtype=t.dtype,
                     device=t.device)
    view = big[pad:pad + rows].view(b, h, w, c).permute(0, 3, 1, 2)
    view.copy_(t)
    return big, view


@pytest.mark.parametrize("shape", SHAPES[:4], ids=_ids)
def test_nothing_outside_the_images_reaches_a_result(shape):
    inp, got, _ = _run(shape)
    big_x, vx = _in_poisoned_buffer(inp["x"])
    big_w, vw = _in_poisoned_buffer(inp["w"])
    assert _C.conv_stem_eligible(vx, vw)
    for big in (big_x, big_w):
        assert bool(big[0].isnan().all()) and bool(big[-1].isnan().all())
    y, part = _C.conv_stem_stats(vx, vw, shape[3])
    assert bool(y.isfinite().all()) and bool(part.isfinite().all())
    assert torch.equal(_bits(y), _bits(got["y"])) and torch.equal(
        part, got["part"])


def test_an_infinity_reaches_exactly_the_windows_that_hold_it():
    inp, _, _ = _run(SHAPES[2])
    x = inp["x"].clone()
    # Even columns: the operand of output column iw/2 - 2 holds them as
    # elements 21 .. 23 of a filter row, which only conv_stem_keep clears.
    x[0, 1, 7, 12] = x[1, 2, 9, 4] = float("inf")   # interior pixels
    x[0, 0, 7, 11] = float("inf")   # an odd column beside the first
    x[1, 0, 0, 23] = float("inf")   # a corner
    y, _ = _C.conv_stem_stats(x, inp["w"])
    want = ~_ref(x, inp["w"])["y"].isfinite()
    assert int(want.sum()) == 64 * (16 + 12 + 4) and torch.equal(
        ~_rows(y).isfinite(), want)


def test_rejects_what_it_cannot_take():
    x = _bf16_cl(torch.randn(2, 3, 8, 16))
    w = _bf16_cl(torch.randn(64, 3, 7, 7))
    assert _C.conv_stem_eligible(x, w)
    xs = lambda *s: _bf16_cl(torch.randn(*s))  # noqa: E731
    bad = [(x.float(), w), (x, w.float()), (x.contiguous(), w),
           (x, w.contiguous()), (x.cpu(), w.cpu()),
           (xs(2, 4, 8, 16), xs(64, 4, 7, 7)), (x, xs(32, 3, 7, 7)),
           (x, xs(128, 3, 7, 7)), (x, xs(64, 3, 3, 3)), (xs(2, 3, 7, 16), w),
           (xs(2, 3, 8, 12), w)]
    for args in bad:
        assert not _C.conv_stem_eligible(*args)
        with pytest.raises(RuntimeError):
            _C.conv_stem_stats(*args)
    with pytest.raises(RuntimeError):
        _C.conv_stem_stats(x, w, -1)


_REAL = _C.conv_stem_stats, _C.bn_act_pool_forward


def _stem(dtype=torch.float32):
    torch.manual_seed(5)
    conv = torch.nn.Conv2d(3, 64, 7, stride=2, padding=3, bias=False)
    bn, pool = torch.nn.BatchNorm2d(64), torch.nn.MaxPool2d(3, 2, 1)
    g = torch.Generator().manual_seed(23)
    # what the bf16 kernels see, so that fp64 computes the same function
    x = torch.randn(2, 3, 32, 32, generator=g).bfloat16().to(dtype)
    dy = torch.randn(2, 64, 8, 8, generator=g).bfloat16().to(dtype)
    with torch.no_grad():
        conv.weight.copy_(conv.weight.bfloat16())
    conv = conv.to(dtype).to(memory_format=torch.channels_last)
    return conv, bn.to(dtype), pool, x, dy


def _train_step(mode, monkeypatch):
    """One step of a fresh stem under bf16 autocast -> (output, gradients,
    the kernel's (y, part) per call, each bn_act_pool_forward's `part`)."""
    monkeypatch.setenv("CGX_NATIVE_CONV_STEM", mode or "")
    if mode is None:
        monkeypatch.delenv("CGX_NATIVE_CONV_STEM")
    calls, parts = [], []
    real, real_bn = _REAL

    def spy(x, w, max_workgroups=0):
        calls.append(real(x, w, max_workgroups))
        return calls[-1]

    def spy_bn(*args):
        parts.append(args[7])
        return real_bn(*args)

    monkeypatch.setattr(fused_bn._C, "conv_stem_stats", spy)
    monkeypatch.setattr(fused_bn._C, "bn_act_pool_forward", spy_bn)
    conv, bn, pool, x, dy = _stem()
    conv, bn = conv.cuda(), bn.cuda()
    x = x.cuda().contiguous(memory_format=torch.channels_last)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out = fused_bn.conv_stem_bn_act_pool(conv, bn, x, pool)
    out.backward(dy.cuda().bfloat16())
    torch.cuda.synchronize()
    return (out.detach(), [conv.weight.grad, bn.weight.grad, bn.bias.grad],
            calls, parts)


def test_stem_routes_the_forward(monkeypatch):
    assert not _C.conv_stem_plan(2, 32, 32)["native"]
    out, grads, calls, parts = _train_step("all", monkeypatch)
    assert len(calls) == 1 and len(parts) == 1 and parts[0] is calls[0][1]
    out0, grads0, calls0, parts0 = _train_step("0", monkeypatch)
    assert not calls0 and parts0 == [None]
    # test_bottleneck_routes_the_forward's argument with two roundings to bf16:
    # two half-ulps of 2^-8 each way, and half of it against the largest.
    a, b = out.double(), out0.double()
    tol = 2.0 ** -7 * b.abs() + 2.0 ** -8 * b.abs().max()
    assert a.shape == b.shape and bool(((a - b).abs() <= tol).all())
    # against the same stem in fp64: native error at most 1.5x the stock's
    conv, bn, pool, x, dy = _stem(torch.float64)
    pool(torch.relu(bn(conv(x)))).backward(dy)
    for a, b, r in zip(grads, grads0,
                       [conv.weight.grad, bn.weight.grad, bn.bias.grad]):
        ea, eb = ((t.double().cpu() - r).norm().item() / r.norm().item()
                  for t in (a, b))
        print(f"gradient {tuple(r.shape)}: rel-L2 error native {ea:.3e} "
              f"stock {eb:.3e}")
        assert a.shape == r.shape and ea <= 1.5 * eb
    # a bf16 input that is not 16-byte aligned goes the stock way
    monkeypatch.setenv("CGX_NATIVE_CONV_STEM", "all")
    conv, bn, pool, x, _ = _stem()
    flat = torch.zeros(x.numel() + 8, dtype=torch.bfloat16, device="cuda")
    for off in (0, 1):
        v = flat[off:off + x.numel()].view(2, 32, 32, 3).permute(0, 3, 1, 2)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            assert fused_bn._conv_stem_native(conv.cuda(), bn.cuda(), v,
                                              pool) == (off == 0)
    # the default takes only the table's problems; CGX_FUSED_BN reaches it
    assert not _train_step(None, monkeypatch)[2]
    monkeypatch.setenv("CGX_FUSED_BN", "0")
    assert fused_bn.native_conv_stem_mode() == "0"
    assert not _train_step("all", monkeypatch)[2]
