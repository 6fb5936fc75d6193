"""conv1x1s2_stats (csrc/conv1x1s2_kernels.hip) against fp64 and the stock
convolution, with the helpers and budgets of test_gpu_conv3x3_fwd.py."""

import functools
import math

import pytest
import torch
import torch.nn.functional as F
from test_gpu_conv3x3_fwd import (EPS, U, _bf16_cl, _bits, _bn, _ids,
                                  _in_poisoned_buffer, _rows, _within)
from test_gpu_conv3x3_fwd import _inputs as _inputs3x3

pytestmark = pytest.mark.gpu

from torch_cgx_amd import _C  # noqa: E402
from torch_cgx_amd.models.resnet import Bottleneck  # noqa: E402
from torch_cgx_amd.ops import fused_bn  # noqa: E402

# (batch, C, N, H, W of the input, max_workgroups); a tile is 256 output
# pixels x 256 channels, a K chunk 64 channels, the ring has two stages.
SHAPES = [(2, 64, 256, 2, 2, 0), (2, 64, 256, 5, 7, 0), (3, 128, 512, 7, 4, 0),
          (3, 256, 512, 20, 20, 0), (2, 1024, 2048, 4, 4, 0),
          (2, 2048, 256, 2, 2, 0), (5, 64, 256, 32, 32, 2),
          (16, 128, 512, 28, 28, 6)]
_plan = lambda s: _C.conv1x1s2_plan(  # noqa: E731
    s[0], s[3], s[4], s[1], s[2], s[5])


def _inputs(shape, offset=False):
    # x and the BatchNorm's parameters as the 3x3 tests draw them; with
    # `offset` x is near 1 and every output near 100, where bf16 steps by 0.5
    inp, (_, c, n, _, _, _) = _inputs3x3(shape, offset), shape
    g = torch.Generator().manual_seed(c + n)
    wt = torch.randn(n, c, 1, 1, generator=g) / math.sqrt(c)
    inp["w"] = _bf16_cl(0.5 * wt + 100.0 / c if offset else wt)
    return inp


@functools.lru_cache(maxsize=None)
def _run(shape, offset=False):
    inp = _inputs(shape, offset)
    keep = inp["x"].clone(), inp["w"].clone()
    y, part = _C.conv1x1s2_stats(inp["x"], inp["w"], shape[5])
    y2, part2 = _C.conv1x1s2_stats(inp["x"], inp["w"], shape[5])
    got = dict(y=y, part=part, y2=y2, part2=part2,
               stock=F.conv2d(inp["x"], inp["w"], stride=2),
               fused=_bn(inp, y, part), plain=_bn(inp, y, None))
    torch.cuda.synchronize()
    got["inputs_unchanged"] = (torch.equal(_bits(inp["x"]), _bits(keep[0]))
                               and torch.equal(_bits(inp["w"]), _bits(keep[1])))
    x64, w64 = inp["x"].double().cpu(), inp["w"].double().cpu()
    ref = dict(y=_rows(F.conv2d(x64, w64, stride=2)),
               mag=_rows(F.conv2d(x64.abs(), w64.abs(), stride=2)))
    return inp, got, ref


def test_shapes_reach_the_plans_they_are_for():
    plans = [_plan(s) for s in SHAPES]
    assert all(p["eligible"] for p in plans)
    assert all((p["tile_rows"], p["tile_channels"], p["k_chunk"], p["stages"])
               == (256, 256, 64, 2) for p in plans)
    assert plans[0]["rows"] == 2 and plans[0]["k_chunks"] == 1
    assert [(p["ho"], p["wo"]) for p in plans[1:3]] == [(3, 4), (4, 2)]
    assert plans[3]["rows"] == 300 and plans[3]["row_tiles"] == 2
    assert plans[3]["k_chunks"] == 4 and plans[3]["ntiles"] == 2
    assert [(plans[i]["k_chunks"], plans[i]["ntiles"]) for i in (4, 5)] == [
        (16, 8), (32, 1)]
    assert plans[6]["row_tiles"] == 5 and plans[6]["grid"] == 2
    assert plans[6]["tiles_per_split"] == 3
    assert plans[7]["row_tiles"] == 13 and plans[7]["splits"] == 3
    assert plans[7]["rows"] % 256 != 0


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_accuracy_and_against_stock(shape):
    _, got, ref = _run(shape)
    y, (b, c, n, h, w, _) = got["y"], shape
    assert tuple(y.shape) == (b, n, (h + 1) // 2, (w + 1) // 2)
    assert y.dtype == torch.bfloat16 and not bool(y.isnan().any())
    assert y.is_contiguous(memory_format=torch.channels_last)
    assert torch.equal(_bits(y), _bits(got["y2"]))
    assert torch.equal(got["part"], got["part2"]) and got["inputs_unchanged"]
    err = (_rows(y) - ref["y"]).abs()
    bound = 2.0 ** -8 * ref["y"].abs() + (c + 1) * U * ref["mag"]
    (a_abs, a_l2), (b_abs, b_l2) = (
        (d.abs().max().item(), (d.norm() / ref["y"].norm()).item())
        for d in (_rows(y) - ref["y"], _rows(got["stock"]) - ref["y"]))
    msg = (f"native max-abs {a_abs:.3e} rel-L2 {a_l2:.3e}; stock {b_abs:.3e} "
           f"{b_l2:.3e}; err/bound {(err / bound).max().item():.3f}")
    print(msg)
    assert bool((err <= bound).all()), msg
    assert a_abs <= 1.5 * b_abs and a_l2 <= 1.5 * b_l2, msg


@pytest.mark.parametrize(
    "shape,offset", [(s, False) for s in SHAPES] + [(SHAPES[7], True)])
def test_statistics(shape, offset):
    _, got, _ = _run(shape, offset)
    p, n = _plan(shape), shape[2]
    part = got["part"].double().cpu()
    assert tuple(part.shape) == (p["splits"], p["pstride"])
    y64 = _rows(got["y"])
    rows = y64.shape[0]
    if offset:
        assert 95.0 < float(y64.mean(0).min()) and float(y64.std(0).max()) < 2.0
    cnt = part[:, 2 * n:]  # every output pixel once per channel tile
    assert bool((cnt.sum(0) == rows).all()) and rows == p["rows"]
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


@pytest.mark.parametrize("shape", SHAPES[:4], ids=_ids)
def test_nothing_but_the_even_pixels_reaches_a_result(shape):
    inp, got, _ = _run(shape)
    big_x, vx = _in_poisoned_buffer(inp["x"])
    big_w, vw = _in_poisoned_buffer(inp["w"])
    assert _C.conv1x1s2_eligible(vx, vw)
    assert bool(big_x[0].isnan().all()) and bool(big_w[-1].isnan().all())
    # ... and inside the image every pixel of an odd row or column
    vx[:, :, 1::2, :] = float("nan")
    vx[:, :, :, 1::2] = float("nan")
    y, part = _C.conv1x1s2_stats(vx, vw, shape[5])
    assert bool(y.isfinite().all()) and bool(part.isfinite().all())
    assert torch.equal(_bits(y), _bits(got["y"]))
    assert torch.equal(part, got["part"])


def test_rejects_what_it_cannot_take():
    x = _bf16_cl(torch.randn(2, 128, 4, 4))
    w = _bf16_cl(torch.randn(256, 128, 1, 1))
    assert _C.conv1x1s2_eligible(x, w)
    xs = lambda c: _bf16_cl(torch.randn(2, c, 4, 4))  # noqa: E731
    ws = lambda n, c: _bf16_cl(torch.randn(n, c, 1, 1))  # noqa: E731
    bad = [(x.float(), w), (x, w.float()), (x.contiguous(), w),
           (x.cpu(), w.cpu()), (x, ws(256, 64)), (xs(32), ws(256, 32)),
           (xs(96), ws(256, 96)), (xs(4096), ws(256, 4096)), (x, ws(128, 128)),
           (x, ws(384, 128)), (x, ws(4096, 128)),
           (x, _bf16_cl(torch.randn(256, 128, 3, 3)))]
    for args in bad:
        assert not _C.conv1x1s2_eligible(*args)
        with pytest.raises(RuntimeError):
            _C.conv1x1s2_stats(*args)
    with pytest.raises(RuntimeError):
        _C.conv1x1s2_stats(x, w, -1)


_REAL = _C.conv1x1s2_stats, _C.bn_act2_forward


def _block():
    torch.manual_seed(3)
    nn = torch.nn
    return Bottleneck(256, 64, stride=2, downsample=nn.Sequential(
        nn.Conv2d(256, 256, 1, stride=2, bias=False), nn.BatchNorm2d(256)))


def _train_step(mode, monkeypatch, others="1"):
    # -> output, gradients, the kernel's (y, part) per call, the join's partd
    monkeypatch.setenv("CGX_NATIVE_CONV1X1_S2", mode)
    for name in ("CONV1X1", "CONV1X1_BWD", "CONV1X1_WRW", "CONV1X1_TILED",
                 "CONV3X3", "CONV3X3_S2"):  # the other switches
        monkeypatch.setenv("CGX_NATIVE_" + name, others)
    calls, partds = [], []

    def spy(x, w, max_workgroups=0):
        calls.append(_REAL[0](x, w, max_workgroups))
        return calls[-1]

    def spy_bn(*args):
        partds.append(args[-1])
        return _REAL[1](*args)

    monkeypatch.setattr(fused_bn._C, "conv1x1s2_stats", spy)
    monkeypatch.setattr(fused_bn._C, "bn_act2_forward", spy_bn)
    blk = _block().cuda().to(memory_format=torch.channels_last)
    g = torch.Generator().manual_seed(17)
    x = _bf16_cl(torch.randn(4, 256, 12, 12, generator=g)).requires_grad_(True)
    dy = _bf16_cl(torch.randn(4, 256, 6, 6, generator=g))
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out = blk(x)
    out.backward(dy)
    torch.cuda.synchronize()
    grads = [x.grad] + [q.grad for q in blk.parameters()]
    return out.detach(), grads, calls, partds


def test_bottleneck_routes_the_forward(monkeypatch):
    out, grads, calls, partds = _train_step("all", monkeypatch)
    out0, grads0, calls0, partds0 = _train_step("0", monkeypatch)
    assert len(calls) == len(partds) == 1 and not calls0
    assert partds[0] is calls[0][1] and partds0 == [None]
    a, b = out.double(), out0.double()
    assert a.shape == b.shape and bool(((a - b).abs() <= 2.0 ** -6 * b.abs()
                                        + 2.0 ** -7 * b.abs().max()).all())
    # gradients: against the block in fp64 at most 1.5x the stock block's error
    ref = _block().double()
    g = torch.Generator().manual_seed(17)
    x = torch.randn(4, 256, 12, 12, generator=g).bfloat16().double()
    dy = torch.randn(4, 256, 6, 6, generator=g).bfloat16().double()
    ref(x.requires_grad_(True)).backward(dy)
    for a, b, r in zip(grads, grads0, [x.grad] + [q.grad
                                                  for q in ref.parameters()]):
        ea, eb = ((t.double().cpu() - r).norm().item() / r.norm().item()
                  for t in (a, b))
        print(f"gradient {tuple(r.shape)}: native {ea:.3e} stock {eb:.3e}")
        assert a.shape == r.shape and ea <= 1.5 * eb
    assert not _train_step("0", monkeypatch, others="all")[2]
    assert len(_train_step("all", monkeypatch, others="0")[2]) == 1
    assert fused_bn.native_conv1x1_s2_mode() == "all"
    monkeypatch.setenv("CGX_FUSED_BN", "0")
    assert fused_bn.native_conv1x1_s2_mode() == "0"
    assert not _train_step("all", monkeypatch)[2]
