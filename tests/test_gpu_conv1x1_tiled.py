"""The tiled walk of the native 1x1 convolution (conv1x1_tiled_stats and
conv1x1_tiled_bwd_data in csrc/conv1x1_kernels.hip): 256-row tiles, B staged
chunk by chunk into two LDS buffers.

Every accumulator is one chain over k in ascending order, as in the kernels
that keep B resident, so the outputs are held to the bits of
``_C.conv1x1_stats`` / ``_C.conv1x1_bwd_data``, which take every eligible
shape when called directly and are themselves held by
tests/golden/conv1x1_bits.json.  The statistics are sums in another order
(a lane's run is 32 rows per tile) and are held to the bound of
test_gpu_conv1x1_bn.py with the tiled plan's run length: |err| <= (L +
log2(R/L) + 4) 2^-24 sum|terms| against fp64 statistics of y itself.
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

# (batch, K, N, H, W, max_workgroups)
SHAPES = [
    (2, 64, 128, 7, 7, 0),      # a single K chunk
    (2, 128, 128, 1, 1, 0),     # 2 rows; the double buffer wraps once
    (3, 1024, 256, 5, 5, 0),    # 75 rows, ragged inside the first sub-tile
    (2, 1024, 256, 14, 14, 0),  # a full tile and a tail, second sub-tile ragged
    (2, 2048, 512, 3, 3, 0),    # 32 chunks
    (2, 512, 2048, 3, 3, 0),    # most channel tiles
    (2, 256, 1024, 28, 28, 3),  # capped grid: several tiles, moments carried
    # the forward instantiation with two MFMA tiles, which those leave out
    (2, 128, 64, 3, 3, 0),
]
MOMENTUM, EPS = 0.1, 1e-5
U = 2.0 ** -24


def _ids(s):
    return "{}x{}to{}x{}x{}-wg{}".format(*s)


def _bf16_cl(t):
    return t.bfloat16().cuda().contiguous(memory_format=torch.channels_last)


def _rows(t):
    """[N,C,H,W] -> fp64 CPU [R, C]"""
    return t.detach().double().cpu().permute(0, 2, 3, 1).reshape(
        -1, t.shape[1])


def _bits(a, b):
    return (a.shape == b.shape and a.dtype == b.dtype == torch.bfloat16
            and torch.equal(a.view(torch.int16), b.view(torch.int16)))


def _inputs(shape, offset=False):
    """The inputs of test_gpu_conv1x1_bn.py, and a dy and a skip gradient."""
    b, k, n, h, w, _ = shape
    g = torch.Generator().manual_seed(k * 7 + n * 3 + h)
    if offset:
        # every output is 100 +- about 1.3, where bf16 has a spacing of 0.5
        x = 1.0 + 0.1 * torch.randn(b, k, h, w, generator=g)
        wt = (100.0 / k) * (1.0 + 0.01 * torch.randn(n, 1, 1, 1, generator=g)) \
            * torch.ones(n, k, 1, 1)
    else:
        x = torch.randn(b, k, h, w, generator=g) * (
            0.5 + torch.rand(1, k, 1, 1, generator=g)) + 0.3 * torch.randn(
                1, k, 1, 1, generator=g)
        wt = torch.randn(n, k, 1, 1, generator=g) / math.sqrt(k)
    return dict(
        x=_bf16_cl(x), w=wt.bfloat16().cuda(),
        weight=(1.0 + 0.2 * torch.randn(n, generator=g)).cuda(),
        bias=(0.2 * torch.randn(n, generator=g)).cuda(),
        running_mean=(0.1 * torch.randn(n, generator=g)).cuda(),
        running_var=(0.5 + torch.rand(n, generator=g)).cuda(),
        dy=_bf16_cl(torch.randn(b, n, h, w, generator=g)),
        skip=_bf16_cl(torch.randn(b, k, h, w, generator=g)))


@functools.lru_cache(maxsize=None)
def _run(shape, offset=False):
    inp = _inputs(shape, offset)
    wg = shape[5]
    got = {}
    got["y"], got["part"] = _C.conv1x1_tiled_stats(inp["x"], inp["w"], wg)
    got["y2"], got["part2"] = _C.conv1x1_tiled_stats(inp["x"], inp["w"], wg)
    got["y_old"], _ = _C.conv1x1_stats(inp["x"], inp["w"])
    rm, rv = inp["running_mean"].clone(), inp["running_var"].clone()
    _, mean, invstd, _ = _C.bn_act_forward(
        got["y"], None, inp["weight"], inp["bias"], rm, rv, MOMENTUM, EPS,
        True, got["part"])
    got["bn"] = dict(mean=mean, invstd=invstd, running_mean=rm,
                     running_var=rv)
    for name, s in (("plain", None), ("add", inp["skip"])):
        got["dx_" + name] = _C.conv1x1_tiled_bwd_data(inp["dy"], inp["w"], s,
                                                      wg)
        got["dx_" + name + "2"] = _C.conv1x1_tiled_bwd_data(
            inp["dy"], inp["w"], s, wg)
        got["dx_" + name + "_old"] = _C.conv1x1_bwd_data(inp["dy"], inp["w"],
                                                         s)
    torch.cuda.synchronize()
    return inp, got


def _plan(shape):
    b, k, n, h, w, wg = shape
    return _C.conv1x1_tiled_plan(b * h * w, k, n, wg)


def _bwd_plan(shape, add):
    b, k, n, h, w, wg = shape
    return _C.conv1x1_tiled_bwd_plan(b * h * w, k, n, add, wg)


def test_shapes_reach_every_instantiation():
    fwd, bwd = set(), set()
    for s in SHAPES:
        p = _plan(s)
        assert p["eligible"] and p["k_chunk"] == 64 and not p["resident"]
        fwd.add(p["mfma_tiles"])
        for add in (False, True):
            q = _bwd_plan(s, add)
            assert q["eligible"] and q["k_chunk"] == 64
            bwd.add((q["mfma_tiles"], add))
    # conv1x1_tiled_stats<2 | 4>, conv1x1_tiled_bwd_data<2 | 4, add or not>
    assert fwd == {2, 4}
    assert bwd == {(nt, add) for nt in (2, 4) for add in (False, True)}
    assert _plan(SHAPES[0])["k_chunks"] == 1
    assert _plan(SHAPES[1])["k_chunks"] == 2
    assert _plan(SHAPES[3])["row_tiles"] == 2
    assert _plan(SHAPES[4])["k_chunks"] == 32
    assert _plan(SHAPES[5])["ntiles"] == 16
    p = _plan(SHAPES[6])
    assert p["grid"] <= 8 and p["tiles_per_split"] >= 4


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_forward_has_the_bits_of_conv1x1_stats(shape):
    _, got = _run(shape)
    assert got["y"].is_contiguous(memory_format=torch.channels_last)
    assert not bool(got["y"].isnan().any())
    assert _bits(got["y"], got["y_old"])


@pytest.mark.parametrize("add", ["plain", "add"])
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_backward_data_has_the_bits_of_conv1x1_bwd_data(shape, add):
    _, got = _run(shape)
    dx = got["dx_" + add]
    assert dx.is_contiguous(memory_format=torch.channels_last)
    assert not bool(dx.isnan().any())
    assert _bits(dx, got["dx_" + add + "_old"])


def _check_stat(name, got, want, bound):
    err = (got.double().cpu() - want).abs()
    worst = (err / bound.clamp_min(1e-300)).max().item()
    msg = f"{name}: max err {err.max().item():.3e}, worst err/bound {worst:.3f}"
    print(msg)
    assert bool((err <= bound).all()), msg


def _check_stats(shape, inp, y, bn):
    """_check_stats of test_gpu_conv1x1_bn.py with the tiled plan's run."""
    rows = y.numel() // y.shape[1]
    run = _plan(shape)["run"]
    k = (run + math.log2(rows / run) + 4) * U
    y64 = _rows(y)
    mean, var = y64.mean(0), y64.var(0, unbiased=False)
    invstd = 1.0 / torch.sqrt(var + EPS)
    abs_mean = y64.abs().mean(0)
    _check_stat("mean", bn["mean"], mean, k * abs_mean)
    _check_stat("invstd", bn["invstd"], invstd, 0.5 * k * invstd)
    rm0 = inp["running_mean"].double().cpu()
    rv0 = inp["running_var"].double().cpu()
    unbiased = var * rows / (rows - 1)
    _check_stat("running_mean", bn["running_mean"],
                (1 - MOMENTUM) * rm0 + MOMENTUM * mean,
                k * ((1 - MOMENTUM) * rm0.abs() + MOMENTUM * abs_mean))
    _check_stat("running_var", bn["running_var"],
                (1 - MOMENTUM) * rv0 + MOMENTUM * unbiased,
                k * ((1 - MOMENTUM) * rv0.abs() + MOMENTUM * unbiased))


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_statistics(shape):
    inp, got = _run(shape)
    part, p = got["part"], _plan(shape)
    assert tuple(part.shape) == (p["splits"], p["partial_stride"])
    rows = got["y"].numel() // got["y"].shape[1]
    cnt = part[:, 2 * shape[2]:].double().sum(0).cpu()
    assert cnt.numel() == p["ntiles"] and bool((cnt == rows).all())
    _check_stats(shape, inp, got["y"], got["bn"])


def test_mean_offset():
    """Outputs near 100 with unit spread, as in test_gpu_conv1x1_bn.py."""
    shape = SHAPES[6]
    inp, got = _run(shape, True)
    y64 = _rows(got["y"])
    mean, var = y64.mean(0), y64.var(0, unbiased=False)
    assert float(mean.min()) > 95.0 and float(mean.max()) < 105.0
    # spread 100 * 0.1 / sqrt(K) = 0.625 at K = 256, far below the mean
    assert float(var.min()) > 0.25
    assert float((var / mean ** 2).max()) < 1e-3
    assert _bits(got["y"], got["y_old"])
    _check_stats(shape, inp, got["y"], got["bn"])


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_reproducible(shape):
    _, got = _run(shape)
    assert not bool(got["part"].isnan().any())
    assert _bits(got["y"], got["y2"])
    assert torch.equal(got["part"], got["part2"])
    for add in ("plain", "add"):
        assert _bits(got["dx_" + add], got["dx_" + add + "2"])


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
def calls(monkeypatch):
    """How often each of the four entry points is called; for the two
    backward-data ones, how often with a skip gradient."""
    seen = {}

    def spy(name):
        real = getattr(_C, name)

        def f(*a, **k):
            seen[name] = seen.get(name, 0) + 1
            if "bwd" in name and len(a) > 2 and a[2] is not None:
                seen[name + "+skip"] = seen.get(name + "+skip", 0) + 1
            return real(*a, **k)

        monkeypatch.setattr(fused_bn._C, name, f)

    for name in ("conv1x1_stats", "conv1x1_bwd_data", "conv1x1_tiled_stats",
                 "conv1x1_tiled_bwd_data"):
        spy(name)
    return seen


def _train_step(blk, x, dy, env, monkeypatch):
    for name, value in env.items():
        monkeypatch.setenv(name, value)
    blk = copy.deepcopy(blk).cuda().to(memory_format=torch.channels_last)
    x = x.clone().requires_grad_(True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out = blk(x)
    out.backward(dy)
    torch.cuda.synchronize()
    return blk, out.detach(), x.grad


def _errors(got, want):
    d = got - want
    return d.abs().max().item(), (d.norm() / want.norm().clamp_min(1e-300)).item()


def _data(downsample):
    g = torch.Generator().manual_seed(17)
    x = _bf16_cl(torch.randn(4, 64 if downsample else 256, 12, 12,
                             generator=g))
    dy = _bf16_cl(torch.randn(4, 256, 12, 12, generator=g))
    return x, dy


@pytest.mark.parametrize("downsample", [False, True], ids=["plain", "down"])
def test_bottleneck_routes_to_the_tiled_kernels(downsample, calls,
                                                monkeypatch):
    """CGX_NATIVE_CONV1X1_TILED=all against 0, both against the block in fp64
    by the rule of test_gpu_conv1x1_bwd.py: 1.5x the error of the
    switched-off run."""
    blk = _block(downsample)
    x, dy = _data(downsample)
    nconv = 3 if downsample else 2
    on, out_on, dx_on = _train_step(
        blk, x, dy, {"CGX_NATIVE_CONV1X1_TILED": "all"}, monkeypatch)
    assert calls == {"conv1x1_tiled_stats": nconv,
                     "conv1x1_tiled_bwd_data": nconv,
                     "conv1x1_tiled_bwd_data+skip": 1}
    calls.clear()
    off, out_off, dx_off = _train_step(
        blk, x, dy, {"CGX_NATIVE_CONV1X1_TILED": "0"}, monkeypatch)
    assert not any("tiled" in name for name in calls)

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


@pytest.mark.parametrize("env", [
    {"CGX_NATIVE_CONV1X1_TILED": "0"},
    {"CGX_NATIVE_CONV1X1_TILED": "all", "CGX_NATIVE_CONV1X1": "0"},
    {"CGX_NATIVE_CONV1X1_TILED": "all", "CGX_FUSED_BN": "0"},
    {"CGX_NATIVE_CONV1X1_TILED": "1"},  # the tables list no row count so small
], ids=["tiled0", "fwd0", "bn_off", "plan"])
def test_switched_off_never_calls_the_tiled_kernels(env, calls, monkeypatch):
    x, dy = _data(True)
    _train_step(_block(True), x, dy, env, monkeypatch)
    assert not any("tiled" in name for name in calls)


def test_backward_switch_holds_the_tiled_backward_data(calls, monkeypatch):
    x, dy = _data(False)
    _train_step(_block(False), x, dy,
                {"CGX_NATIVE_CONV1X1_TILED": "all",
                 "CGX_NATIVE_CONV1X1_BWD": "0"}, monkeypatch)
    assert calls == {"conv1x1_tiled_stats": 2}
