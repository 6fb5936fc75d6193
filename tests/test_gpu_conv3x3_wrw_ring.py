"""conv3x3_wrw_ring (csrc/conv3x3_kernels.hip), the 3x3 weight gradient through
a ring of LDS stages: bit for bit conv3x3_wrw's result where the two plans
agree on tile, hr, images and splits, and within the error budget of
test_gpu_conv3x3_wrw.py everywhere: |err| <= 2^-8 |ref| + (R+1) 2^-24 mag, one
rounding plus R = B*H*W fp32 additions in any order, mag the same sum over
absolute values; the zero pads and the zero steps past a strip add exact zeros.
"""

import functools

import pytest
import torch

pytestmark = pytest.mark.gpu

from torch_cgx_amd import _C  # noqa: E402
from torch_cgx_amd.models.resnet import Bottleneck  # noqa: E402
from torch_cgx_amd.ops import fused_bn  # noqa: E402

U = 2.0 ** -24
# (batch, C of X, N of dY, H, W, stages); SAME: the plan is conv3x3_wrw's
SAME = [(2, 64, 64, 14, 14, 2),     # chunks of a split: exactly the stages
        (3, 64, 64, 14, 14, 2),     # one more
        (5, 64, 64, 14, 14, 2),     # twice round the ring
        (1, 64, 64, 14, 14, 2),     # fewer than stages
        (2, 64, 64, 8, 56, 2),      # a long strip of a small tensor
        (64, 128, 64, 14, 14, 2)]   # eight splits, two tiles
OTHER = [(11, 128, 64, 7, 7, 2),    # 4 images a chunk, 3 in the last
         (2, 64, 128, 30, 28, 2),   # rows past the image in the last chunk
         (64, 128, 64, 14, 14, 3),  # three stages, 16 chunks a split
         (9, 64, 64, 7, 7, 3),      # exactly three chunks
         (2, 64, 64, 14, 14, 3),    # four
         (4, 128, 128, 14, 14, 3)]  # eight, four tiles
SHAPES = SAME + OTHER


def _ids(s):
    return "{}x{}to{}x{}x{}-st{}".format(*s)


def _bf16_cl(t):
    return t.bfloat16().cuda().contiguous(memory_format=torch.channels_last)


def _bits(t):
    return t.contiguous().view(torch.int16)


def _plans(shape):
    b, c, n, h, w, st = shape
    return (_C.conv3x3_wrw_ring_plan(b, h, w, c, n, 0, st),
            _C.conv3x3_wrw_plan(b, h, w, c, n))


def _reference(dy, x):
    dy64, x64 = dy.detach().double().cpu(), x.detach().double().cpu()
    size = (dy.shape[1], x.shape[1], 3, 3)
    dw = torch.nn.grad.conv2d_weight(x64, size, dy64, padding=1)
    mag = torch.nn.grad.conv2d_weight(x64.abs(), size, dy64.abs(), padding=1)
    rows = dy.shape[0] * dy.shape[2] * dy.shape[3]
    return dict(dw=dw, bound=2.0 ** -8 * dw.abs() + (rows + 1) * U * mag)


def _operands(shape):
    b, c, n, h, w, _ = shape
    g = torch.Generator().manual_seed(c * 7 + n * 3 + h)
    dy = _bf16_cl(torch.randn(b, n, h, w, generator=g) * (
        0.5 + torch.rand(1, n, 1, 1, generator=g)))
    x = _bf16_cl(torch.randn(b, c, h, w, generator=g))
    return dy, x


@functools.lru_cache(maxsize=None)
def _run(shape):
    dy, x = _operands(shape)
    keep = dy.clone(), x.clone()
    got = dict(dw=_C.conv3x3_wrw_ring(dy, x, 0, shape[5]),
               dw2=_C.conv3x3_wrw_ring(dy, x, 0, shape[5]),
               old=_C.conv3x3_wrw(dy, x))
    torch.cuda.synchronize()
    got["inputs_unchanged"] = (torch.equal(_bits(dy), _bits(keep[0]))
                               and torch.equal(_bits(x), _bits(keep[1])))
    return got, _reference(dy, x)


def test_shapes_reach_the_plans_they_are_for():
    for shape in SHAPES:
        ring, old = _plans(shape)
        assert ring["eligible"] and ring["stages"] == shape[5]
        same = all(ring[k] == old[k]
                   for k in ("bn", "bk", "hr", "images", "splits"))
        assert same == (shape in SAME), shape
    per_split = [_plans(s)[0]["chunks_per_split"] for s in SHAPES]
    assert per_split[:4] == [2, 3, 5, 1]
    assert _plans(SAME[4])[0]["strip_x"] > 300
    assert _plans(SAME[5])[0]["splits"] == 8
    p7, p30 = _plans(OTHER[0])[0], _plans(OTHER[1])[0]
    assert p7["images"] == 4 and 11 % 4 and p7["ntiles_k"] == 2
    assert p30["chunks_per_image"] >= 2 and 30 % p30["hr"]
    assert p30["ntiles_n"] == 2
    assert per_split[8:] == [16, 3, 4, 8]
    assert len(SAME) * 3 >= len(SHAPES)


@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_accuracy_bits_and_determinism(shape):
    got, ref = _run(shape)
    _, c, n, _, _, _ = shape
    dw = got["dw"]
    assert tuple(dw.shape) == (n, c, 3, 3) and dw.dtype == torch.bfloat16
    assert dw.is_contiguous(memory_format=torch.channels_last)
    worst = {}
    for name in ("dw", "old"):
        err = (got[name].double().cpu() - ref["dw"]).abs()
        worst[name] = (err / ref["bound"].clamp_min(1e-300)).max().item()
    print(f"worst error / bound: ring {worst['dw']:.3f}, conv3x3_wrw "
          f"{worst['old']:.3f}")
    assert bool(dw.isfinite().all())
    assert worst["dw"] <= 1.0
    assert torch.equal(_bits(dw), _bits(got["dw2"]))
    assert got["inputs_unchanged"]
    if shape in SAME:
        assert torch.equal(_bits(dw), _bits(got["old"]))


@pytest.mark.parametrize("shape", OTHER[:2] + SAME[4:5], ids=_ids)
def test_no_stale_factor_after_a_poisoned_call(shape):
    got, _ = _run(shape)
    big = SAME[5]
    for fill in (float("nan"), float("inf")):
        dy = _bf16_cl(torch.full((big[0], big[2], big[3], big[4]), fill))
        x = _bf16_cl(torch.full((big[0], big[1], big[3], big[4]), fill))
        _C.conv3x3_wrw_ring(dy, x, 0, shape[5])
        dy, x = _operands(shape)
        dw = _C.conv3x3_wrw_ring(dy, x, 0, shape[5])
        assert bool(dw.isfinite().all())
        assert torch.equal(_bits(dw), _bits(got["dw"]))


def test_rejects_what_it_cannot_take():
    dy = _bf16_cl(torch.randn(2, 64, 4, 4))
    x = _bf16_cl(torch.randn(2, 128, 4, 4))
    assert _C.conv3x3_wrw_ring_eligible(dy, x)
    for args in [(dy.float(), x), (dy, x.contiguous()), (dy, x[:1]),
                 (dy, _bf16_cl(torch.randn(2, 96, 4, 4))), (dy.cpu(), x.cpu())]:
        assert not _C.conv3x3_wrw_ring_eligible(*args)
        with pytest.raises(RuntimeError):
            _C.conv3x3_wrw_ring(*args)
    for bad in ((dy, x, -1), (dy, x, 0, 4)):
        with pytest.raises(RuntimeError):
            _C.conv3x3_wrw_ring(*bad)


def _train_step(mode, monkeypatch):
    """One step of a Bottleneck(256, 64) under bf16 autocast -> (block, the
    (dy, x) of every call of the ring, the calls of conv3x3_wrw)."""
    monkeypatch.setenv("CGX_NATIVE_CONV3X3_WRW_RING", mode)
    # ... with conv3x3_wrw switched on for every problem, as the path that
    # the ring takes the problem from
    monkeypatch.setenv("CGX_NATIVE_CONV3X3_WRW", "all")
    ring_calls, old_calls = [], []
    real_ring, real_old = _C.conv3x3_wrw_ring, _C.conv3x3_wrw

    def spy_ring(dy, x, *a):
        ring_calls.append((dy, x))
        return real_ring(dy, x, *a)

    def spy_old(dy, x, *a):
        old_calls.append((dy, x))
        return real_old(dy, x, *a)

    monkeypatch.setattr(fused_bn._C, "conv3x3_wrw_ring", spy_ring)
    monkeypatch.setattr(fused_bn._C, "conv3x3_wrw", spy_old)
    torch.manual_seed(3)
    blk = Bottleneck(256, 64).cuda().to(memory_format=torch.channels_last)
    g = torch.Generator().manual_seed(17)
    x = _bf16_cl(torch.randn(4, 256, 12, 12, generator=g)).requires_grad_(True)
    dy = _bf16_cl(torch.randn(4, 256, 12, 12, generator=g))
    with torch.autocast("cuda", dtype=torch.bfloat16):
        out = blk(x)
    out.backward(dy)
    torch.cuda.synchronize()
    return blk, ring_calls, old_calls


def test_routing(monkeypatch):
    off, ring_calls, old_calls = _train_step("0", monkeypatch)
    assert not ring_calls and len(old_calls) == 1   # the parent's path
    ref_off = _reference(*old_calls[0])
    on, ring_calls, old_calls = _train_step("all", monkeypatch)
    assert len(ring_calls) == 1 and not old_calls
    ref_on = _reference(*ring_calls[0])
    g_on = on.conv2.weight.grad.double().cpu()
    g_off = off.conv2.weight.grad.double().cpu()
    assert bool(((g_on - ref_on["dw"]).abs() <= ref_on["bound"]).all())
    assert bool(((g_off - ref_off["dw"]).abs() <= ref_off["bound"]).all())
    # each within the bound of the reference of the dy that reached it (what
    # runs before the convolution's backward need not repeat its bits)
    slack = (ref_on["dw"] - ref_off["dw"]).abs()
    assert bool(((g_on - g_off).abs()
                 <= ref_on["bound"] + ref_off["bound"] + slack).all())
    monkeypatch.setenv("CGX_NATIVE_CONV3X3_WRW_RING", "all")
    monkeypatch.setenv("CGX_FUSED_BN", "0")
    assert fused_bn.native_conv3x3_wrw_ring_mode() == "0"
