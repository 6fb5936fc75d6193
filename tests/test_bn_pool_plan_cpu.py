"""Stem BatchNorm + ReLU + 3x3/2/1 max-pool: the pooling geometry the kernels
index with (csrc/bn_plan.h), replayed without a GPU, and a torch model of the
argmax-byte forward and the gather backward against max_pool2d's autograd."""

import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

from torch_cgx_amd import _C
from torch_cgx_amd.ops.fused_bn import bn_act_pool

# (h, w) of the GPU test's shapes and of the benchmark's stem
IMAGES = [(8, 8), (7, 9), (2, 2), (30, 30), (112, 112), (1, 1), (1, 5)]
NONE = 9  # the reserved byte: no gradient


def _pooled(n):
    return (n - 1) // 2 + 1


@pytest.mark.parametrize("h,w", IMAGES)
def test_windows_list_exactly_the_in_bounds_pixels(h, w):
    windows, _ = _C.bn_pool_geometry(h, w)
    oh, ow = _pooled(h), _pooled(w)
    assert (oh, ow) == tuple(F.max_pool2d(torch.zeros(1, 1, h, w), 3, 2,
                                          1).shape[2:])
    assert windows.shape == (oh * ow, 9)
    want = torch.full((oh * ow, 9), -1, dtype=torch.long)
    for o in range(oh * ow):
        for k in range(9):
            ih, iw = 2 * (o // ow) - 1 + k // 3, 2 * (o % ow) - 1 + k % 3
            if 0 <= ih < h and 0 <= iw < w:
                want[o, k] = ih * w + iw
    assert torch.equal(windows, want)
    # every window has its centre, and every pixel is in some window
    assert bool((windows[:, 4] >= 0).all())
    assert windows[windows >= 0].unique().numel() == h * w


@pytest.mark.parametrize("h,w", IMAGES)
def test_covers_are_the_windows_inverted_in_ascending_order(h, w):
    windows, covers = _C.bn_pool_geometry(h, w)
    assert covers.shape == (h * w, 4, 2)
    for i in range(h * w):
        # (o, k) ascending in o is ascending in (oh, ow)
        want = [(o, k) for o, k in (windows == i).nonzero().tolist()]
        got = [tuple(e) for e in covers[i].tolist() if e[0] >= 0]
        assert got == want, i
        assert len(got) in (1, 2, 4)
        # the live entries are a prefix
        assert [tuple(e) for e in covers[i].tolist()[:len(got)]] == got


def _model_forward(y, windows):
    """y: [N, C, H, W] after ReLU -> (pooled [N, C, OH*OW], byte)"""
    n, c, h, w = y.shape
    flat = y.reshape(n, c, h * w)
    best = torch.full((n, c, windows.shape[0]), float("-inf"))
    pos = torch.full((n, c, windows.shape[0]), NONE, dtype=torch.long)
    for k in range(9):
        live = windows[:, k] >= 0
        v = flat[:, :, windows[:, k].clamp_min(0)]
        take = live & (v > best)  # strict: the first of equal values wins
        best = torch.where(take, v, best)
        pos = torch.where(take, torch.full_like(pos, k), pos)
    pos[best <= 0] = NONE
    return best, pos


def _model_backward(dy, pos, covers):
    """dy, pos: [N, C, OH*OW] -> g [N, C, H*W], summed in the covers' order"""
    g = torch.zeros(dy.shape[0], dy.shape[1], covers.shape[0])
    for slot in range(4):
        o, k = covers[:, slot, 0], covers[:, slot, 1]
        hit = (o >= 0) & (pos[:, :, o.clamp_min(0)] == k)
        g = g + torch.where(hit, dy[:, :, o.clamp_min(0)], torch.zeros(()))
    return g


@pytest.mark.parametrize("h,w", [(8, 8), (7, 9), (2, 2), (30, 30)])
def test_argmax_byte_model_is_max_pool_autograd(h, w):
    gen = torch.Generator().manual_seed(h * 100 + w)
    # four distinct values, two of them not positive: most windows tie
    values = torch.tensor([-1.0, 0.0, 0.5, 2.0])
    x = values[torch.randint(0, 4, (2, 3, h, w), generator=gen)]
    x.requires_grad_(True)
    out = F.max_pool2d(torch.relu(x), 3, 2, 1)
    dy = torch.randn(out.shape, generator=gen)
    out.backward(dy)
    windows, covers = _C.bn_pool_geometry(h, w)
    pooled, pos = _model_forward(torch.relu(x.detach()), windows)
    assert torch.equal(pooled.reshape(out.shape), out.detach())
    g = _model_backward(dy.reshape(2, 3, -1), pos, covers)
    assert torch.equal(g.reshape(x.shape), x.grad)
    if h * w >= 64:  # both kinds of pooled element occur
        assert bool((pos == NONE).any()) and bool((pos != NONE).any())


def test_cpu_bn_act_pool_is_the_stock_composition():
    torch.manual_seed(2)
    bn = nn.BatchNorm2d(8)
    pool = nn.MaxPool2d(3, 2, 1)
    import copy
    ref = copy.deepcopy(bn)
    x = torch.randn(2, 8, 9, 9)
    assert torch.equal(bn_act_pool(bn, x, pool), pool(torch.relu(ref(x))))
    assert torch.equal(bn.running_var, ref.running_var)
    assert int(bn.num_batches_tracked) == 1
