"""Fused BatchNorm: launch geometry (csrc/bn_plan.cc) and the Python routing
(torch_cgx_amd/ops/fused_bn.py), checked without a GPU."""

import copy

import pytest
import torch
import torch.nn as nn

from torch_cgx_amd import _C
from torch_cgx_amd.models import resnet50
from torch_cgx_amd.models.resnet import Bottleneck
from torch_cgx_amd.ops.fused_bn import bn_act

SHAPES = [(2, 64), (98, 64), (75, 256), (196, 2048), (6272, 64),
          (12544, 2048), (256 * 112 * 112, 64)]


@pytest.mark.parametrize("rows,channels", SHAPES)
def test_sweep_covers_every_vector_once(rows, channels):
    plan = _C.bn_plan(rows, channels)
    assert plan["eligible"]
    nvec = rows * channels // 8
    idx = _C.bn_sweep_indices(rows, channels)
    threads = plan["threads"]
    assert idx.shape == (plan["grid"] * threads, plan["rows_per_thread"] + 1)
    # no thread runs longer than the plan says
    assert bool((idx[:, -1] == -1).all())
    seen = idx[idx >= 0]
    # no index out of range, every vector exactly once
    assert int(seen.max()) < nvec
    assert seen.numel() == nvec
    assert bool((torch.bincount(seen, minlength=nvec) == 1).all())
    # a thread's run is a prefix of its row, and its channel group is constant
    live = idx >= 0
    assert bool((live[:, :-1] >= live[:, 1:]).all())
    cg = idx % plan["cgs"]
    cg0 = cg[:, :1].expand_as(cg)
    assert bool((cg[live] == cg0[live]).all())
    # the longest run is the run length the plan reports
    assert int(live.sum(1).max()) == plan["rows_per_thread"]


@pytest.mark.parametrize("rows,channels", SHAPES)
def test_partials_fit_and_do_not_collide(rows, channels):
    plan = _C.bn_plan(rows, channels)
    assert plan["grid"] == plan["ctiles"] * plan["splits"]
    assert plan["partial_floats"] == plan["splits"] * channels
    # two fp32 partial rows per split stay a few per cent of the tensor
    if rows >= 80:
        assert 2 * 4 * plan["partial_floats"] <= 0.05 * 2 * rows * channels
    seen = torch.zeros(plan["partial_floats"], dtype=torch.int32)
    wgs = range(plan["grid"]) if plan["grid"] <= 64 else (
        list(range(8)) + list(range(plan["grid"] - 8, plan["grid"])))
    for wg in wgs:
        offs = torch.tensor(_C.bn_partial_offsets(rows, channels, wg))
        assert int(offs.min()) >= 0
        assert int(offs.max()) < plan["partial_floats"]
        seen[offs] += 1
    assert int(seen.max()) == 1
    if plan["grid"] <= 64:
        assert int(seen.min()) == 1


def test_benchmark_shapes_fill_the_chip():
    # ResNet-50 at batch 256: every BatchNorm gets at least one workgroup per
    # CU of a 256-CU part
    for hw, channels in [(112, 64), (56, 64), (56, 256), (28, 128), (28, 512),
                         (14, 256), (14, 1024), (7, 512), (7, 2048)]:
        assert _C.bn_plan(256 * hw * hw, channels)["grid"] >= 256


def test_row_count_limit():
    # rows are counted in fp32 inside the kernels: exact up to 2^24
    assert _C.bn_plan(1 << 24, 64)["eligible"]
    assert not _C.bn_plan((1 << 24) + 1, 64)["eligible"]


@pytest.mark.parametrize("rows,channels", [(98, 12), (98, 4096), (1, 64),
                                           (98, 4), (98, 0)])
def test_ineligible(rows, channels):
    assert not _C.bn_plan(rows, channels)["eligible"]
    with pytest.raises(RuntimeError):
        _C.bn_sweep_indices(rows, channels)


def test_cpu_tensors_are_not_eligible():
    x = torch.randn(2, 64, 7, 7).bfloat16().to(
        memory_format=torch.channels_last)
    assert not _C.bn_eligible(x)


def test_resnet50_names_do_not_depend_on_the_switch(monkeypatch):
    names = []
    for flag in ("0", "1"):
        monkeypatch.setenv("CGX_FUSED_BN", flag)
        m = resnet50(num_classes=10)
        names.append(([n for n, _ in m.named_parameters()],
                      [n for n, _ in m.named_buffers()],
                      list(m.state_dict().keys())))
    assert names[0] == names[1]
    assert "layer1.0.bn3.weight" in names[0][0]
    assert "layer1.0.downsample.1.running_var" in names[0][1]


def _reference_bottleneck_forward(blk, x):
    """The composition Bottleneck.forward ran before bn_act existed."""
    identity = x
    out = blk.relu(blk.bn1(blk.conv1(x)))
    out = blk.relu(blk.bn2(blk.conv2(out)))
    out = blk.bn3(blk.conv3(out))
    if blk.downsample is not None:
        identity = blk.downsample(x)
    return blk.relu(out + identity)


@pytest.mark.parametrize("with_downsample", [False, True])
@pytest.mark.parametrize("flag", ["0", "1"])
def test_cpu_bottleneck_is_bitwise_the_old_composition(monkeypatch, flag,
                                                       with_downsample):
    monkeypatch.setenv("CGX_FUSED_BN", flag)
    torch.manual_seed(7)
    if with_downsample:
        down = nn.Sequential(nn.Conv2d(16, 32, 1, stride=2, bias=False),
                             nn.BatchNorm2d(32))
        new = Bottleneck(16, 8, stride=2, downsample=down)
    else:
        new = Bottleneck(32, 8)
    for bn in (new.bn1, new.bn2, new.bn3):
        nn.init.normal_(bn.weight, 1.0, 0.2)
        nn.init.normal_(bn.bias, 0.0, 0.2)
    old = copy.deepcopy(new)
    x_new = torch.randn(3, new.conv1.in_channels, 9, 9, requires_grad=True)
    x_old = x_new.detach().clone().requires_grad_(True)
    for _ in range(2):  # the second step starts from updated running stats
        y_new = new(x_new)
        y_old = _reference_bottleneck_forward(old, x_old)
        assert torch.equal(y_new, y_old)
        y_new.square().sum().backward()
        y_old.square().sum().backward()
    assert torch.equal(x_new.grad, x_old.grad)
    for (n, a), (_, b) in zip(new.named_parameters(), old.named_parameters()):
        assert torch.equal(a.grad, b.grad), n
    for (n, a), (_, b) in zip(new.named_buffers(), old.named_buffers()):
        assert torch.equal(a, b), n


def test_cpu_bn_act_eval_and_plain_bn():
    torch.manual_seed(3)
    bn = nn.BatchNorm2d(8)
    x = torch.randn(4, 8, 5, 5)
    idn = torch.randn(4, 8, 5, 5)
    ref = copy.deepcopy(bn)
    assert torch.equal(bn_act(bn, x, idn), torch.relu(ref(x) + idn))
    assert torch.equal(bn_act(bn, x, relu=False), ref(x))
    bn.eval(), ref.eval()
    assert torch.equal(bn_act(bn, x), torch.relu(ref(x)))
    assert torch.equal(bn.running_mean, ref.running_mean)
    assert int(bn.num_batches_tracked) == int(ref.num_batches_tracked) == 2
