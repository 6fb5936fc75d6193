#!/usr/bin/env python3
"""Per-problem timing of the 1x1 / stride 2 downsample convolution's forward
together with the join that follows it: the native conv1x1s2_stats and
bn_act2_forward with its `partd`, against F.conv2d(stride=2) (MIOpen) and
bn_act2_forward with a statistics pass of its own for the downsample
BatchNorm, for the three downsample problems of ResNet-50 at batch 256.  The
main path's `x3`, its partials and both BatchNorms' parameters are held fixed.

Device events, 5 warm-up calls and 20 timed iterations of native / stock
alternating in one process, after a comparison of both outputs on the timed
inputs.  Prints one markdown table row per problem: min / med / max of both
pairs in us and of the convolution alone, the TFLOP/s of the 2*R*N*K flops and
the bytes floor (X's read pixels, W and Y once each, at 8 TB/s) over the
native convolution's median, the plan's splits and tiles per split, and the
decision: native only where the slowest native pair beat the fastest stock
pair."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from torch_cgx_amd import _C  # noqa: E402

# (K, N, input image side)
PROBLEMS = [(256, 512, 56), (512, 1024, 28), (1024, 2048, 14)]
HBM_BYTES_PER_US = 8.0e6


def timed(fn):
    a, b = (torch.cuda.Event(enable_timing=True) for _ in range(2))
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("conv1x1_s2_fwd_shapes.py needs a GPU")
    print("| K→N @ HxW in | native conv + join, min / med / max us | stock "
          "conv + join, min / med / max us | native conv alone | stock conv "
          "alone | native conv TFLOP/s | bytes floor / native conv | splits x "
          "tiles | decision |")
    print("|---|---|---|---|---|---|---|---|---|")
    for k, n, hw in PROBLEMS:
        g = torch.Generator().manual_seed(k)

        def cl(t):
            return t.bfloat16().cuda().contiguous(
                memory_format=torch.channels_last)

        x = cl(torch.randn(args.batch, k, hw, hw, generator=g))
        w = cl(torch.randn(n, k, 1, 1, generator=g) / k ** 0.5)
        # the main path's conv3 output and its partials, as the model has them
        x3, part3 = _C.conv1x1_stats(
            cl(torch.randn(args.batch, 64, hw // 2, hw // 2, generator=g)),
            cl(torch.randn(n, 64, 1, 1, generator=g) / 8))
        bn = [torch.ones(n).cuda(), torch.zeros(n).cuda(),
              torch.zeros(n).cuda(), torch.ones(n).cuda(), 0.1, 1e-5]
        plan = _C.conv1x1s2_plan(args.batch, hw, hw, k, n)
        rows = plan["rows"]

        def join(yd, partd):
            return _C.bn_act2_forward(x3, yd, *bn, *bn, True, part3, partd)

        def native():
            return join(*_C.conv1x1s2_stats(x, w))

        def stock():
            return join(F.conv2d(x, w, stride=2), None)

        # both paths round an fp32 sum to bf16 and normalise it: outputs of
        # unit scale that differ by a few bf16 roundings
        got, want = native()[0].float(), stock()[0].float()
        err = (got - want).abs().max().item()
        assert got.shape == want.shape and err <= 2.0 ** -5 * (
            1.0 + want.abs().max().item()), f"{k}@{hw}: outputs differ, {err}"

        runs = {"native": native, "stock": stock,
                "native conv": lambda: _C.conv1x1s2_stats(x, w),
                "stock conv": lambda: F.conv2d(x, w, stride=2)}
        for _ in range(args.warmup):
            for fn in runs.values():
                fn()
        torch.cuda.synchronize()
        t = {name: [] for name in runs}
        for _ in range(args.iters):
            for name, fn in runs.items():
                t[name].append(timed(fn))
        wins = max(t["native"]) < min(t["stock"])

        def mmm(v):
            return f"{min(v):.0f} / {statistics.median(v):.0f} / {max(v):.0f}"

        med = statistics.median(t["native conv"])
        floor = 2 * (rows * k + n * k + rows * n) / HBM_BYTES_PER_US
        print(f"| {k}→{n} @{hw} | {mmm(t['native'])} | {mmm(t['stock'])} | "
              f"{mmm(t['native conv'])} | {mmm(t['stock conv'])} | "
              f"{2 * rows * n * k / med / 1e6:.0f} | {floor / med:.2f} | "
              f"{plan['splits']} x {plan['tiles_per_split']} | "
              f"{'native' if wins else 'stock'} |", flush=True)
        del x, w, x3


if __name__ == "__main__":
    main()
