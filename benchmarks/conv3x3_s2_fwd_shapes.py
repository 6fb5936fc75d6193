#!/usr/bin/env python3
"""Per-problem timing of the 3x3 / stride 2 convolution's forward together
with the BatchNorm that follows it: the native conv3x3s2_stats and
bn_act_forward with its partials, against F.conv2d(stride=2) (MIOpen) and
bn_act_forward with a statistics pass of its own, for the three strided 3x3
problems of ResNet-50 (conv2 of the first block of layer2..4) at batch 256.

Device events, 5 warm-up calls and 20 timed iterations of native / stock
alternating in one process, after a comparison of both outputs on the timed
inputs.  Prints one markdown table row per problem: min / med / max of both
pairs in us and of the convolution kernel alone, the TFLOP/s of the 2*R*N*9C
real flops at the native convolution's median, the plan's tile, splits and
tiles per split, and the decision: native only where the slowest native run
beat the fastest stock run."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from torch_cgx_amd import _C  # noqa: E402

# (C = N, input image side)
PROBLEMS = [(128, 56), (256, 28), (512, 14)]


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
        sys.exit("conv3x3_s2_fwd_shapes.py needs a GPU")
    print("| C→N @ HxW in | native conv + bn, min / med / max us | stock conv "
          "+ bn, min / med / max us | native conv alone | stock conv alone | "
          "native conv TFLOP/s | tile rows x bn, splits x tiles | decision |")
    print("|---|---|---|---|---|---|---|---|")
    for c, hw in PROBLEMS:
        g = torch.Generator().manual_seed(c)
        x = torch.randn(args.batch, c, hw, hw, generator=g).bfloat16().cuda() \
            .contiguous(memory_format=torch.channels_last)
        w = (torch.randn(c, c, 3, 3, generator=g) / (3 * c ** 0.5)).bfloat16() \
            .cuda().contiguous(memory_format=torch.channels_last)
        gamma, beta = torch.ones(c).cuda(), torch.zeros(c).cuda()
        rm, rv = torch.zeros(c).cuda(), torch.ones(c).cuda()
        plan = _C.conv3x3s2_fwd_plan(args.batch, hw, hw, c, c)
        rows = plan["rows"]

        def bn(y, part):
            return _C.bn_act_forward(y, None, gamma, beta, rm, rv, 0.1, 1e-5,
                                     True, part)

        def native():
            return bn(*_C.conv3x3s2_stats(x, w))

        def stock():
            return bn(F.conv2d(x, w, stride=2, padding=1), None)

        # both paths round an fp32 sum to bf16 and normalise it: outputs of
        # unit scale that differ by a few bf16 roundings
        got, want = native()[0].float(), stock()[0].float()
        err = (got - want).abs().max().item()
        assert got.shape == want.shape and err <= 2.0 ** -5 * (
            1.0 + want.abs().max().item()), f"{c}@{hw}: outputs differ, {err}"

        runs = {"native": native, "stock": stock,
                "native conv": lambda: _C.conv3x3s2_stats(x, w),
                "stock conv": lambda: F.conv2d(x, w, stride=2, padding=1)}
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

        tflops = 2 * rows * c * 9 * c / statistics.median(t["native conv"]) / 1e6
        print(f"| {c}→{c} @{hw} | {mmm(t['native'])} | {mmm(t['stock'])} | "
              f"{mmm(t['native conv'])} | {mmm(t['stock conv'])} | "
              f"{tflops:.0f} | {plan['tile_rows']} x {plan['bn']}, "
              f"{plan['splits']} x {plan['tiles_per_split']} | "
              f"{'native' if wins else 'stock'} |", flush=True)
        del x, w


if __name__ == "__main__":
    main()
