#!/usr/bin/env python3
"""Per-problem timing of the 1x1 convolution's weight gradient: the native
conv1x1_wrw (GEMM and finalize) against aten.convolution_backward for the
weight alone (MIOpen's workspace fill, igemm and cast), for the twelve
stride-1 1x1 problems of ResNet-50 at batch 256.

Device events, 5 warm-up calls and 20 timed iterations of native / stock
alternating in one process.  Prints one markdown table row per problem:
min / med / max of both in us, the bytes floor R*(N+K)*2 / 6.3 TB/s, the
input bytes over the native median, the plan's tile and splits, and whether
the slowest native run beat the fastest stock run."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from torch_cgx_amd import _C  # noqa: E402

# (K, N, image side, convolutions per step)
PROBLEMS = [(64, 64, 56, 1), (64, 256, 56, 4), (256, 64, 56, 2),
            (256, 128, 56, 1), (128, 512, 28, 4), (512, 128, 28, 3),
            (512, 256, 28, 1), (256, 1024, 14, 6), (1024, 256, 14, 5),
            (1024, 512, 14, 1), (512, 2048, 7, 3), (2048, 512, 7, 2)]


def stock(dy, x, w):
    return torch.ops.aten.convolution_backward(
        dy, x, w, None, (1, 1), (0, 0), (1, 1), False, (0, 0), 1,
        (False, True, False))[1]


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
    print("| K→N @ HxW | per step | native, min / med / max us | stock, min / "
          "med / max us | bytes floor us | native TB/s | tile bn x bk, splits "
          "| decision |")
    print("|---|---|---|---|---|---|---|---|")
    total = {"native": 0.0, "stock": 0.0, "best": 0.0}
    for k, n, hw, per_step in PROBLEMS:
        g = torch.Generator().manual_seed(k + n)
        dy = torch.randn(args.batch, n, hw, hw, generator=g).bfloat16().cuda() \
            .contiguous(memory_format=torch.channels_last)
        x = torch.randn(args.batch, k, hw, hw, generator=g).bfloat16().cuda() \
            .contiguous(memory_format=torch.channels_last)
        w = torch.empty(n, k, 1, 1, dtype=torch.bfloat16, device="cuda")
        rows = args.batch * hw * hw
        plan = _C.conv1x1_wrw_plan(rows, k, n)
        for _ in range(args.warmup):
            _C.conv1x1_wrw(dy, x)
            stock(dy, x, w)
        torch.cuda.synchronize()
        t = {"native": [], "stock": []}
        for _ in range(args.iters):
            t["native"].append(timed(lambda: _C.conv1x1_wrw(dy, x)))
            t["stock"].append(timed(lambda: stock(dy, x, w)))
        med = {name: statistics.median(v) for name, v in t.items()}
        wins = max(t["native"]) < min(t["stock"])
        nbytes = rows * (n + k) * 2
        for name in med:
            total[name] += per_step * med[name]
        total["best"] += per_step * (med["native"] if wins else med["stock"])

        def mmm(v):
            return f"{min(v):.0f} / {statistics.median(v):.0f} / {max(v):.0f}"

        print(f"| {k}→{n} @{hw} | {per_step} | {mmm(t['native'])} | "
              f"{mmm(t['stock'])} | {nbytes / 6.3e6:.0f} | "
              f"{nbytes / med['native'] / 1e6:.2f} | {plan['bn']} x "
              f"{plan['bk']}, {plan['splits']} | "
              f"{'native' if wins else 'stock'} |", flush=True)
        del dy, x
    print(f"\nmedians weighted by convolutions per step: native "
          f"{total['native'] / 1e3:.2f} ms, stock {total['stock'] / 1e3:.2f} ms, "
          f"winners native and the rest stock {total['best'] / 1e3:.2f} ms")


if __name__ == "__main__":
    main()
