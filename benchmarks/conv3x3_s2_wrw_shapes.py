#!/usr/bin/env python3
"""Per-problem timing of the stride-2 3x3 convolution's weight gradient: the
native conv3x3s2_wrw (kernel plus finalize) against aten.convolution_backward
with output mask (False, True, False) (MIOpen's fill + igemm + cast), for the
three strided 3x3 problems of ResNet-50 at batch 256.

The two outputs are compared first (max-abs difference over the stock
result's max-abs).  Then device events, 5 warm-up calls and 20 timed
iterations of native / stock alternating in one process.  Prints one markdown
table row per problem: min / med / max of both in us, the TFLOP/s of the
2*R*N*9C real flops (R the rows of dY) and the share of the bytes floor (dY,
X and dW once each) at the native median, the plan's rows per chunk, images,
steps per chunk, splits and chunks per split, and the decision: native only
where the slowest native run beat the fastest stock run."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from torch_cgx_amd import _C  # noqa: E402

# (C = N, side of dY)
PROBLEMS = [(128, 28), (256, 14), (512, 7)]
HBM_BYTES_PER_US = 8e6  # 8 TB/s


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
        sys.exit("conv3x3_s2_wrw_shapes.py needs a GPU")
    print("| C→N @ X → dY | max diff / max | native, min / med / max us | "
          "stock, min / med / max us | native TFLOP/s | bytes floor / native "
          "| hr, images, steps; splits x chunks | decision |")
    print("|---|---|---|---|---|---|---|---|")
    for c, o in PROBLEMS:
        g = torch.Generator().manual_seed(c)
        dy = torch.randn(args.batch, c, o, o, generator=g).bfloat16().cuda() \
            .contiguous(memory_format=torch.channels_last)
        x = torch.randn(args.batch, c, 2 * o, 2 * o, generator=g).bfloat16() \
            .cuda().contiguous(memory_format=torch.channels_last)
        # the stock backward takes its shape only
        w = torch.zeros(c, c, 3, 3, dtype=torch.bfloat16, device="cuda") \
            .contiguous(memory_format=torch.channels_last)
        rows = args.batch * o * o
        plan = _C.conv3x3s2_wrw_plan(args.batch, 2 * o, 2 * o, c, c)

        def stock():
            return torch.ops.aten.convolution_backward(
                dy, x, w, None, (2, 2), (1, 1), (1, 1), False, (0, 0), 1,
                (False, True, False))[1]

        runs = {"native": lambda: _C.conv3x3s2_wrw(dy, x), "stock": stock}
        a, b = runs["native"]().float(), runs["stock"]().float()
        diff = ((a - b).abs().max() / b.abs().max()).item()
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

        med = statistics.median(t["native"])
        tflops = 2 * rows * c * 9 * c / med / 1e6
        floor = 2 * (rows * c + 4 * rows * c + 9 * c * c) / HBM_BYTES_PER_US
        print(f"| {c}→{c} @{2 * o} → {o} | {diff:.1e} | {mmm(t['native'])} | "
              f"{mmm(t['stock'])} | {tflops:.0f} | {floor / med:.2f} | "
              f"{plan['hr']}, {plan['images']}, {plan['strip_dy'] // 16}; "
              f"{plan['splits']} x {plan['chunks_per_split']} | "
              f"{'native' if wins else 'stock'} |", flush=True)
        del dy, w, x, a, b


if __name__ == "__main__":
    main()
