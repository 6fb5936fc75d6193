#!/usr/bin/env python3
"""Per-problem timing of the 1x1 convolution's weight gradient by the ring
kernel (conv1x1_wrw_ring and the finalize) against conv1x1_wrw and against
aten.convolution_backward for the weight alone, for the twelve stride-1 1x1
problems of ResNet-50 at batch 256.  The ring has no tile for 64 channels;
those problems show the other two only.

Device events, 5 warm-up calls and 20 timed iterations of ring / conv1x1_wrw /
stock alternating in one process.  Prints one markdown table row per problem:
min / med / max of the three in us, the bytes floor R*(N+K)*2 / 6.3 TB/s, the
input bytes and the FLOPs over the ring's median, tiles x splits x stages, and
whether the slowest ring run beat the fastest run of the path the problem
takes without it."""
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


def mmm(v):
    if not v:
        return "-"
    return f"{min(v):.0f} / {statistics.median(v):.0f} / {max(v):.0f}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    print("| K→N @ HxW | per step | ring, min / med / max us | conv1x1_wrw, "
          "min / med / max us | stock, min / med / max us | bytes floor us | "
          "ring TB/s | ring TFLOP/s | ring tiles x splits x stages "
          "(conv1x1_wrw tiles x splits) | decision |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    total = {"today": 0.0, "ring": 0.0, "best": 0.0}
    for k, n, hw, per_step in PROBLEMS:
        g = torch.Generator().manual_seed(k + n)
        dy = torch.randn(args.batch, n, hw, hw, generator=g).bfloat16().cuda() \
            .contiguous(memory_format=torch.channels_last)
        x = torch.randn(args.batch, k, hw, hw, generator=g).bfloat16().cuda() \
            .contiguous(memory_format=torch.channels_last)
        w = torch.empty(n, k, 1, 1, dtype=torch.bfloat16, device="cuda")
        rows = args.batch * hw * hw
        plan = _C.conv1x1_wrw_ring_plan(rows, k, n)
        old = _C.conv1x1_wrw_plan(rows, k, n)
        fns = {"wrw": lambda: _C.conv1x1_wrw(dy, x),
               "stock": lambda: stock(dy, x, w)}
        if plan["eligible"]:
            fns = {"ring": lambda: _C.conv1x1_wrw_ring(dy, x), **fns}
        for _ in range(args.warmup):
            for fn in fns.values():
                fn()
        torch.cuda.synchronize()
        t = {"ring": [], "wrw": [], "stock": []}
        for _ in range(args.iters):
            for name, fn in fns.items():
                t[name].append(timed(fn))
        med = {name: statistics.median(v) for name, v in t.items() if v}
        # the path the problem takes without the ring
        today = "wrw" if old["native"] else "stock"
        wins = bool(t["ring"]) and max(t["ring"]) < min(t[today])
        nbytes = rows * (n + k) * 2
        flops = 2 * rows * n * k
        total["today"] += per_step * med[today]
        total["ring"] += per_step * med.get("ring", med[today])
        total["best"] += per_step * (med["ring"] if wins else med[today])
        if plan["eligible"]:
            ring_cols = (f"{nbytes / med['ring'] / 1e6:.2f} | "
                         f"{flops / med['ring'] / 1e6:.0f} | "
                         f"{plan['ntiles_n'] * plan['ntiles_k']} of "
                         f"{plan['bn']} x {plan['bk']} x {plan['splits']} x "
                         f"{plan['stages']}")
        else:
            ring_cols = "- | - | -"
        print(f"| {k}→{n} @{hw} | {per_step} | {mmm(t['ring'])} | "
              f"{mmm(t['wrw'])} | {mmm(t['stock'])} | {nbytes / 6.3e6:.0f} | "
              f"{ring_cols} ({old['ntiles_n'] * old['ntiles_k']} of "
              f"{old['bn']} x {old['bk']} x {old['splits']}) | "
              f"{'ring' if wins else today} |", flush=True)
        del dy, x
    print(f"\nmedians weighted by convolutions per step: today's paths "
          f"{total['today'] / 1e3:.2f} ms, the ring wherever it has a tile "
          f"{total['ring'] / 1e3:.2f} ms, the ring where it wins and today's "
          f"path elsewhere {total['best'] / 1e3:.2f} ms")


if __name__ == "__main__":
    main()
