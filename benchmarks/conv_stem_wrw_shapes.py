#!/usr/bin/env python3
"""Per-problem timing of the stem convolution's weight gradient: the native
conv_stem_wrw with its finalize against aten.convolution_backward with mask
(False, True, False) (MIOpen), for the stem of ResNet-50 at batch 256,
224 x 224.

Device events, 5 warm-up calls and 20 timed iterations of native / stock
alternating in one process.  Prints one markdown table row per grid cap: min /
med / max of both in us, the TFLOP/s of the 2*R*64*147 real flops and the TB/s
of the bytes of dy and x at the native median, the plan's band, splits and
bands per split, and the decision: native only where the slowest native run
beat the fastest stock run.  --max-workgroups adds rows with the grid
capped."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from torch_cgx_amd import _C  # noqa: E402


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
    ap.add_argument("--size", type=int, default=224)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--max-workgroups", type=int, nargs="*", default=[])
    args = ap.parse_args()
    b, hw = args.batch, args.size
    g = torch.Generator().manual_seed(3)
    x = torch.randn(b, 3, hw, hw, generator=g).bfloat16().cuda() \
        .contiguous(memory_format=torch.channels_last)
    dy = torch.randn(b, 64, hw // 2, hw // 2, generator=g).bfloat16().cuda() \
        .contiguous(memory_format=torch.channels_last)
    w = torch.empty(64, 3, 7, 7, dtype=torch.bfloat16, device="cuda") \
        .contiguous(memory_format=torch.channels_last)
    rows = b * (hw // 2) ** 2

    def stock():
        return torch.ops.aten.convolution_backward(
            dy, x, w, None, (2, 2), (3, 3), (1, 1), False, (0, 0), 1,
            (False, True, False))[1]

    print("| B x H x W, grid cap | native, min / med / max us | stock, min / "
          "med / max us | native TFLOP/s | TB/s | band rows, splits x bands | "
          "decision |")
    print("|---|---|---|---|---|---|---|")
    for cap in [0] + args.max_workgroups:
        plan = _C.conv_stem_wrw_plan(b, hw, hw, cap)
        runs = {"native": lambda: _C.conv_stem_wrw(dy, x, cap), "stock": stock}
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
        tflops = 2 * rows * 64 * 147 / med / 1e6
        tbs = 2 * (x.numel() + dy.numel()) / med / 1e6
        print(f"| {b} x {hw} x {hw}, {cap or 'none'} | {mmm(t['native'])} | "
              f"{mmm(t['stock'])} | {tflops:.0f} | {tbs:.2f} | "
              f"{plan['band_rows']}, {plan['splits']} x "
              f"{plan['bands_per_split']} | "
              f"{'native' if wins else 'stock'} |", flush=True)


if __name__ == "__main__":
    main()
