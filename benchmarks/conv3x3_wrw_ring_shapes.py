#!/usr/bin/env python3
"""Per-problem timing of the 3x3 weight gradient through a ring of LDS stages
(conv3x3_wrw_ring and the finalize) against conv3x3_wrw and against
aten.convolution_backward for the weight alone, for the four stride-1 3x3
problems of ResNet-50's bottlenecks at batch 256.

Device events, 5 warm-up calls and 20 timed iterations of the ring with two
stages, the ring with three, conv3x3_wrw and stock alternating in one process.
Prints one markdown table row per problem and ring geometry: min / med / max
in us, the bytes floor R*(C+N)*2 / 6.3 TB/s and the factor by which the ring
reads X more than once (hr + 2 rows per hr, one per group of whole images),
the TFLOP/s of the 2*R*N*9C real flops at the ring's median, tiles x splits x
stages with hr, and the decision: the ring only where its slowest run beat the
fastest run of the path the problem takes today (conv3x3_wrw where its plan
says native, stock elsewhere)."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
from torch_cgx_amd import _C  # noqa: E402

# (C = N, image side, convolutions per step)
PROBLEMS = [(64, 56, 3), (128, 28, 3), (256, 14, 5), (512, 7, 2)]
STAGES = (2, 3)


def stock(dy, x, w):
    return torch.ops.aten.convolution_backward(
        dy, x, w, None, (1, 1), (1, 1), (1, 1), False, (0, 0), 1,
        (False, True, False))[1]


def timed(fn):
    a, b = (torch.cuda.Event(enable_timing=True) for _ in range(2))
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3


def mmm(v):
    return f"{min(v):.0f} / {statistics.median(v):.0f} / {max(v):.0f}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    print("| C→N @ HxW | per step | stages | ring, min / med / max us | "
          "conv3x3_wrw | stock | today | bytes floor us, X re-read | ring "
          "TFLOP/s | tiles x splits x stages, hr | decision |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    total = {st: {"ring": 0.0, "today": 0.0, "best": 0.0} for st in STAGES}
    for c, hw, per_step in PROBLEMS:
        g = torch.Generator().manual_seed(c)
        dy = torch.randn(args.batch, c, hw, hw, generator=g).bfloat16().cuda() \
            .contiguous(memory_format=torch.channels_last)
        x = torch.randn(args.batch, c, hw, hw, generator=g).bfloat16().cuda() \
            .contiguous(memory_format=torch.channels_last)
        w = torch.empty(c, c, 3, 3, dtype=torch.bfloat16, device="cuda") \
            .contiguous(memory_format=torch.channels_last)
        rows = args.batch * hw * hw
        today = ("conv3x3_wrw"
                 if _C.conv3x3_wrw_plan(args.batch, hw, hw, c, c)["native"]
                 else "stock")
        fns = {f"ring{st}": (lambda st=st: _C.conv3x3_wrw_ring(dy, x, 0, st))
               for st in STAGES}
        fns["conv3x3_wrw"] = lambda: _C.conv3x3_wrw(dy, x)
        fns["stock"] = lambda: stock(dy, x, w)
        for _ in range(args.warmup):
            for fn in fns.values():
                fn()
        torch.cuda.synchronize()
        t = {name: [] for name in fns}
        for _ in range(args.iters):
            for name, fn in fns.items():
                t[name].append(timed(fn))
        for st in STAGES:
            ring = t[f"ring{st}"]
            plan = _C.conv3x3_wrw_ring_plan(args.batch, hw, hw, c, c, 0, st)
            wins = max(ring) < min(t[today])
            med = statistics.median(ring)
            total[st]["ring"] += per_step * med
            total[st]["today"] += per_step * statistics.median(t[today])
            total[st]["best"] += per_step * (
                med if wins else statistics.median(t[today]))
            reread = (1.0 if plan["images"] > 1
                      else (plan["hr"] + 2) / plan["hr"])
            chunk = (f"{plan['hr']}" if plan["images"] == 1
                     else f"{plan['hr']} ({plan['images']} images)")
            tiles = plan["ntiles_n"] * plan["ntiles_k"]
            print(f"| {c}→{c} @{hw} | {per_step} | {st} | {mmm(ring)} | "
                  f"{mmm(t['conv3x3_wrw'])} | {mmm(t['stock'])} | {today} | "
                  f"{rows * 2 * c * 2 / 6.3e6:.0f}, {reread:.2f} | "
                  f"{2 * rows * c * 9 * c / med / 1e6:.0f} | "
                  f"{tiles} x {plan['splits']} x {st}, {chunk} | "
                  f"{'ring' if wins else today} |", flush=True)
        del dy, x
    for st in STAGES:
        v = total[st]
        print(f"\n{st} stages, medians weighted by convolutions per step: ring "
              f"{v['ring'] / 1e3:.2f} ms, today's paths "
              f"{v['today'] / 1e3:.2f} ms, winners by the ring and the rest "
              f"as today {v['best'] / 1e3:.2f} ms")


if __name__ == "__main__":
    main()
