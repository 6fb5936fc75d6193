#!/usr/bin/env python3
"""Per-problem timing of the tiled walk of the native 1x1 convolution
(conv1x1_tiled_stats, conv1x1_tiled_bwd_data) against the kernel that keeps
its weight tile in LDS (conv1x1_stats, conv1x1_bwd_data) and against the stock
path, for the twelve stride-1 1x1 problems of ResNet-50 at batch 256: the
forward, and backward-data with and without a skip gradient.

The forward is timed with the bn_act_forward that follows it, as the model
runs it: the two native kernels hand it their partials, the stock convolution
leaves it the statistics pass.  Backward-data with a skip gradient includes
the bf16 add on the stock side.  The tiled GEMM is also timed alone, for its
TB/s over R*(K+N)*2 bytes and its TFLOP/s, and torch.mm on the same
[R, K] x [K, N] for comparison only.

Device events, 5 warm-up calls and 20 timed iterations of the candidates
alternating in one process.  Prints one markdown table row per problem with
min / med / max in us, and whether the slowest tiled run beat the fastest run
of the path the problem takes today (the resident kernel where its plan says
native, else stock); then the rows for kNativeTiled / kNativeTiledBwd."""
import argparse
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402
from torch_cgx_amd import _C  # noqa: E402

# (K, N, image side, convolutions per step)
PROBLEMS = [(64, 64, 56, 1), (64, 256, 56, 4), (256, 64, 56, 2),
            (256, 128, 56, 1), (128, 512, 28, 4), (512, 128, 28, 3),
            (512, 256, 28, 1), (256, 1024, 14, 6), (1024, 256, 14, 5),
            (1024, 512, 14, 1), (512, 2048, 7, 3), (2048, 512, 7, 2)]


def timed(fn):
    a, b = (torch.cuda.Event(enable_timing=True) for _ in range(2))
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) * 1e3


def measure(cands, warmup, iters):
    for _ in range(warmup):
        for fn in cands.values():
            fn()
    torch.cuda.synchronize()
    t = {name: [] for name in cands}
    for _ in range(iters):
        for name, fn in cands.items():
            t[name].append(timed(fn))
    return t


def mmm(v):
    return f"{min(v):.0f} / {statistics.median(v):.0f} / {max(v):.0f}"


def stock_dx(dy, x, w):
    return torch.ops.aten.convolution_backward(
        dy, x, w, None, (1, 1), (0, 0), (1, 1), False, (0, 0), 1,
        (True, False, False))[0]


def rand_cl(g, *shape):
    return torch.randn(*shape, generator=g, device="cuda").bfloat16() \
        .contiguous(memory_format=torch.channels_last)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=256)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    head = ("| {} | tiled, min / med / max us | resident | stock | today | "
            "tiled GEMM alone | bytes floor us | TB/s | TFLOP/s | torch.mm | "
            "tiles x splits | decision |")
    sep = "|" + "---|" * 12
    wins = {"fwd": [], "bwd": []}
    total = {}

    def row(kind, label, k, n, rows, t, plan, today, per_step):
        alone = statistics.median(t["alone"])
        nbytes, flop = rows * (k + n) * 2, 2.0 * rows * k * n
        win = max(t["tiled"]) < min(t[today])
        for name in ("tiled", "resident", "stock"):
            key = (kind, name)
            total[key] = total.get(key, 0.0) + per_step * statistics.median(
                t[name])
        key = (kind, "today")
        total[key] = total.get(key, 0.0) + per_step * statistics.median(
            t[today])
        key = (kind, "best")
        total[key] = total.get(key, 0.0) + per_step * statistics.median(
            t["tiled" if win else today])
        print(f"| {label} | {mmm(t['tiled'])} | {mmm(t['resident'])} | "
              f"{mmm(t['stock'])} | {today} | {mmm(t['alone'])} | "
              f"{nbytes / 6.3e6:.0f} | {nbytes / alone / 1e6:.2f} | "
              f"{flop / alone / 1e6:.0f} | {mmm(t['mm'])} | "
              f"{plan['ntiles']} x {plan['splits']} | "
              f"{'tiled' if win else today} |", flush=True)
        return win

    print(head.format("forward K→N @ side (per step)"))
    print(sep)
    for k, n, hw, per_step in PROBLEMS:
        g = torch.Generator(device="cuda").manual_seed(k + n)
        x = rand_cl(g, args.batch, k, hw, hw)
        w = (torch.randn(n, k, 1, 1, generator=g, device="cuda")
             / k ** 0.5).bfloat16()
        rows = args.batch * hw * hw
        bn = [torch.ones(n, device="cuda"), torch.zeros(n, device="cuda"),
              torch.zeros(n, device="cuda"), torch.ones(n, device="cuda")]
        a2, b2 = x.permute(0, 2, 3, 1).reshape(rows, k), w.view(n, k).t()

        def with_bn(conv):
            def f():
                y, part = conv()
                _C.bn_act_forward(y, None, *bn, 0.1, 1e-5, True, part)
            return f

        cands = {
            "tiled": with_bn(lambda: _C.conv1x1_tiled_stats(x, w)),
            "resident": with_bn(lambda: _C.conv1x1_stats(x, w)),
            "stock": with_bn(lambda: (F.conv2d(x, w), None)),
            "alone": lambda: _C.conv1x1_tiled_stats(x, w),
            "mm": lambda: torch.mm(a2, b2),
        }
        t = measure(cands, args.warmup, args.iters)
        today = "resident" if _C.conv1x1_plan(rows, k, n)["native"] else "stock"
        if row("fwd", f"{k}→{n} @{hw} ({per_step})", k, n, rows, t,
               _C.conv1x1_tiled_plan(rows, k, n), today, per_step):
            wins["fwd"].append(f"{{{k}, {n}, {rows}}}")
        del x, a2

    print()
    print(head.format("backward-data K←N @ side (per step counts both)"))
    print(sep)
    for k, n, hw, per_step in PROBLEMS:
        g = torch.Generator(device="cuda").manual_seed(k + n + 1)
        dy = rand_cl(g, args.batch, n, hw, hw)
        skip = rand_cl(g, args.batch, k, hw, hw)
        w = (torch.randn(n, k, 1, 1, generator=g, device="cuda")
             / n ** 0.5).bfloat16()
        rows = args.batch * hw * hw
        a2, b2 = dy.permute(0, 2, 3, 1).reshape(rows, n), w.view(n, k)
        for add in (False, True):
            s = skip if add else None
            cands = {
                "tiled": lambda: _C.conv1x1_tiled_bwd_data(dy, w, s),
                "resident": lambda: _C.conv1x1_bwd_data(dy, w, s),
                "stock": (lambda: stock_dx(dy, skip, w) + skip) if add
                else (lambda: stock_dx(dy, skip, w)),
                "alone": lambda: _C.conv1x1_tiled_bwd_data(dy, w, s),
                "mm": lambda: torch.mm(a2, b2),
            }
            t = measure(cands, args.warmup, args.iters)
            today = ("resident" if _C.conv1x1_bwd_plan(rows, k, n, add)["native"]
                     else "stock")
            label = f"{k}←{n} @{hw}{' +skip' if add else ''} ({per_step})"
            if row("bwd+" if add else "bwd", label, n, k, rows, t,
                   _C.conv1x1_tiled_bwd_plan(rows, k, n, add), today, per_step):
                wins["bwd"].append(
                    f"{{{k}, {n}, {rows}, {'true' if add else 'false'}}}")
        del dy, skip, a2

    print("\nmedians weighted by convolutions per step, ms:")
    for kind in ("fwd", "bwd", "bwd+"):
        print(f"  {kind}: " + ", ".join(
            f"{name} {total[(kind, name)] / 1e3:.2f}"
            for name in ("tiled", "resident", "stock", "today", "best")))
    print("\nkNativeTiled:    " + ", ".join(wins["fwd"]))
    print("kNativeTiledBwd: " + ", ".join(wins["bwd"]))


if __name__ == "__main__":
    main()
