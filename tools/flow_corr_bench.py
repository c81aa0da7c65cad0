#!/usr/bin/env python
"""Time of FlowCorrBlock (temporalstereo_amd.FlowCorrBlock; csrc/flow_corr.hip), num_levels = 4, radius = 4, at the reference stub's own
shapes (aggregation/utils/raft_corr.py:170-194: C = 80 at 1/16 and 1/8 of 384 x 1248, i.e. [1,80,24,78] and [1,80,48,156]) and at
[4,80,24,78]:
  (a) the HIP path: build (ts_flow_corr_pyramid_fwd), lookup (ts_flow_corr_lookup_fwd), build + lookup, and build + lookup + backward
      (ts_flow_corr_lookup_bwd with the folded cotangent, ts_flow_corr_pyramid_bwd), through the public interface, allocations included;
  (b) the same four on the framework composition a user runs today on the same device -- tests/flow_corr_ref.py: three matmuls and
      their combine, 2x2 averages, gathers -- (a) and (b) alternating within every repetition;
  (c) the same run's ceilings: a device fill and a device copy of 256 MiB (ts_calib_stream, as benchlegs/k1.py).  The build is
      reported as a share of the fill ceiling, from the pyramid's bytes written plus 2 B C H W 4 read.
Before timing, outputs and gradients of (a) and (b) are compared at every shape.  us per call: median of 5 x N (min .. max).
Usage: python tools/flow_corr_bench.py [--out FILE] [--iters N]"""
import argparse
import os
import platform
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import flow_corr_ref as R  # noqa: E402
import temporalstereo_amd as ts  # noqa: E402
from timing import ceilings, timed  # noqa: E402

SHAPES = [(1, 80, 24, 78), (1, 80, 48, 156), (4, 80, 24, 78)]
L, RAD = 4, 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=20)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    fill, copy = ceilings(dev)
    lines = ["flow_corr_bench: FlowCorrBlock, num_levels = %d, radius = %d; us per call, median of 5 x %d (min .. max of the 5)" % (L, RAD, args.iters),
             "GPU: %s; CPU: %s, torch %s; device fill of 256 MiB: %.0f GB/s, copy: %.0f GB/s (read + write)"
             % (torch.cuda.get_device_name(0), platform.processor() or platform.machine(), torch.__version__, fill / 1e9, copy / 1e9),
             "for orientation only: the reference quotes 1199.6 us and 2107.2 us for build + lookup 'at scale=8' on its own GPU and clock (raft_corr.py:224-225)",
             "%-32s %30s %30s %9s" % ("shape, leg", "(a) HIP", "(b) framework composition", "(b)/(a)")]
    losers = []
    for B, C, H, W in SHAPES:
        g = torch.Generator().manual_seed(100 * B + C)
        f1, f2 = torch.randn(B, C, H, W, generator=g).to(dev), torch.randn(B, C, H, W, generator=g).to(dev)
        flow = (torch.rand(B, 2, H, W, generator=g) - 0.5) * 0.5 * torch.tensor([W, H], dtype=torch.float32).view(1, 2, 1, 1)
        coords = ts.FlowCorrBlock.init_flow((B, C, H, W), dev, flow_init=flow.to(dev))[1].contiguous()      # the target coordinates
        cot = torch.randn(B, L * (2 * RAD + 1) ** 2, H, W, generator=g).to(dev)
        name = "[%d,%d,%d,%d]" % (B, C, H, W)

        # ---- (a) against (b): outputs and gradients
        def grads(fn):
            a, b_, d = (t.clone().requires_grad_(True) for t in (f1, f2, coords))
            o = fn(a, b_, d)
            return (o.detach(),) + torch.autograd.grad(o, (a, b_, d), cot)
        ga = grads(lambda a, b_, d: ts.FlowCorrBlock(a, b_, L, RAD)(d))
        gb = grads(lambda a, b_, d: R.flow_corr_block(a, b_, d, L, RAD))
        # a coordinate on a kink may round to the other cell in one of the two: report the share of outputs that differ visibly
        diff = (ga[0] - gb[0]).abs()
        rel = [float((x - y).norm() / y.norm()) for x, y in zip(ga[1:], gb[1:])]
        lines.append("%-32s max |out (a) - (b)| %.2e (max |out| %.1f, %.4f %% of the outputs differ by more than 1e-4); relative L2 of the gradients: "
                     "fmap1 %.2e fmap2 %.2e coords %.2e" % (name + " check", float(diff.max()), float(gb[0].abs().max()),
                                                          100.0 * float((diff > 1e-4).float().mean()), rel[0], rel[1], rel[2]))
        # a broken build must not leave a bench file: loose bounds, far above rounding (positions on a kink may flip a cell)
        assert max(rel) < 1e-3, "%s: gradients of (a) and (b) differ: %s" % (name, rel)
        assert float((diff > 1e-4).float().mean()) < 1e-3, "%s: outputs of (a) and (b) differ" % name
        del ga, gb, diff

        # ---- the four legs
        with torch.no_grad():
            blk = ts.FlowCorrBlock(f1, f2, L, RAD)
            lev = R.corr_pyramid(f1, f2, L)
        a1, b1, d1 = (t.clone().requires_grad_(True) for t in (f1, f2, coords))

        def nograd(fn):
            def run():
                with torch.no_grad():
                    return fn()
            return run

        def train_a():
            torch.autograd.grad(ts.FlowCorrBlock(a1, b1, L, RAD)(d1), (a1, b1, d1), cot)

        def train_b():
            torch.autograd.grad(R.flow_corr_block(a1, b1, d1, L, RAD), (a1, b1, d1), cot)
        legs = [("build", nograd(lambda: ts.FlowCorrBlock(f1, f2, L, RAD)), nograd(lambda: R.corr_pyramid(f1, f2, L))),
                ("lookup", nograd(lambda: blk(coords)), nograd(lambda: R.lookup(lev, coords, RAD))),
                ("build + lookup", nograd(lambda: ts.FlowCorrBlock(f1, f2, L, RAD)(coords)), nograd(lambda: R.flow_corr_block(f1, f2, coords, L, RAD))),
                ("build + lookup + backward", train_a, train_b)]
        for leg, fa, fb in legs:
            ta, tb = timed([fa, fb], args.iters)
            extra = ""
            if leg == "build":
                nbytes = 4.0 * (B * H * W * sum((H >> i) * (W >> i) for i in range(L)) + 2 * B * C * H * W)
                extra = "   %.0f %% of the fill ceiling" % (100.0 * nbytes / (ta[0] * 1e-6) / fill)
            if ta[0] > tb[0]:
                losers.append("%s %s: HIP %.1f us against %.1f us (%.2f x slower)" % (name, leg, ta[0], tb[0], ta[0] / tb[0]))
            lines.append("%-32s %10.1f (%8.1f .. %8.1f) %10.1f (%8.1f .. %8.1f) %9.2f%s"
                         % (name + " " + leg, ta[0], ta[1], ta[2], tb[0], tb[1], tb[2], tb[0] / ta[0], extra))
        del blk, lev
        torch.cuda.empty_cache()
    lines.append("shapes where a HIP median is slower than the composition's: " + ("; ".join(losers) if losers else "none"))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
