#!/usr/bin/env python
"""Time of ConvGRU (temporalstereo_amd.ConvGRU; csrc/conv_gru.hip) at Ch = Cx = 64 on 68x120 and 136x240 (B = 1 and 4) and at
Ch = Cx = 32 on 272x480 (B = 1), three legs:
  forward            one step under no_grad;
  forward + backward one step and the gradients of last_hidden, x and the six parameters;
  chain of 8         eight steps under no_grad, the output the next step's last_hidden.
Three arms in the same process, alternating within every repetition, on the same module and parameters:
  (a) the module's own path: functional.conv_gru (weight layout + two launches);
  (b) the module's _reference_forward on the HIP convolution kernels (the composition on layers.Conv2d);
  (c) the module's _reference_forward under set_conv_backend('torch'): the framework's convolutions.
Outputs of (a) are compared with (c) before anything is timed.  us per call: median of 5 x N (min .. max of the 5).

Launches per call come from a kernel trace collected in a run of its own:
  rocprofv3 --kernel-trace --output-format csv -d DIR -- python tools/conv_gru_bench.py --trace-run
runs every (arm, leg) once at [1,64,68,120] with a calib_fill launch between them, and
  python tools/conv_gru_bench.py --out FILE --trace-dir DIR
counts the kernels between those marks and adds the table to the report.
Usage: python tools/conv_gru_bench.py [--out FILE] [--iters N] [--trace-dir DIR] | --trace-run"""
import argparse
import csv
import glob
import os
import platform
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import temporalstereo_amd as ts  # noqa: E402
from temporalstereo_amd import _lib, layers  # noqa: E402
from timing import timed  # noqa: E402

#          B  C   H    W
SHAPES = [(1, 64, 68, 120), (4, 64, 68, 120), (1, 64, 136, 240), (4, 64, 136, 240), (1, 32, 272, 480)]
ARMS = ("(a) fused cell", "(b) HIP convolutions", "(c) framework")
LEGS = ("forward", "forward + backward", "chain of 8")
MARK = "calib_fill"


def make(B, C, H, W, dev):
    g = torch.Generator().manual_seed(B + C + H)
    m = ts.ConvGRU(C, C)
    with torch.no_grad():
        for p in m.parameters():
            p.copy_(torch.randn(p.shape, generator=g) * ((2.0 / (9 * 2 * C) ** 0.5) if p.dim() == 4 else 0.5))
    m = m.to(dev)
    h = torch.tanh(torch.randn(B, C, H, W, generator=g)).to(dev)
    x = torch.randn(B, C, H, W, generator=g).to(dev)
    cot = torch.randn(B, C, H, W, generator=g).to(dev)
    return m, h, x, cot


def arms_of(m):
    def torch_backend(h, x):
        layers.set_conv_backend("torch")
        try:
            return m._reference_forward(h, x)
        finally:
            layers.set_conv_backend("hip")
    return (m, m._reference_forward, torch_backend)


def legs_of(step, m, h, x, cot):
    hg, xg = h.clone().requires_grad_(True), x.clone().requires_grad_(True)
    params = [hg, xg] + list(m.parameters())

    def forward():
        with torch.no_grad():
            return step(h, x)

    def both():
        return torch.autograd.grad(step(hg, xg), params, cot)

    def chain():
        with torch.no_grad():
            o = h
            for _ in range(8):
                o = step(o, x)
            return o
    return (forward, both, chain)


def trace_run(dev):
    """every (arm, leg) once, a calib_fill launch before each and after the last"""
    m, h, x, cot = make(*SHAPES[0], dev)
    buf = torch.zeros(1 << 20, device=dev, dtype=torch.uint8)
    mark = lambda: _lib.check(_lib.lib().ts_calib_stream(0, buf.data_ptr(), buf.data_ptr(), buf.numel(), _lib.current_stream_handle()), "mark")
    runs = [fn for step in arms_of(m) for fn in legs_of(step, m, h, x, cot)]
    for fn in runs:                      # first calls: allocator growth, MIOpen's find step
        fn()
        fn()
    torch.cuda.synchronize()
    for fn in runs:
        mark()
        fn()
    mark()
    torch.cuda.synchronize()


def launches(trace_dir):
    """kernels between consecutive marks of a --trace-run trace, in (arm, leg) order"""
    rows = []
    for path in glob.glob(os.path.join(trace_dir, "**", "*kernel_trace.csv"), recursive=True):
        with open(path) as fh:
            rows += [(int(r["Start_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(fh)]
    rows.sort()
    marks = [i for i, (_, name) in enumerate(rows) if MARK in name]
    need = len(ARMS) * len(LEGS) + 1
    if len(marks) < need:
        raise SystemExit("trace under %s holds %d marks, %d expected" % (trace_dir, len(marks), need))
    marks = marks[-need:]
    return [marks[i + 1] - marks[i] - 1 for i in range(need - 1)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--trace-run", action="store_true")
    ap.add_argument("--trace-dir", default=None)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    if args.trace_run:
        trace_run(dev)
        return
    lines = ["conv_gru_bench: ConvGRU, one step = z, r, q and the blend; us per call, median of 5 x N (min .. max of the 5); N is stated per shape",
             "GPU: %s; CPU: %s, torch %s" % (torch.cuda.get_device_name(0), platform.processor() or platform.machine(), torch.__version__),
             "(a) functional.conv_gru; (b) _reference_forward on the HIP convolution kernels; (c) _reference_forward, set_conv_backend('torch')",
             "%-40s %28s %28s %28s %8s %8s" % ("shape [B,Ch=Cx,H,W], leg", "(a) fused cell", "(b) HIP convolutions", "(c) framework", "(b)/(a)", "(c)/(a)")]
    losers = []
    for B, C, H, W in SHAPES:
        iters = args.iters if B * H * W < 100000 else max(4, args.iters // 4)
        m, h, x, cot = make(B, C, H, W, dev)
        name = "[%d,%d,%d,%d]" % (B, C, H, W)
        arms = arms_of(m)
        with torch.no_grad():
            oa, ob, oc = (step(h, x) for step in arms)
        rel = [float((o - oc).norm() / oc.norm()) for o in (oa, ob)]
        lines.append("%-40s N = %d; relative L2 against (c): (a) %.2e, (b) %.2e" % (name, iters, rel[0], rel[1]))
        assert max(rel) < 1e-4, name
        del oa, ob, oc
        per_arm = [legs_of(step, m, h, x, cot) for step in arms]
        for li, leg in enumerate(LEGS):
            ta, tb, tc = timed([legs[li] for legs in per_arm], iters)
            for other, t in (("(b)", tb), ("(c)", tc)):
                if ta[0] > t[0]:
                    losers.append("%s %s: (a) %.1f us against %s %.1f us (%.2f x slower)" % (name, leg, ta[0], other, t[0], ta[0] / t[0]))
            lines.append("%-40s %10.1f (%7.1f ..%7.1f) %10.1f (%7.1f ..%7.1f) %10.1f (%7.1f ..%7.1f) %8.2f %8.2f"
                         % (name + " " + leg, ta[0], ta[1], ta[2], tb[0], tb[1], tb[2], tc[0], tc[1], tc[2], tb[0] / ta[0], tc[0] / ta[0]))
        del m, h, x, cot, per_arm, arms
        torch.cuda.empty_cache()
    lines.append("legs where the fused cell's median is the slower one: " + ("; ".join(losers) if losers else "none"))
    if args.trace_dir:
        counts = launches(args.trace_dir)
        lines.append("kernel launches per call at [%d,%d,%d,%d], from a kernel trace of `--trace-run` collected in a run of its own:" % SHAPES[0])
        for ai, arm in enumerate(ARMS):
            lines.append("  %-24s %s" % (arm, ", ".join("%s %d" % (leg, counts[ai * len(LEGS) + li]) for li, leg in enumerate(LEGS))))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
