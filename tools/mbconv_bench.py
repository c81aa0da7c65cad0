#!/usr/bin/env python
"""Time of one MemoryInvertedResidual block (temporalstereo_amd.MemoryInvertedResidual; csrc/mbconv.hip) at the three shapes the
reference's encoder (efficientnetv2_rw_s on a 544 x 960 image) runs it at, a memory of a quarter of the channels given, batch 2 and 8:
  C = 128, Cmid = 512, Cr = 32 on 34 x 60;   C = 160, Cmid = 960, Cr = 40 on 34 x 60;   C = 272, Cmid = 1632, Cr = 68 on 17 x 30
Legs and arms, the arms alternating within every repetition, in one process:
  eval forward              (a) the four-launch form inside WeightLayouts / BNFolds contexts (layouts and folds made once, as a pass keeps
                            them); (a') the same as a bare call: two weight layouts and three folds launched with it; (c) the same module on
                            the reference's op sequence, set_conv_backend('torch')
  train forward + backward  (a) the module's training form (splice and depthwise convolution on the kernels, the rest framework ops);
                            (c) the reference's op sequence, set_conv_backend('torch')
  depthwise alone           (a) functional.depthwise_conv3x3 against (c) F.conv2d(groups = C) on the block's expanded map, forward and
                            forward + backward
The eval output of (a) is compared with (c) before anything is timed.  us per call: median of 21 timed windows of N calls (min .. max of the
21), after three untimed rounds of every arm.
Usage: python tools/mbconv_bench.py [--out FILE] [--reps R]"""
import argparse
import os
import platform
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import temporalstereo_amd as ts  # noqa: E402
from temporalstereo_amd import functional as TF  # noqa: E402
from timing import cell, timed, torch_backend  # noqa: E402

#          C    Cmid  Cr   plane
SHAPES = [(128, 512, 32, (34, 60)), (160, 960, 40, (34, 60)), (272, 1632, 68, (17, 30))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--batches", type=int, nargs="+", default=[2, 8])
    args = ap.parse_args()
    assert args.reps >= 20
    dev = torch.device("cuda:0")
    iters = 4
    lines = ["mbconv_bench: one MemoryInvertedResidual block, memory_percent 1/4, memory given; us per call, median of %d windows of %d calls "
             "(min .. max of them)" % (args.reps, iters),
             "GPU: %s; CPU: %s, torch %s" % (torch.cuda.get_device_name(0), platform.processor() or platform.machine(), torch.__version__),
             "(a) the kernel path; (a') eval forward as a bare call (+ 2 weight layouts, 3 BatchNorm folds); (c) the reference's op sequence, "
             "set_conv_backend('torch')"]
    head = "%-52s %32s %32s %32s %8s" % ("block [B, C -> Cmid (Cr), H x W], leg", "(a) kernel path", "(a') bare call", "(c) framework", "(c)/(a)")
    print("\n".join(lines), flush=True)
    losses = []

    def emit(line):
        lines.append(line)
        print(line, flush=True)

    def row(label, ta, tb, tc, shape=""):
        if ta[0] > tc[0]:
            losses.append("%s %s: (a) %.1f us against (c) %.1f us (min %.1f .. max %.1f)" % (shape, label.strip(), ta[0], tc[0], tc[1], tc[2]))
        emit("%-52s %s %s %s %8.2f" % (label, cell(ta), cell(tb), cell(tc), tc[0] / ta[0]))
    emit(head)
    for B in args.batches:
        for C, Cmid, Cr, (H, W) in SHAPES:
            g = torch.Generator().manual_seed(B * 1000 + C)
            m = ts.MemoryInvertedResidual(C, mid_chs=Cmid, se_chs=Cr)
            with torch.no_grad():
                for p in m.parameters():
                    if p.dim() == 4:
                        p.copy_(torch.randn(p.shape, generator=g) * (2.0 / (p.shape[1] * p.shape[2] * p.shape[3]) ** 0.5))
            m = m.to(dev).eval()
            x = torch.randn((B, C, H, W), generator=g).to(dev)
            memory = torch.randn((B, C // 4, H, W), generator=g).to(dev)
            cot = torch.randn((B, C, H, W), generator=g).to(dev)
            reference = torch_backend(m)                         # the module itself: that backend routes it to _reference_forward
            label = "[%d, %d -> %d (%d), %dx%d]" % (B, C, Cmid, Cr, H, W)
            with torch.no_grad():
                assert m._route(x, memory) == "kernels"
                own, ref = m(x, memory)[0], reference(x, memory)[0]
            rel = float((own - ref).norm() / ref.norm())
            assert rel < 1e-4, rel

            def no_grad(fn):
                def run():
                    with torch.no_grad():
                        return fn(x, memory)
                return run
            with TF.WeightLayouts(), TF.BNFolds():
                no_grad(m)()                                     # lays the weights out, folds the BatchNorms
                ta, tc = timed([no_grad(m), no_grad(reference)], iters, args.reps)
            (tb,) = timed([no_grad(m)], iters, args.reps)
            row("%s eval forward, rel L2 vs (c) %.1e" % (label, rel), ta, tb, tc)

            m.train()
            xg, mg = x.clone().requires_grad_(True), memory.clone().requires_grad_(True)
            wrt = [xg, mg] + list(m.parameters())
            assert m._route(xg, mg) == "train"
            ta, tc = timed([lambda: torch.autograd.grad(m(xg, mg)[0], wrt, cot), lambda: torch.autograd.grad(reference(xg, mg)[0], wrt, cot)],
                           iters, args.reps)
            row("%52s" % "train forward + backward", ta, None, tc, label)

            e = torch.randn((B, Cmid, H, W), generator=g).to(dev)
            w = m.conv_dw.weight.detach()
            ta, tc = timed([lambda: TF.depthwise_conv3x3(e, w), lambda: F.conv2d(e, w, None, 1, 1, 1, Cmid)], iters, args.reps)
            row("%52s" % "depthwise 3x3 alone, forward", ta, None, tc, label)
            eg, wg = e.clone().requires_grad_(True), w.clone().requires_grad_(True)
            ta, tc = timed([lambda: torch.autograd.grad(TF.depthwise_conv3x3(eg, wg), [eg, wg], e),
                            lambda: torch.autograd.grad(F.conv2d(eg, wg, None, 1, 1, 1, Cmid), [eg, wg], e)], iters, args.reps)
            row("%52s" % "depthwise 3x3 alone, forward + backward", ta, None, tc, label)
            del m, x, memory, cot, e, eg, wg, xg, mg
            torch.cuda.empty_cache()
    emit("rows where the kernel path's median is the slower one against the framework: " + ("; ".join(losses) if losses else "none"))
    text = "\n".join(lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
