#!/usr/bin/env python
"""Time of the encoder's large planes (temporalstereo_amd.StemConv / ConvBnAct / FusedInvertedResidual; csrc/fused_mbconv.hip) at the
shapes the reference's encoder (efficientnetv2_rw_s on a 544 x 960 image) runs them at, batch 2 and 8 (the batch is both eyes):
  the stem 3 -> 24, stride 2, on 544 x 960;   a ConvBnAct 24 -> 24 with its skip on 272 x 480;
  the four distinct fused blocks: 24 -> 96 -> 48 stride 2 (272 x 480 -> 136 x 240), 48 -> 192 -> 48 on 136 x 240,
  48 -> 192 -> 64 stride 2 (136 x 240 -> 68 x 120), 64 -> 256 -> 64 on 68 x 120;
  the whole front of the backbone: stem, block0 (2 members), block1 (4), block2 (4).
Eval forward, two arms alternating within every repetition, in one process:
  (a) the kernel form inside WeightLayouts / BNFolds contexts (layouts and folds made once, as TemporalStereoBackbone.forward keeps them);
  (b) the same module on its reference route, set_conv_backend('torch'): the framework's convolution, BatchNorm, SiLU and add.
The output of (a) is compared with (b) before anything is timed.  us per call: median of 21 timed windows of N calls between device
events (min .. max of the 21), after three untimed rounds of every arm.  Every row is reported, losses included.  For a fused block also
the bytes of the mid map it writes and reads back: what a one-launch form with the mid tile kept in LDS would save.
Usage: python tools/encoder_bench.py [--out FILE] [--reps R] [--batches B ...]"""
import argparse
import os
import platform
import sys

import torch
import torch.nn as nn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import temporalstereo_amd as ts  # noqa: E402
from temporalstereo_amd import functional as TF  # noqa: E402
from timing import cell, timed, torch_backend  # noqa: E402


def rows():
    """(label, module factory, input channels, input plane, mid map (channels, plane) or None)"""
    def front():
        net = ts.TemporalStereoBackbone()
        stem = ts.StemConv.from_modules(net.conv_stem, net.bn1, net.act1)
        return nn.Sequential(stem, net.block0, net.block1, net.block2)
    return [("stem 3 -> 24, stride 2", lambda: ts.StemConv(3, 24), 3, (544, 960), None),
            ("ConvBnAct 24 -> 24, skip", lambda: ts.ConvBnAct(24, 24, skip=True), 24, (272, 480), None),
            ("fused 24 -> 96 -> 48, stride 2", lambda: ts.FusedInvertedResidual(24, 48, stride=2), 24, (272, 480), (96, (136, 240))),
            ("fused 48 -> 192 -> 48, residual", lambda: ts.FusedInvertedResidual(48, 48), 48, (136, 240), (192, (136, 240))),
            ("fused 48 -> 192 -> 64, stride 2", lambda: ts.FusedInvertedResidual(48, 64, stride=2), 48, (136, 240), (192, (68, 120))),
            ("fused 64 -> 256 -> 64, residual", lambda: ts.FusedInvertedResidual(64, 64), 64, (68, 120), (256, (68, 120))),
            ("front: stem, block0, block1, block2", front, 3, (544, 960), None)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--batches", type=int, nargs="+", default=[2, 8])
    args = ap.parse_args()
    assert args.reps >= 20
    dev = torch.device("cuda:0")
    iters = 4
    lines = ["encoder_bench: the encoder's large planes, eval forward; us per call, median of %d windows of %d calls (min .. max of them)"
             % (args.reps, iters),
             "GPU: %s; CPU: %s, torch %s" % (torch.cuda.get_device_name(0), platform.processor() or platform.machine(), torch.__version__),
             "(a) the kernel form inside WeightLayouts / BNFolds contexts; (b) the same module's reference route, set_conv_backend('torch')"]
    print("\n".join(lines), flush=True)
    losses = []

    def emit(line):
        lines.append(line)
        print(line, flush=True)
    emit("%-64s %32s %32s %8s  %s" % ("row [B, input plane]", "(a) kernel form", "(b) framework", "(b)/(a)", "mid map written + read"))
    for B in args.batches:
        for label, make, cin, (H, W), mid in rows():
            g = torch.Generator().manual_seed(B * 1000 + cin + H)
            m = make()
            with torch.no_grad():
                for p in m.parameters():
                    if p.dim() == 4:
                        p.copy_(torch.randn(p.shape, generator=g) * (1.0 / (p.shape[1] * p.shape[2] * p.shape[3]) ** 0.5))
                for mod in m.modules():
                    if isinstance(mod, nn.BatchNorm2d):
                        mod.running_mean.copy_(torch.randn(mod.num_features, generator=g) * 0.1)
                        mod.running_var.copy_(torch.rand(mod.num_features, generator=g) + 0.5)
            m = m.to(dev).eval()
            x = torch.randn((B, cin, H, W), generator=g).to(dev)
            reference = torch_backend(m)                         # the module itself: that backend routes it to _reference_forward
            with torch.no_grad():
                first = m[0] if isinstance(m, nn.Sequential) else m
                assert first._route(x) == "kernels"
                own, ref = m(x), reference(x)
            rel = float((own - ref).norm() / ref.norm())
            assert rel < 1e-4, rel
            del own, ref

            def no_grad(fn):
                def run():
                    with torch.no_grad():
                        return fn(x)
                return run
            with TF.WeightLayouts(), TF.BNFolds():
                no_grad(m)()                                     # lays the weights out, folds the BatchNorms
                ta, tb = timed([no_grad(m), no_grad(reference)], iters, args.reps)
            name = "%s [%d, %dx%d]" % (label, B, H, W)
            if ta[0] > tb[0]:
                losses.append("%s: (a) %.1f us against (b) %.1f us (min %.1f .. max %.1f)" % (name, ta[0], tb[0], tb[1], tb[2]))
            note = ""
            if mid is not None:
                nbytes = 2 * 4 * B * mid[0] * mid[1][0] * mid[1][1]
                note = "%.1f MB" % (nbytes / 1e6)
            emit("%-64s %s %s %8.2f  %s" % (name + ", rel L2 vs (b) %.1e" % rel, cell(ta), cell(tb), tb[0] / ta[0], note))
            del m, x
            torch.cuda.empty_cache()
    emit("rows where the kernel form's median is the slower one: " + ("; ".join(losses) if losses else "none"))
    text = "\n".join(lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
