#!/usr/bin/env python
"""Time of SPP3D (temporalstereo_amd.SPP3D; csrc/spp3d.hip), strides (2, 4, 8, 16), at [1,64,48,136,240], [1,32,24,68,120] and
[4,32,24,68,120]:
  pool        ts_spp3d_pool_fwd (one launch) against the four F.avg_pool3d calls it replaces, and as a share of the same run's copy
              ceiling from its algorithmic bytes (x read once, the levels written);
  expand      ts_spp3d_expand_fwd (one launch) against four F.interpolate and a torch.cat, share of the copy ceiling from x read and the
              concatenation written;
  conv 3x3x3  the "hw3" composition (three (1,3,3) launches and ts_depth_sum3_fwd) against the framework's convolution, forward and
              forward + backward, C + 64 -> C channels;
  module      the whole module, forward (eval, no_grad) and forward + backward (train), against the reference's op sequence on
              layers.Conv3d (SPP3D._reference_forward: what a user runs today), the same parameters.
(a) and (b) alternate within every repetition; outputs are compared before anything is timed.  us per call: median of 5 x N (min .. max).
The ceilings are a device fill and a device copy of 256 MiB (ts_calib_stream, as benchlegs/k1.py).
Usage: python tools/spp3d_bench.py [--out FILE] [--iters N]"""
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
from timing import ceilings, timed  # noqa: E402

SHAPES = [(1, 64, 48, 136, 240), (1, 32, 24, 68, 120), (4, 32, 24, 68, 120)]
STRIDES = (2, 4, 8, 16)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=5)         # (the largest shape runs max(3, N / 5) calls per repetition)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    fill, copy = ceilings(dev)
    lines = ["spp3d_bench: SPP3D, strides %s; us per call, median of 5 x N (min .. max of the 5); N is stated per shape" % (STRIDES,),
             "GPU: %s; CPU: %s, torch %s; device fill of 256 MiB: %.0f GB/s, copy: %.0f GB/s (read + write)"
             % (torch.cuda.get_device_name(0), platform.processor() or platform.machine(), torch.__version__, fill / 1e9, copy / 1e9),
             "%-44s %30s %30s %9s" % ("shape, leg", "(a) HIP", "(b) framework", "(b)/(a)")]
    losers = []
    for B, C, D, H, W in SHAPES:
        iters = args.iters if B * C * D * H * W < (1 << 26) else max(3, args.iters // 5)
        g = torch.Generator().manual_seed(B + C)
        x = torch.randn(B, C, D, H, W, generator=g).to(dev)
        name = "[%d,%d,%d,%d,%d]" % (B, C, D, H, W)
        vol = D * H * W
        sizes = ts.spp3d_level_sizes((D, H, W), STRIDES)
        boxes = [tuple(min(n, s) for n in (D, H, W)) for s in STRIDES]
        lv16 = [torch.randn((B, 16) + n, generator=g).to(dev) for n in sizes]
        lines.append("%-44s N = %d" % (name, iters))
        ccat = C + 16 * len(STRIDES)
        w3 = (torch.randn(C, ccat, 3, 3, 3, generator=g) * (2.0 / (27 * ccat)) ** 0.5).to(dev)

        def pool_b():
            return [F.avg_pool3d(x, kernel_size=k, stride=k) for k in boxes]

        def expand_b():
            return torch.cat([x] + [F.interpolate(l, size=(D, H, W), mode="trilinear", align_corners=True) for l in lv16], dim=1)
        with torch.no_grad():
            for a, b_ in zip(ts.spp3d_pool(x, STRIDES), pool_b()):
                assert float((a - b_).abs().max()) < 1e-5, name
            cat = ts.spp3d_expand(lv16, x, STRIDES)
            assert float((cat - expand_b()).abs().max()) < 1e-4, name
            ya, yb = ts.conv3d_k333(cat, w3), F.conv3d(cat, w3, None, 1, 1)
            rel = float((ya - yb).norm() / yb.norm())
            lines.append("%-44s relative L2 of conv3d_k333 against the framework's convolution %.2e" % (name + " check", rel))
            assert rel < 1e-3, name
            del ya, yb
        m = ts.SPP3D(in_planes=C, strides=STRIDES).to(dev)
        cot = torch.randn(B, C, D, H, W, generator=g).to(dev)
        xg = x.clone().requires_grad_(True)
        m.train()
        oa, ob = m(xg), m._reference_forward(xg)
        rel = float((oa - ob).norm() / ob.norm())
        lines.append("%-44s relative L2 of the module against the reference's op sequence (train) %.2e" % (name + " check", rel))
        assert rel < 1e-3, name
        del oa, ob
        catg, w3g = cat.clone().requires_grad_(True), w3.clone().requires_grad_(True)
        params = [xg] + list(m.parameters())

        def nograd(fn):
            def run():
                with torch.no_grad():
                    return fn()
            return run

        def module_eval(fn):
            def run():
                m.eval()
                with torch.no_grad():
                    return fn(x)
            return run

        def module_train(fn):
            def run():
                m.train()
                torch.autograd.grad(fn(xg), params, cot)
            return run
        pool_bytes = 4.0 * (B * C * vol + B * C * sum(n[0] * n[1] * n[2] for n in sizes))
        expand_bytes = 4.0 * (B * C * vol + B * ccat * vol)
        legs = [("pool", nograd(lambda: ts.spp3d_pool(x, STRIDES)), nograd(pool_b), pool_bytes),
                ("expand", nograd(lambda: ts.spp3d_expand(lv16, x, STRIDES)), nograd(expand_b), expand_bytes),
                ("conv 3x3x3 forward", nograd(lambda: ts.conv3d_k333(cat, w3)), nograd(lambda: F.conv3d(cat, w3, None, 1, 1)), None),
                ("conv 3x3x3 forward + backward", lambda: torch.autograd.grad(ts.conv3d_k333(catg, w3g), (catg, w3g), cot),
                 lambda: torch.autograd.grad(F.conv3d(catg, w3g, None, 1, 1), (catg, w3g), cot), None),
                ("module forward (eval)", module_eval(m), module_eval(m._reference_forward), None),
                ("module forward + backward (train)", module_train(m), module_train(m._reference_forward), None)]
        for leg, fa, fb, nbytes in legs:
            ta, tb = timed([fa, fb], iters)
            extra = "   %.0f %% of the copy ceiling" % (100.0 * nbytes / (ta[0] * 1e-6) / copy) if nbytes else ""
            if ta[0] > tb[0]:
                losers.append("%s %s: HIP %.1f us against %.1f us (%.2f x slower)" % (name, leg, ta[0], tb[0], ta[0] / tb[0]))
            lines.append("%-44s %10.1f (%8.1f .. %8.1f) %10.1f (%8.1f .. %8.1f) %9.2f%s"
                         % (name + " " + leg, ta[0], ta[1], ta[2], tb[0], tb[1], tb[2], tb[0] / ta[0], extra))
        del m, cat, catg, lv16, x, xg
        torch.cuda.empty_cache()
    lines.append("legs where a HIP median is slower than the framework's: " + ("; ".join(losers) if losers else "none"))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
