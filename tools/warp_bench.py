#!/usr/bin/env python
"""Time of the 2-D inverse warp (temporalstereo_amd.inverse_warp; csrc/inverse_warp.hip), forward and backward, bilinear, zeros padding,
disparity and depth mode, B = 1 and 4 at 544x960 with C = 3 and at 136x240 with C = 32 and C = 64:
  (a) the eager call (forward: ts.inverse_warp; backward: torch.autograd.grad through it, which includes zero-filling grad_img);
  (b) the same launch recorded once and replayed as a plan (no Python, no allocation; the backward replay accumulates into a
      grad_img that is not cleared between replays);
  (c) the framework composition a user runs today on the same device: pixel grid, (depth mode: the rigid projection in torch ops,)
      normalisation, the [B,H,W,2] grid tensor and F.grid_sample -- tests/warp_ref.py, which is exactly that;
  (d) the algorithmic bytes of (b) -- forward: image + motion + output; backward: grad_out + image + motion + grad_img + grad_motion --
      over its time, as a fraction of what a plain device copy of 256 MiB sustains in the same run (read + write bytes per second).
Usage: python tools/warp_bench.py [--out FILE]"""
import argparse
import os
import platform
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import warp_ref as R  # noqa: E402
import temporalstereo_amd as ts  # noqa: E402
from temporalstereo_amd import _lib  # noqa: E402
from timing import timed  # noqa: E402

SHAPES = [(544, 960, 3), (136, 240, 32), (136, 240, 64)]


def copy_rate(dev):
    """bytes per second (read + write) of a 256 MiB device copy"""
    n = 256 << 20
    a, b = torch.empty(n, device=dev, dtype=torch.uint8), torch.empty(n, device=dev, dtype=torch.uint8)
    a.zero_()
    L = _lib.lib()
    st = _lib.current_stream_handle()
    med = timed([lambda: L.ts_calib_stream(1, b.data_ptr(), a.data_ptr(), n, st)], 20, warmup=10)[0][0]
    return 2.0 * n / (med * 1e-6)


def scene(B, H, W, C, dev, seed):
    g = torch.Generator().manual_seed(seed)
    img = torch.randn(B, C, H, W, generator=g)
    disp = -torch.rand(B, 1, H, W, generator=g) * 0.2 * W
    K = torch.eye(3).repeat(B, 1, 1)
    K[:, 0, 0] = K[:, 1, 1] = 0.8 * W
    K[:, 0, 2], K[:, 1, 2] = (W - 1) / 2.0, (H - 1) / 2.0
    T = torch.eye(4).repeat(B, 1, 1)
    T[:, :3, :3] = torch.tensor([[0.995, -0.0998, 0.0], [0.0998, 0.995, 0.0], [0.0, 0.0, 1.0]])
    T[:, :3, 3] = torch.tensor([0.2, -0.05, 0.1])
    depth = 1.0 + 8.0 * torch.rand(B, 1, H, W, generator=g)
    return [t.to(dev) for t in (img, disp, depth, K, torch.inverse(K).contiguous(), T)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=200)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    rate = copy_rate(dev)
    lines = ["warp_bench: inverse_warp, bilinear, zeros padding; us per call, median of 5 x %d (min in brackets)" % args.iters,
             "GPU: %s; CPU: %s, torch %s; device copy of 256 MiB: %.0f GB/s (read + write)"
             % (torch.cuda.get_device_name(0), platform.processor() or platform.machine(), torch.__version__, rate / 1e9),
             "%-34s %16s %16s %16s %8s %8s" % ("shape, mode, direction", "(a) eager", "(b) plan replay", "(c) framework", "(c)/(b)", "(d)")]
    for B in (1, 4):
        for H, W, C in SHAPES:
            img, disp, depth, K, iK, T = scene(B, H, W, C, dev, 1000 + B + C)
            for mode in ("disparity", "depth"):
                motion = disp if mode == "disparity" else depth
                geo = (K, iK, T) if mode == "depth" else (None, None, None)
                name = "B=%d C=%-2d %dx%d %-9s" % (B, C, H, W, mode)
                # ---- forward
                a = timed([lambda: ts.inverse_warp(img, motion, mode, *geo)], args.iters, warmup=10)[0]
                with _lib.Recorder() as rec:
                    ts.inverse_warp(img, motion, mode, *geo)
                b = timed([rec.run], args.iters, warmup=10)[0]
                with torch.no_grad():
                    c = timed([lambda: R.inverse_warp(img, motion, mode, *geo)], args.iters, warmup=10)[0]
                nbytes = 4.0 * (img.numel() + motion.numel() + B * C * H * W)
                lines.append("%-34s %8.1f (%5.1f) %8.1f (%5.1f) %8.1f (%5.1f) %8.2f %7.0f%%"
                             % (name + " fwd", a[0], a[1], b[0], b[1], c[0], c[1], c[0] / b[0], 100 * nbytes / (b[0] * 1e-6) / rate))
                # ---- backward
                gout = torch.randn(B, C, H, W, device=dev)
                i1, m1 = img.clone().requires_grad_(True), motion.clone().requires_grad_(True)
                o1 = ts.inverse_warp(i1, m1, mode, *geo)
                a = timed([lambda: torch.autograd.grad(o1, (i1, m1), gout, retain_graph=True)], args.iters, warmup=10)[0]
                gi, gm = torch.zeros_like(img), torch.empty_like(motion)
                p = _lib.ptr
                kd = 3 if mode == "depth" else 0
                with _lib.Recorder() as rec:
                    rc = _lib.lib().ts_inverse_warp_bwd(p(img), p(motion), p(geo[0]), p(geo[1]), p(geo[2]), p(gout), p(gi), p(gm), B, C, H, W,
                                                        H, W, 0 if mode == "disparity" else 2, 0, 0, kd, kd, 1e-7,
                                                        _lib.current_stream_handle())
                    _lib.check(rc, "ts_inverse_warp_bwd")
                b = timed([rec.run], args.iters, warmup=10)[0]
                i2, m2 = img.clone().requires_grad_(True), motion.clone().requires_grad_(True)
                o2 = R.inverse_warp(i2, m2, mode, *geo)[0]
                c = timed([lambda: torch.autograd.grad(o2, (i2, m2), gout, retain_graph=True)], args.iters, warmup=10)[0]
                nbytes = 4.0 * (gout.numel() + 2 * img.numel() + 2 * motion.numel())
                lines.append("%-34s %8.1f (%5.1f) %8.1f (%5.1f) %8.1f (%5.1f) %8.2f %7.0f%%"
                             % (name + " bwd", a[0], a[1], b[0], b[1], c[0], c[1], c[0] / b[0], 100 * nbytes / (b[0] * 1e-6) / rate))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
