#!/usr/bin/env python
"""Time of rendering a frame at 544x960 from an estimate at 136x240 (every output of render_frame: the estimate coloured above the
ground truth, both error maps, the legend, the 16-bit map), B = 1 and B = 4, uint8 and fp32:
  (a) temporalstereo_amd.render_frame on the GPU: eager calls, and the same launches recorded once and replayed as a plan
      (hipEvents around a loop of calls after warm-up); beside it the algorithmic bytes (inputs read once + outputs written once)
      and the fraction of the fill ceiling measured in the same run on a stream of the outputs' size (benchlegs/k1.stream_ceilings);
  (b) for scale, the host method: `.cpu()` of the estimate and the ground truth and a numpy restatement of visualize's pictures
      (video_inference.py:169-227: F.interpolate, disp_to_color of the stacked maps, the error classes, the re-valued error
      through a jet table, the legend, the uint16 cast), per image as the reference works.
The file this writes records what was measured; it is not a pass criterion.
Usage: python tools/render_bench.py [--out FILE]"""
import argparse
import os
import platform
import sys
import time

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import synth  # noqa: E402
from benchlegs.k1 import stream_ceilings  # noqa: E402
from temporalstereo_amd import _lib, render_frame  # noqa: E402
from temporalstereo_amd.visualization import jet_table  # noqa: E402
from timing import timed  # noqa: E402

H, W, LH, LW = 544, 960, 136, 240
JET = jet_table().astype(np.float64)
CLASS_LO = np.array([0, 0.1875, 0.375, 0.75, 1.5, 3, 6, 12, 24, 48]) / 3.0
CLASS_RGB = np.array([[49, 54, 149], [69, 117, 180], [116, 173, 209], [171, 217, 233], [224, 243, 248], [254, 224, 144],
                      [253, 174, 97], [244, 109, 67], [215, 48, 39], [165, 0, 38]]) / 255.0
EDGES = np.array([0.0, 0.114, 0.299, 0.413, 0.587, 0.701, 0.886])
WIDTH = np.array([114.0, 185.0, 114.0, 174.0, 114.0, 185.0, 114.0]) / 1000.0
ROWS = np.array([[0, 0, 0], [0, 0, 1], [1, 0, 0], [1, 0, 1], [0, 1, 0], [0, 1, 1], [1, 1, 0], [1, 1, 1]], dtype=np.float64)


def scene(B, seed):
    g = lambda tag, shape, lo, hi: torch.from_numpy(synth.uniform(seed, tag, shape, lo, hi))
    gt = g("gt", (B, 1, H, W), 1.0, 150.0) * (g("keep", (B, 1, H, W), 0.0, 1.0) > 0.3)
    low = F.interpolate(gt, size=(LH, LW), mode='bilinear', align_corners=True) * (LW / W) + g("n", (B, 1, LH, LW), -1.0, 1.0)
    return low.contiguous(), gt.contiguous()


def host_frame(est, gt):
    """One image on the host, numpy: what visualize computes before it hands the pictures to matplotlib."""
    e = F.interpolate(est[None] * W / est.shape[-1], size=(H, W), mode='bilinear', align_corners=True)[0, 0].numpy()
    g = gt[0].numpy()
    cat = np.concatenate((e, g), axis=0)
    t = (cat / cat.max()).astype(np.float64)
    s = (t[..., None] > EDGES[1:]).sum(-1)
    r = ((t - EDGES[s]) / WIDTH[s])[..., None]
    disp_color = (ROWS[s] * (1 - r) + ROWS[s + 1] * r).clip(0, 1)
    a, b = e * 255.0, g * 255.0
    E = np.abs(a - b)
    ok = b > 0
    rel = np.zeros_like(b)
    rel[ok] = E[ok] / b[ok] / 0.05
    E = np.minimum(E / 3.0, rel)
    cls = np.where(ok[..., None], CLASS_RGB[(E[..., None] >= CLASS_LO[1:]).sum(-1)], 0.0)
    err = np.abs(e - g) * (g > 0)
    ups = [1, 2, 4, 12, 16, max(192, err.max())]
    pts = [0, 0.25, 0.38, 0.66, 0.83, 0.95, 1]
    lo = 0
    for i, hi in enumerate(ups):
        m = (err > lo) & (err <= hi)
        if m.any():
            mn, mx = err[m].min(), err[m].max()
            err[m] = ((err[m] - mn) / (mx - mn + 1e-7)) * (pts[i + 1] - pts[i]) + pts[i]
        lo = hi
    jet = JET[np.minimum((err * 256).astype(np.int64), 255)]
    nb = [W // 8, W // 8, W // 4, W // 4, W // 8, W - (W // 4 + W // 4 + W // 8 + W // 8 + W // 8)]
    bar = np.concatenate([np.linspace(pts[i], pts[i + 1], nb[i]) for i in range(6)])
    legend = np.broadcast_to(JET[np.minimum((bar * 256).astype(np.int64), 255)], (50, W, 3))
    return disp_color, cls, np.concatenate((jet, legend), axis=0), (e * 256).astype('uint16')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=200)
    args = ap.parse_args()
    torch.set_num_threads(16)
    dev = torch.device("cuda:0")
    lines = ["render_bench: render_frame, every output, %dx%d from an estimate at %dx%d" % (H, W, LH, LW),
             "GPU: %s; CPU: %s, torch %s, numpy %s, %d threads" % (torch.cuda.get_device_name(0), platform.processor() or platform.machine(),
                                                                   torch.__version__, np.__version__, torch.get_num_threads())]
    for B in (1, 4):
        est, gt = scene(B, synth.SEED0 + 980 + B)
        dest, dgt = est.to(dev), gt.to(dev)
        for dtype, size in ((torch.uint8, 1), (torch.float32, 4)):
            fn = lambda: render_frame(dest, dgt, dtype=dtype)
            for _ in range(20):
                fn()
            torch.cuda.synchronize()
            eager = timed([fn], args.iters, warmup=0)[0]
            with _lib.Recorder() as rec:
                fn()
            torch.cuda.synchronize()
            plan = timed([rec.run], args.iters, warmup=0)[0]
            out_bytes = B * ((2 * H + H + H + 50) * W * 3 * size + H * W * 2)
            in_bytes = B * (H * W + LH * LW) * 4
            ceil = stream_ceilings(dev, [out_bytes])
            fill = list(ceil.values())[0]["fill"]
            ach = (out_bytes + in_bytes) / (plan[0] * 1e-6)
            tag = "B=%d %-7s" % (B, str(dtype).replace("torch.", ""))
            lines.append("%s (a) render_frame eager call   %8.1f us/call (median of 5 x %d; min %.1f)" % (tag, eager[0], args.iters, eager[1]))
            lines.append("%s (a) same launches, plan replay %8.1f us/call (median of 5 x %d; min %.1f)" % (tag, plan[0], args.iters, plan[1]))
            lines.append("%s     algorithmic bytes %.2f MB (read %.2f, written %.2f): %.0f GB/s, %.2f of the fill ceiling of this run "
                         "(%.0f GB/s on %.1f MB)" % (tag, (out_bytes + in_bytes) / 1e6, in_bytes / 1e6, out_bytes / 1e6, ach / 1e9,
                                                     ach / fill, fill / 1e9, out_bytes / 1e6))
        host = []
        for _ in range(3):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ce, cg = dest.cpu(), dgt.cpu()
            for b in range(B):
                host_frame(ce[b], cg[b])
            host.append((time.perf_counter() - t0) * 1e6)
        lines.append("B=%d         (b) .cpu() + numpy restatement %10.1f us/call (median of 3; min %.1f)" % (B, sorted(host)[1], min(host)))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
