#!/usr/bin/env python
"""Time of preparing a batch of stereo frames (ToTensor + normalize + resize of both eyes), per geometry of BASELINE configs[1]-[4]:
  (a) the host method as the reference does it (video_inference.py:100-110 per image: from_numpy, permute, / 255, normalize,
      F.interpolate with align_corners) on this machine's CPU threads;
  (b) its upload: the fp32 color_aug tensors of both eyes, pageable memory, as `.to(device)` does;
  (c) the upload of the uint8 frames instead;
  (d) ts_frames_prepare_fwd on the device, color_aug only, at the same size and resized: eager calls and the same launch replayed
      from a plan (hipEvents around a loop after warm-up, median of 5 rounds), the algorithmic bytes (uint8 read once, fp32 written
      once) and the fraction of the fill ceiling measured in the same run on a stream of the output's size;
  (e) prepare_batch end to end (color + color_aug, the K pyramid, the 16-bit ground truth): three launches.
Then the observed maxima of the resized fixtures (tests/golden/prepare_*.npz) against their bars.
The file this writes records what was measured; it is not a pass criterion.
Usage: python tools/prepare_bench.py [--out FILE]"""
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
from temporalstereo_amd import _lib, preprocess as pp  # noqa: E402
from timing import timed  # noqa: E402

# (name, batch, source size, target size)
GEOMETRIES = (("config 1", 1, (480, 640), (544, 960)), ("config 2", 4, (480, 640), (544, 960)),
              ("config 3", 8, (480, 640), (480, 640)), ("config 4", 2, (375, 1242), (384, 1248)))
RESIZED = ("prepare_dataset_up", "prepare_video_up", "prepare_down", "prepare_degenerate")


def host_image(u8, size):
    image = torch.from_numpy(u8).permute(2, 0, 1).contiguous().to(torch.float32).div(255)
    mean, std = torch.tensor(pp.IMAGENET_MEAN), torch.tensor(pp.IMAGENET_STD)
    proc = (image - mean[:, None, None]) / std[:, None, None]
    if tuple(size) != tuple(u8.shape[:2]):
        proc = F.interpolate(proc.unsqueeze(dim=1), size=size, mode='bilinear', align_corners=True).squeeze(dim=1)
    return image, proc


def wall(fn, rounds=5):
    per = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        per.append((time.perf_counter() - t0) * 1e6)
    return sorted(per)[len(per) // 2], min(per)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=200)
    args = ap.parse_args()
    torch.set_num_threads(16)
    dev = torch.device("cuda:0")
    lines = ["prepare_bench: uint8 stereo frames -> color_aug of both eyes (ToTensor, normalize, align-corners resize)",
             "GPU: %s; CPU: %s, torch %s, numpy %s, %d threads" % (torch.cuda.get_device_name(0), platform.processor() or platform.machine(),
                                                                   torch.__version__, np.__version__, torch.get_num_threads())]
    for name, B, src, dst in GEOMETRIES:
        seed = synth.SEED0 + 990 + B
        u8 = [synth._rs(seed, tag).randint(0, 256, size=(B,) + src + (3,)).astype(np.uint8) for tag in ("L", "R")]
        tag = "%s B=%d %dx%d -> %dx%d" % ((name, B) + src + dst)
        host = lambda: [torch.stack([host_image(a[b], dst)[1] for b in range(B)]) for a in u8]
        host()
        t_host = wall(host)
        procs = host()
        t_up32 = wall(lambda: [p.to(dev) for p in procs])
        frames = [torch.from_numpy(a) for a in u8]
        t_up8 = wall(lambda: [f.to(dev) for f in frames])
        lines.append("%s" % tag)
        lines.append("  (a) host ToTensor + normalize + resize, both eyes   %10.1f us (median of 5; min %.1f)" % t_host)
        lines.append("  (b) upload of the fp32 color_aug, %6.2f MB          %10.1f us (median of 5; min %.1f)" % ((2 * B * 3 * dst[0] * dst[1] * 4 / 1e6,) + t_up32))
        lines.append("  (c) upload of the uint8 frames,   %6.2f MB          %10.1f us (median of 5; min %.1f)" % ((2 * B * 3 * src[0] * src[1] / 1e6,) + t_up8))
        dL, dR = (f.to(dev) for f in frames)
        forms = [("resized", src, dst)] if src != dst else []
        forms.append(("same size", dst, dst))
        kernel_us = None
        for form, s, d in forms:
            if s == src:
                a, b = dL, dR
            else:                       # the same-size form of a resized geometry: frames that already have the target size
                a, b = (torch.from_numpy(synth._rs(seed, t + "s").randint(0, 256, size=(B,) + d + (3,)).astype(np.uint8)).to(dev) for t in ("L", "R"))
            outs = tuple(torch.empty((B, 3) + d, device=dev) for _ in range(2))
            fn = lambda: pp.prepare_frames(a, b, size=d, color=False, out=outs)
            for _ in range(20):
                fn()
            torch.cuda.synchronize()
            eager = timed([fn], args.iters, warmup=0)[0]
            with _lib.Recorder() as rec:
                fn()
            torch.cuda.synchronize()
            plan = timed([rec.run], args.iters, warmup=0)[0]
            in_bytes, out_bytes = 2 * B * 3 * s[0] * s[1], 2 * B * 3 * d[0] * d[1] * 4
            fill = list(stream_ceilings(dev, [out_bytes]).values())[0]["fill"]
            ach = (in_bytes + out_bytes) / (plan[0] * 1e-6)
            lines.append("  (d) ts_frames_prepare_fwd %-9s eager call     %8.1f us (median of 5 x %d; min %.1f)" % ((form,) + (eager[0], args.iters, eager[1])))
            lines.append("  (d) ts_frames_prepare_fwd %-9s plan replay    %8.1f us (median of 5 x %d; min %.1f)" % ((form,) + (plan[0], args.iters, plan[1])))
            lines.append("      algorithmic bytes %.2f MB (read %.2f, written %.2f): %.0f GB/s, %.2f of the fill ceiling of this run (%.0f GB/s on %.1f MB)"
                         % ((in_bytes + out_bytes) / 1e6, in_bytes / 1e6, out_bytes / 1e6, ach / 1e9, ach / fill, fill / 1e9, out_bytes / 1e6))
            if kernel_us is None:
                kernel_us = plan[0]
        kn = torch.eye(4, dtype=torch.float64, device=dev)
        raw = torch.from_numpy(synth._rs(seed, "gt").randint(0, 65536, size=(B,) + src).astype(np.uint16).view(np.int16)).to(dev)
        fn = lambda: pp.prepare_batch(dL, dR, kn, 0.54, dst, disp_gt_raw=raw)
        for _ in range(20):
            fn()
        torch.cuda.synchronize()
        e2e = timed([fn], args.iters, warmup=0)[0]
        lines.append("  (e) prepare_batch (3 launches + allocations), eager   %8.1f us (median of 5 x %d; min %.1f)" % (e2e[0], args.iters, e2e[1]))
        lines.append("      (a)+(b) = %.1f us against (c)+(d) = %.1f us: %.0fx" % (t_host[0] + t_up32[0], t_up8[0] + kernel_us,
                                                                                 (t_host[0] + t_up32[0]) / (t_up8[0] + kernel_us)))
    golden = os.path.join(ROOT, "tests", "golden")
    lines.append("observed maxima of the resized fixtures (bars: dev32_64 and 1.5 x dev32_64)")
    for name in RESIZED:
        g = dict(np.load(os.path.join(golden, name + ".npz")))
        d32 = d64 = 0.0
        for k in range(int(g["subs"])):
            size = tuple(g["aug_l%d" % k].shape[-2:])
            r = pp.prepare_frames(torch.from_numpy(g["left%d" % k]).to(dev), torch.from_numpy(g["right%d" % k]).to(dev), size=size, color=False)
            for s in "lr":
                got = r["color_aug_" + s].cpu().numpy().astype(np.float64)
                ref32 = g["aug_%s%d" % (s, k)].astype(np.float64)
                d32 = max(d32, float(np.abs(got - ref32).max()))
                d64 = max(d64, float(np.abs(got - ref32 - g["d64_%s%d" % (s, k)]).max()))
        lines.append("  %-20s max |device - reference fp32| %.3g (bar %.3g)   max |device - reference fp64| %.3g (bar %.3g)"
                     % (name, d32, float(g["dev32_64"]), d64, 1.5 * float(g["dev32_64"])))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
