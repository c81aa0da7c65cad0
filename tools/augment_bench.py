#!/usr/bin/env python
"""Time of augmenting a batch of training frames on the device (temporalstereo_amd/augment.py), 540 x 960 frames -> a 512 x 960 window
(the reference's SceneFlow training size), B = 1, 4, 8, three parameter mixes:
  none      no image is colour-augmented (identity table): the same window bytes as prepare_frames(size, crop) plus the table read
  no hue    every image: brightness, contrast, saturation in drawn orders + gamma, rectangles on half the right eyes
  all       every image: the four operations in drawn orders + gamma, rectangles on half the right eyes
beside prepare_frames(size, crop) on the same frames in the same run (a), and prepare_train_batch (frames, K pyramid, 16-bit ground
truth).  Per call: hipEvents around a loop of warm calls, median of 5 rounds x --iters calls (>= 100 calls in all).
(b) the statistics launch: the call at a 4 x 4 window (the apply launch is then one block per image), contrast last in every order, so
    the full frames are read and three operations evaluated per pixel; its frame bytes per second against the copy ceiling measured
    in the same run on a stream of the same size.
(c) images per second against the host chain: ColorJitter + AdjustGamma as PIL calls on one 540 x 960 image, one thread, timed here
    when PIL is installed.
The file this writes records what was measured; it is not a pass criterion.
Usage: python tools/augment_bench.py [--out FILE] [--iters N]"""
import argparse
import os
import platform
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from benchlegs.k1 import stream_ceilings  # noqa: E402
from temporalstereo_amd import augment as ag, preprocess as pp  # noqa: E402
from timing import timed  # noqa: E402

SRC, WIN = (540, 960), (512, 960)


def mix(name, B, dev, size=WIN):
    if name == "none":
        return ag.Augmentation.identity(B, crop=[(14, 0)] * B, device=dev)
    a = ag.draw_augmentation(B, SRC, size, seed=5, p_color=1.0, p_occlusion=0.5,
                             patch_w=(min(50, size[1]), min(250, size[1])), patch_h=(min(50, size[0]), min(180, size[0])))
    if name == "no hue":
        a.order = np.where(a.order == ag.HUE, ag.NONE, a.order)
    elif name == "contrast last":
        a.order[:] = (ag.BRIGHTNESS, ag.SATURATION, ag.HUE, ag.CONTRAST)
    return a.to(dev)


def host_chain_ms():
    try:
        from PIL import Image, ImageEnhance
    except ImportError:
        return None
    img = Image.fromarray(np.random.RandomState(0).randint(0, 256, size=SRC + (3,)).astype(np.uint8), "RGB")
    table = [int(v) for v in ag.gamma_table(0.9)] * 3

    def chain():
        x = ImageEnhance.Brightness(img).enhance(1.3)
        x = ImageEnhance.Contrast(x).enhance(0.8)
        x = ImageEnhance.Color(x).enhance(1.2)
        h, s, v = x.convert("HSV").split()
        h = Image.fromarray((np.array(h, dtype=np.uint8).astype(np.int64) + 12).astype(np.uint8), "L")
        return Image.merge("HSV", (h, s, v)).convert("RGB").point(table)
    chain()
    per = []
    for _ in range(5):
        t0 = time.perf_counter()
        chain()
        per.append((time.perf_counter() - t0) * 1e3)
    return sorted(per)[2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=40)
    args = ap.parse_args()
    dev = torch.device("cuda:0")
    lines = ["augment_bench: uint8 stereo frames %dx%d -> color + color_aug of both eyes at a %dx%d window" % (SRC + WIN),
             "GPU: %s; CPU: %s, torch %s, numpy %s" % (torch.cuda.get_device_name(0), platform.processor() or platform.machine(),
                                                       torch.__version__, np.__version__),
             "per call: hipEvents around %d warm calls, median of 5 rounds (minimum in brackets)" % args.iters]
    host = host_chain_ms()
    lines.append("(c) host chain (PIL, one thread, this machine): " + ("%.1f ms per image = %.1f images/s" % (host, 1e3 / host)
                                                                       if host else "PIL is not installed here: not timed"))
    kn = torch.tensor([[0.58, 0, 0.5, 0], [0, 1.92, 0.5, 0], [0, 0, 1, 0], [0, 0, 0, 1]], dtype=torch.float32, device=dev)
    for B in (1, 4, 8):
        rs = np.random.RandomState(B)
        L = torch.from_numpy(rs.randint(0, 256, size=(B,) + SRC + (3,)).astype(np.uint8)).to(dev)
        Rt = torch.from_numpy(rs.randint(0, 256, size=(B,) + SRC + (3,)).astype(np.uint8)).to(dev)
        raw = torch.from_numpy(rs.randint(0, 32768, size=(B,) + SRC).astype(np.int16)).to(dev)
        base = torch.full((B,), 0.54, device=dev)
        crop = torch.tensor([(14, 0)] * B, dtype=torch.int32, device=dev)
        lines.append("B = %d" % B)
        fn = lambda: pp.prepare_frames(L, Rt, size=WIN, crop=crop)
        fn(); torch.cuda.synchronize()
        ref = timed([fn], args.iters, warmup=0)[0][:2]
        lines.append("  prepare_frames(size, crop)            %8.1f us (%.1f)" % ref)
        for name in ("none", "no hue", "all"):
            a = mix(name, B, dev)
            fn = lambda: ag.augment_frames(L, Rt, a, WIN)
            fn(); torch.cuda.synchronize()
            t = timed([fn], args.iters, warmup=0)[0][:2]
            fb = lambda: ag.prepare_train_batch(L, Rt, kn, base, WIN, a, disp_gt_raw=raw)
            fb(); torch.cuda.synchronize()
            tb = timed([fb], args.iters, warmup=0)[0][:2]
            lines.append("  augment_frames  %-8s              %8.1f us (%.1f)  %.2f x prepare_frames  %8.0f images/s%s" % (
                (name,) + t + (t[0] / ref[0], 2 * B / (t[0] * 1e-6), ("  = %.0f x the host chain" % (2 * B / (t[0] * 1e-6) * host / 1e3)) if host else "")))
            lines.append("  prepare_train_batch %-8s          %8.1f us (%.1f)" % ((name,) + tb))
        a = mix("contrast last", B, dev, size=(4, 4))
        fn = lambda: ag.augment_frames(L, Rt, a, (4, 4))
        fn(); torch.cuda.synchronize()
        t = timed([fn], args.iters, warmup=0)[0][:2]
        nbytes = 2 * B * SRC[0] * SRC[1] * 3
        ceil = list(stream_ceilings(dev, [2 * nbytes]).values())[0]["copy"]
        lines.append("  (b) statistics launch (4x4 window, contrast last) %8.1f us (%.1f): %.2f MB of frames read, %.0f GB/s = %.2f of the copy "
                     "ceiling of this run (%.0f GB/s moving %.1f MB)" % (t + (nbytes / 1e6, nbytes / (t[0] * 1e-6) / 1e9, nbytes / (t[0] * 1e-6) / ceil,
                                                                        ceil / 1e9, 2 * nbytes / 1e6)))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
