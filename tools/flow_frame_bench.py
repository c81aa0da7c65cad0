#!/usr/bin/env python
"""Time of the optical-flow metrics and pictures at 544x960, B = 1 and 4:
  metrics   flow_validation_metrics of four levels (full, 1/4, 1/4, 1/8) against one ground truth: one launch pair;
  render    render_flow_frame of a 1/4-resolution estimate with every output (estimate above ground truth with a shared maximum
            radius, error classes), uint8 HWC: a statistics launch pair and the colour launch.
Per workload and batch:
  (a) the eager call (hipEvents around a loop of calls);
  (b) the same launches recorded once and replayed as a plan (no Python between them);
  (c) the same results composed from framework ops on the same GPU in the same run (F.interpolate, elementwise ops, reductions,
      a gather into the colour wheel);
  (d) the reference's semantics on the CPU: tests/flow_frame_ref.py, numpy float32, image by image.
Usage: python tools/flow_frame_bench.py [--out FILE]"""
import argparse
import math
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

import flow_frame_ref as R  # noqa: E402
import synth  # noqa: E402
from temporalstereo_amd import _lib, flow_validation_metrics, make_color_wheel, render_flow_frame  # noqa: E402
from timing import timed  # noqa: E402

H, W = 544, 960
LEVELS = [(H, W), (H // 4, W // 4), (H // 4, W // 4), (H // 8, W // 8)]


def scene(B, seed):
    g = lambda tag, shape, s: torch.from_numpy(synth.normal(seed, tag, shape, s))
    gt = g("gt", (B, 2, H, W), 25.0)
    gt[:, :, :40, :200] = 0.0                                                      # a hole, as in a sparse ground truth
    ests = [g("e%d" % i, (B, 2, h, w), 25.0 * w / W) for i, (h, w) in enumerate(LEVELS)]
    return gt, ests


def rescale(e, size):
    s = torch.tensor([size[1] / e.shape[-1], size[0] / e.shape[-2]], device=e.device, dtype=torch.float32).view(1, 2, 1, 1)
    return e if tuple(e.shape[-2:]) == tuple(size) else F.interpolate(e, size=size, mode='bilinear', align_corners=True) * s


def torch_metrics(ests, gt, lb=0.0, ub=400.0):
    gu, gv = gt[:, 0], gt[:, 1]
    rad = torch.sqrt(gu * gu + gv * gv)
    mask = ~((gu.abs() < 1e-12) & (gv.abs() < 1e-12)) & ~(torch.isnan(gu) | torch.isnan(gv)) & (rad > lb) & (rad < ub)
    n = mask.sum().float()
    out = []
    for e in ests:
        f = rescale(e, gt.shape[-2:])
        err = torch.sqrt((gu - f[:, 0]) ** 2 + (gv - f[:, 1]) ** 2)
        err = torch.where(mask, err, torch.zeros_like(err))
        out.append(torch.stack([(err > t).sum().float() / n * 100 for t in (1, 2, 3, 5)] + [err.double().sum().float() / n]))
    return torch.stack(out)


def torch_flow_color(f, maxr, wheel):
    u, v = f[:, 0], f[:, 1]
    unk = (u.abs() > 1e7) | (v.abs() > 1e7) | torch.isnan(u) | torch.isnan(v)
    u, v = torch.where(unk, torch.zeros_like(u), u), torch.where(unk, torch.zeros_like(v), v)
    r0 = torch.sqrt(u * u + v * v)
    den = (maxr + 2.0 ** -52).view(-1, 1, 1)
    un, vn = u / den, v / den
    rad = torch.sqrt(un * un + vn * vn)
    fk = (torch.atan2(-vn, -un) / math.pi + 1) / 2 * 54 + 1
    k0 = fk.floor().clamp(1, 55).long()
    k1 = torch.where(k0 == 55, torch.ones_like(k0), k0 + 1)
    fr = (fk - k0).unsqueeze(-1)
    col = (1 - fr) * wheel[k0 - 1] + fr * wheel[k1 - 1]
    inside = (r0 <= maxr.view(-1, 1, 1)).unsqueeze(-1)
    col = torch.where(inside, 1 - rad.unsqueeze(-1) * (1 - col), col * 0.75)
    return torch.where(unk.unsqueeze(-1), torch.zeros_like(col), col)


def torch_render(est, gt, wheel, lo, rgb):
    f = rescale(est, gt.shape[-2:])
    rad = lambda m: torch.sqrt(m[:, 0] ** 2 + m[:, 1] ** 2).flatten(1).max(dim=1).values
    maxr = torch.maximum(rad(f), rad(gt))
    pic = torch.cat([torch_flow_color(f, maxr, wheel), torch_flow_color(gt, maxr, wheel)], dim=1)
    E = torch.sqrt((gt[:, 0] - f[:, 0]) ** 2 + (gt[:, 1] - f[:, 1]) ** 2)
    cls = (E.unsqueeze(-1) >= lo).sum(dim=-1) - 1
    err = rgb[cls.clamp(min=0)]
    q8 = lambda c: (c.clamp(0, 1) * 255 + 0.5).floor().to(torch.uint8)
    return q8(pic), q8(err)


def cpu_metrics(ests, gt):
    return [R.calc_error(R.rescale(e, gt.shape[-2:]), gt, 0.0, 400, True)[0] for e in ests]


def cpu_render(est, gt):
    f = R.rescale(est, gt.shape[-2:])
    fh, gh = R.hwc(f), R.hwc(gt)
    out = []
    for b in range(gt.shape[0]):
        m = max(R.max_rad(fh[b]), R.max_rad(gh[b]))
        out.append(R.q8(np.concatenate([R.flow_to_color(fh[b], m, data_max=True), R.flow_to_color(gh[b], m, data_max=True)])))
    return out, R.q8(R.class_colors(R.err_class(f, gt)))


def cpu_time(fn, reps=3):
    fn()
    per = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        per.append((time.perf_counter() - t0) * 1e6)
    return sorted(per)[len(per) // 2], min(per)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=200)
    args = ap.parse_args()
    torch.set_num_threads(16)
    dev = torch.device("cuda:0")
    wheel = torch.from_numpy((make_color_wheel() / 255).astype(np.float32)).to(dev)
    lo = torch.from_numpy(R.CLASS_LO).to(dev)
    rgb = torch.from_numpy(R.CLASS_RGB / np.float32(255)).to(dev)
    lines = ["flow_frame_bench: optical-flow metrics (levels %s, sparse) and render_flow_frame (estimate %s, every output, uint8 HWC) at %dx%d"
             % (LEVELS, LEVELS[1], H, W),
             "GPU: %s; CPU: %s, torch %s, numpy %s, %d threads" % (torch.cuda.get_device_name(0), platform.processor() or platform.machine(),
                                                                   torch.__version__, np.__version__, torch.get_num_threads())]
    for B in (1, 4):
        gt, ests = scene(B, synth.SEED0 + 9700 + B)
        dgt, dests = gt.to(dev), [e.to(dev) for e in ests]
        work = (("metrics", lambda: flow_validation_metrics(dests, dgt, sparse=True), lambda: torch_metrics(dests, dgt),
                 lambda: cpu_metrics([e.numpy() for e in ests], gt.numpy())),
                ("render ", lambda: render_flow_frame(dests[1], dgt), lambda: torch_render(dests[1], dgt, wheel, lo, rgb),
                 lambda: cpu_render(ests[1].numpy(), gt.numpy())))
        for name, ours, framework, cpu in work:
            a = timed([ours], args.iters, warmup=10)[0]
            with _lib.Recorder() as rec:
                ours()
            torch.cuda.synchronize()
            b = timed([rec.run], args.iters, warmup=10)[0]
            c = timed([framework], max(args.iters // 10, 5), warmup=10)[0]
            d = cpu_time(cpu)
            lines.append("B=%d %s (a) eager call                 %9.1f us/call (median of 5 x %d; min %.1f)" % (B, name, a[0], args.iters, a[1]))
            lines.append("B=%d %s (b) same launches, plan replay %9.1f us/call (median of 5 x %d; min %.1f)" % (B, name, b[0], args.iters, b[1]))
            lines.append("B=%d %s (c) framework ops, same GPU    %9.1f us/call (median of 5 x %d; min %.1f)   (c) / (b) = %.1f"
                         % (B, name, c[0], max(args.iters // 10, 5), c[1], c[0] / b[0]))
            lines.append("B=%d %s (d) reference semantics, CPU   %9.1f us/call (median of 3; min %.1f)" % (B, name, d[0], d[1]))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
