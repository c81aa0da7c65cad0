#!/usr/bin/env python
"""Time of the validation / test metrics at 544x960 with four levels (full, 1/4, 1/4, 1/8) and the occlusion split:
  (a) temporalstereo_amd.validation_metrics on the GPU (hipEvents around a loop of calls; one launch pair per call);
  (b) the reference's semantics on the CPU at 16 threads, restated here in torch: validation_step's F.interpolate per level, then
      log_metric's do_evaluation + do_occlusion_evaluation per level (projects/TemporalStereo/TemporalStereo.py:183, :463-486;
      data/evaluation/eval.py, pixel_error.py), the 2-D inverse_warp recomputed for every level as the reference does.
Usage: python tools/eval_bench.py [--out FILE]"""
import argparse
import os
import platform
import sys
import time

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import synth  # noqa: E402
from temporalstereo_amd import validation_metrics  # noqa: E402
from timing import timed  # noqa: E402

H, W = 544, 960
LEVELS = [(H, W), (H // 4, W // 4), (H // 4, W // 4), (H // 8, W // 8)]


def scene(B, seed):
    g = lambda tag, shape, lo, hi: torch.from_numpy(synth.uniform(seed, tag, shape, lo, hi))
    gl = g("gl", (B, 1, H, W), 1.0, 150.0)
    gr = g("gr", (B, 1, H, W), 1.0, 150.0)
    ests = [g("e%d" % i, (B, 1, h, w), 0.0, 150.0 * w / W) for i, (h, w) in enumerate(LEVELS)]
    return gl, gr, ests


def calc_error(est, gt, lb, ub):
    est, gt = est.clone().cpu(), gt.clone().cpu()
    mask = (gt > lb) & (gt < ub)
    if abs(mask.float().sum()) < 1.0:
        return [torch.Tensor([0.])] * 5
    a = torch.abs(gt[mask] - est[mask])
    n = mask.float().sum()
    return [torch.Tensor([torch.sum(torch.gt(a, t).float()) / n * 100]) for t in (1, 2, 3, 5)] + [torch.Tensor([a.float().mean()])]


def occlusion(gl, gr):
    B, _, h, w = gl.shape
    x = torch.arange(w, dtype=torch.float32).view(1, 1, 1, w).expand(B, 1, h, w)
    y = torch.arange(h, dtype=torch.float32).view(1, 1, h, 1).expand(B, 1, h, w)
    X = x[:, 0] + (-gl)[:, 0]
    grid = torch.stack((2 * X / (w - 1) - 1, 2 * y[:, 0] / (h - 1) - 1), dim=3)
    warp = F.grid_sample(gr, grid, mode='bilinear', padding_mode='zeros', align_corners=True)
    return (((warp - gl).abs() > 1.0) | (warp.abs() < 1e-6)).prod(dim=1, keepdim=True).type_as(gl).clamp(0, 1)


def cpu_log_metric(ests, gl, gr, lb=0, ub=192):
    full = [F.interpolate(d * W / d.shape[-1], size=(H, W), mode='bilinear', align_corners=True) for d in ests]
    out = []
    for d in full:
        out.append(calc_error(d, gl, lb, ub))
        occ = occlusion(gl.clone().cpu(), gr.clone().cpu())          # do_occlusion_evaluation warps once per level
        out.append(calc_error(d * occ, gl * occ, lb, ub))
        out.append(calc_error(d * (1.0 - occ), gl * (1.0 - occ), lb, ub))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--iters", type=int, default=200)
    args = ap.parse_args()
    torch.set_num_threads(16)
    dev = torch.device("cuda:0")
    lines = ["eval_bench: validation metrics at %dx%d, levels %s, occlusion split on, lb=0 ub=192" % (H, W, LEVELS),
             "GPU: %s; CPU: %s, torch %s, %d threads" % (torch.cuda.get_device_name(0), platform.processor() or platform.machine(),
                                                         torch.__version__, torch.get_num_threads())]
    for B in (1, 4):
        gl, gr, ests = scene(B, synth.SEED0 + 900 + B)
        dgl, dgr, dests = gl.to(dev), gr.to(dev), [e.to(dev) for e in ests]
        eager = timed([lambda: validation_metrics(dests, dgl, dgr)], args.iters, warmup=20)[0]
        # device time alone: the two launches recorded once and replayed as a plan (no Python between them)
        from temporalstereo_amd import _lib
        with _lib.Recorder() as rec:
            validation_metrics(dests, dgl, dgr)
        torch.cuda.synchronize()
        replay = timed([rec.run], args.iters, warmup=0)[0]
        cpu_log_metric(ests, gl, gr)
        cpu = []
        for _ in range(3):
            t0 = time.perf_counter()
            cpu_log_metric(ests, gl, gr)
            cpu.append((time.perf_counter() - t0) * 1e6)
        med = lambda v: sorted(v)[len(v) // 2]
        lines.append("B=%d  (a) validation_metrics eager call  %8.1f us/call (median of 5 x %d; min %.1f)" % (B, eager[0], args.iters, eager[1]))
        lines.append("B=%d  (a) same launches, plan replay    %8.1f us/call (median of 5 x %d; min %.1f)" % (B, replay[0], args.iters, replay[1]))
        lines.append("B=%d  (b) reference semantics, CPU      %8.1f us/call (median of 3; min %.1f)" % (B, med(cpu), min(cpu)))
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
