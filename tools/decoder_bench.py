#!/usr/bin/env python
"""Time of FeatureDecoder (temporalstereo_amd.FeatureDecoder; csrc/feature_decoder.hip) at the reference's geometry for a 544 x 960
image -- x32 17x30, x16 34x60, x8 68x120, x4 136x240, both eyes batched -- at batch 2 and 8: each of the seven layers and the whole
decoder, two legs:
  eval forward               under no_grad, BatchNorm's running statistics folded into the convolution's epilogue;
  train forward + backward   batch statistics, and the gradients of every input and parameter.
Arms, alternating within every repetition, in one process:
  (a) the kernel path: functional.decoder_conv / the module;
  (b) fused layers, eval forward: the unfused form of the same kernel -- ts_resize_bilinear_fwd, a concatenation copy, the Cu = 0 call;
  (c) the framework: the same layers.Conv2d wrappers (the module's _reference_forward) under set_conv_backend('torch');
  (x6) plain layers the entry accepts (W % 4 == 0), eval forward: the existing ts_conv3d_hw_x6_fwd on a weight split beforehand -- the
       yardstick for a later bf16-split form of these layers.
Outputs of (a) are compared with (c) before anything is timed.  us per call: median of 21 timed windows of N calls (min .. max of the 21),
after three untimed rounds of every arm.
Usage: python tools/decoder_bench.py [--out FILE] [--reps R]"""
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
from temporalstereo_amd import _lib  # noqa: E402
from temporalstereo_amd import functional as TF  # noqa: E402
from timing import cell, timed, torch_backend  # noqa: E402

PLANES = {"x32": (17, 30), "x16": (34, 60), "x8": (68, 120), "x4": (136, 240)}
#          layer            up source  skip   (None: the plain form on the previous layer's output)
LAYERS = [("conv32", None, "x32"), ("deconv32_16.0", "x32", "x16"), ("deconv32_16.1", None, "x16"), ("deconv16_8.0", "x16", "x8"),
          ("deconv16_8.1", None, "x8"), ("deconv8_4.0", "x8", "x4"), ("deconv8_4.1", None, "x4")]


def conv_of(m, name):
    mod = m
    for part in name.split("."):
        mod = mod[int(part)] if part.isdigit() else getattr(mod, part)
    return mod


def layer_arms(m, name, up, skip, cot):
    """closures of one layer: dict(leg -> [(arm, fn)])"""
    conv = conv_of(m, name)
    act = conv._fusable() if conv.norm is not None else None
    L = _lib.lib()
    dev = skip.device
    B, Cs, H, W = skip.shape
    Cu = up.shape[1] if up is not None else 0
    Cout = conv.weight.shape[0]

    def kernel(u, s):
        return TF.decoder_conv(u, s, conv.weight, conv.bias, conv.norm, act)

    def framework(u, s):
        x = s if u is None else torch.cat([F.interpolate(u, size=(H, W), mode="bilinear", align_corners=True), s], 1)
        return conv(x)
    framework = torch_backend(framework)

    def unfused(u, s):
        x = torch.empty((B, Cu + Cs, H, W), device=dev)
        _lib.check(L.ts_resize_bilinear_fwd(_lib.ptr(u), _lib.ptr(x), B, Cu, u.shape[2], u.shape[3], H, W, 1.0, (Cu + Cs) * H * W,
                                            _lib.current_stream_handle()), "ts_resize_bilinear_fwd")
        x[:, Cu:].copy_(s)
        return TF.decoder_conv(None, x, conv.weight, conv.bias, conv.norm, act)

    x6 = None
    if up is None and L.ts_conv3d_hw_x6_supported(Cs, Cout, W, 1, 1, 0):
        w6 = torch.empty(TF._q("ts_conv3d_hw_x6_weight_bytes", Cs, Cout), device=dev, dtype=torch.uint8)
        _lib.check(L.ts_conv3d_hw_x6_weight_split_from(_lib.ptr(conv.weight.detach()), _lib.ptr(w6), Cs, Cout, 9, Cs * 9, 1, 0,
                                                       _lib.current_stream_handle()), "ts_conv3d_hw_x6_weight_split_from")
        wsb = TF._q("ts_conv3d_hw_x6_workspace_bytes", B, Cs, Cout, 1, H, W)
        ws = torch.empty(wsb, device=dev, dtype=torch.uint8) if wsb else None

        def x6(u, s):
            y = torch.empty((B, Cout, H, W), device=dev)
            _lib.check(L.ts_conv3d_hw_x6_fwd(_lib.ptr(s), _lib.ptr(w6), None, None, _lib.ptr(y), B, Cs, Cout, 1, H, W, 1, 0, 0.0, s.stride(0),
                                             s.stride(1), y.stride(0), y.stride(1), None, 0, _lib.ptr(ws), wsb, _lib.current_stream_handle()),
                       "ts_conv3d_hw_x6_fwd")
            return y

    ug = up.clone().requires_grad_(True) if up is not None else None
    sg = skip.clone().requires_grad_(True)
    wrt = [t for t in (ug, sg) if t is not None] + list(conv.parameters())

    def fwd(fn):
        def run():
            with torch.no_grad():
                return fn(up, skip)
        return run

    def both(fn):
        return lambda: torch.autograd.grad(fn(ug, sg), wrt, cot)
    return dict(kernel=kernel, framework=framework, unfused=unfused if up is not None else None, x6=x6, fwd=fwd, both=both)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--reps", type=int, default=21)
    ap.add_argument("--batches", type=int, nargs="+", default=[2, 8])
    args = ap.parse_args()
    assert args.reps >= 20
    dev = torch.device("cuda:0")
    lines = ["decoder_bench: FeatureDecoder at x32 17x30, x16 34x60, x8 68x120, x4 136x240; us per call, median of %d windows of N calls "
             "(min .. max of them); N is stated per batch" % args.reps,
             "GPU: %s; CPU: %s, torch %s" % (torch.cuda.get_device_name(0), platform.processor() or platform.machine(), torch.__version__),
             "(a) functional.decoder_conv / the module; (b) ts_resize_bilinear_fwd + concatenation copy + the Cu = 0 call; (c) the same wrappers, "
             "set_conv_backend('torch'); (x6) ts_conv3d_hw_x6_fwd, weight split beforehand",
             "the row that names a layer is its eval forward; the row below it its train forward + backward"]
    head = "%-44s %32s %32s %32s %32s %8s %8s" % ("layer [B, Cu+Cs -> Cout, H x W], leg", "(a) kernel path", "(b) unfused, same kernel", "(c) framework",
                                               "(x6) bf16-split yardstick", "(b)/(a)", "(c)/(a)")
    slower_than_unfused, slower_than_framework = [], []
    print("\n".join(lines), flush=True)

    def emit(line):             # as it comes: a run of minutes shows where it is
        lines.append(line)
        print(line, flush=True)
    for B in args.batches:
        iters = 4 if B <= 2 else 2
        g = torch.Generator().manual_seed(B)
        m = ts.FeatureDecoder()
        with torch.no_grad():
            for p in m.parameters():
                if p.dim() == 4:
                    p.copy_(torch.randn(p.shape, generator=g) * (2.0 / (9 * p.shape[1]) ** 0.5))
        m = m.to(dev)
        maps = {k: torch.randn((B, c) + PLANES[k], generator=g).to(dev) for k, c in zip(("x4", "x8", "x16", "x32"), m.channels[1:])}
        m.eval()
        with torch.no_grad():
            own = m(maps["x4"], maps["x8"], maps["x16"], maps["x32"])
            ref = torch_backend(m._reference_forward)(maps["x4"], maps["x8"], maps["x16"], maps["x32"])
        rel = [float((a - b).norm() / b.norm()) for a, b in zip(own, ref)]
        emit("batch %d: N = %d; relative L2 of the module's [x4, x8, x16] against (c): %s" % (B, iters, ", ".join("%.2e" % r for r in rel)))
        assert max(rel) < 1e-4, rel
        emit(head)
        # the inputs of every layer: the eval pass's own intermediate maps
        feeds, prev = {}, None
        with torch.no_grad():
            for name, up_src, skip_src in LAYERS:
                conv = conv_of(m, name)
                up, skip = (prev, maps[skip_src]) if up_src is not None else (None, prev if prev is not None else maps[skip_src])
                feeds[name] = (up, skip)
                prev = TF.decoder_conv(up, skip, conv.weight, conv.bias, conv.norm, conv._fusable() if conv.norm is not None else None)
        for name, _, _ in LAYERS:
            up, skip = feeds[name]
            conv = conv_of(m, name)
            Cout, Cin = conv.weight.shape[:2]
            Bq, _, H, W = skip.shape
            cot = torch.randn((Bq, Cout, H, W), generator=g).to(dev)
            a = layer_arms(m, name, up, skip, cot)
            label = "%s [%d, %d -> %d, %dx%d]" % (name, B, Cin, Cout, H, W)
            for leg, training in (("eval forward", False), ("train forward + backward", True)):
                m.train(training)
                wrap = a["both"] if training else a["fwd"]
                arms = [("a", a["kernel"]), ("c", a["framework"])]
                if not training:
                    arms += [(k, a[n]) for k, n in (("b", "unfused"), ("x6", "x6")) if a[n] is not None]
                t = dict(zip([k for k, _ in arms], timed([wrap(fn) for _, fn in arms], iters, args.reps)))
                if "b" in t and t["a"][0] > t["b"][2]:
                    slower_than_unfused.append("%s: (a) %.1f us against (b) %.1f us (max %.1f)" % (label, t["a"][0], t["b"][0], t["b"][2]))
                if t["a"][0] > t["c"][0]:
                    slower_than_framework.append("%s %s: %.2f x" % (label, leg, t["a"][0] / t["c"][0]))
                emit("%-44s %s %s %s %s %8s %8.2f" % (label if not training else "%44s" % leg, cell(t["a"]), cell(t.get("b")), cell(t["c"]),
                                                              cell(t.get("x6")), ("%.2f" % (t["b"][0] / t["a"][0])) if "b" in t else "-",
                                                              t["c"][0] / t["a"][0]))
            del a, cot
        # the whole decoder
        grads = {k: v.clone().requires_grad_(True) for k, v in maps.items()}
        cots = [torch.randn(o.shape, generator=g).to(dev) for o in own]
        wrt = list(grads.values()) + list(m.parameters())
        order = ("x4", "x8", "x16", "x32")
        for leg, training in (("eval forward", False), ("train forward + backward", True)):
            m.train(training)
            fns = []
            for fn in (m, torch_backend(m._reference_forward)):
                if training:
                    fns.append(lambda fn=fn: torch.autograd.grad(fn(*[grads[k] for k in order]), wrt, cots))
                else:
                    def run(fn=fn):
                        with torch.no_grad():
                            return fn(*[maps[k] for k in order])
                    fns.append(run)
            ta, tc = timed(fns, iters, args.reps)
            if ta[0] > tc[0]:
                slower_than_framework.append("whole decoder [%d] %s: %.2f x" % (B, leg, ta[0] / tc[0]))
            emit("%-44s %s %s %s %s %8s %8.2f" % (("whole decoder [%d]" % B) if not training else "%44s" % leg, cell(ta), cell(None), cell(tc),
                                                          cell(None), "-", tc[0] / ta[0]))
        del m, maps, grads, cots, own, ref, feeds
        torch.cuda.empty_cache()
    emit("fused layers whose median is above the unfused form's maximum: " + ("; ".join(slower_than_unfused) if slower_than_unfused else "none"))
    emit("legs where the kernel path's median is the slower one against the framework: " +
                 ("; ".join(slower_than_framework) if slower_than_framework else "none"))
    text = "\n".join(lines) + "\n"
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text)


if __name__ == "__main__":
    main()
