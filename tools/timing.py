"""What the tools/*_bench.py scripts share: HIP-event timing, the table cell, the run's own bandwidth ceilings and the framework arm.
Each script keeps its own protocol (warm-up count, repetitions, one callable or alternating arms) and says so in its docstring."""
import torch

from temporalstereo_amd import _lib, layers


def span(fn, iters):
    """us per call of `iters` back-to-back calls between two HIP events"""
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1000.0 / iters


def timed(fns, iters, reps=5, warmup=3):
    """(median, min, max) of every callable, us per call: `warmup` untimed rounds over all of them, then `reps` repetitions of one span
    each, the callables alternating within every repetition"""
    for _ in range(warmup):
        for fn in fns:
            fn()
    torch.cuda.synchronize()
    per = [[] for _ in fns]
    for _ in range(reps):
        for p, fn in zip(per, fns):
            p.append(span(fn, iters))
    return [(sorted(p)[reps // 2], min(p), max(p)) for p in per]


def cell(t):
    return "%10.1f (%8.1f ..%8.1f)" % t if t is not None else "%32s" % "-"


def ceilings(dev):
    """bytes per second of a 256 MiB device fill (written) and copy (read + written)"""
    n = 256 << 20
    a, b = torch.empty(n, device=dev, dtype=torch.uint8), torch.zeros(n, device=dev, dtype=torch.uint8)
    lib, st = _lib.lib(), _lib.current_stream_handle()
    out = []
    for kind, mult in ((0, 1.0), (1, 2.0)):
        median = timed([lambda: lib.ts_calib_stream(kind, a.data_ptr(), b.data_ptr(), n, st)], 20, warmup=5)[0][0]
        out.append(mult * n / (median * 1e-6))
    return out


def torch_backend(fn):
    """`fn` under set_conv_backend('torch'): the framework's convolutions"""
    def run(*a):
        layers.set_conv_backend("torch")
        try:
            return fn(*a)
        finally:
            layers.set_conv_backend("hip")
    return run
