"""What the module tests share: the device, bit equality, the error measures, the bars' common forms and the line that reaches
profiles/*_parity.txt.  Which bar a test uses, and why, stays in that test file's docstring; the factor 4 is argued in
tests/test_raft_corr_gpu.py."""
import os

import numpy as np
import torch

from temporalstereo_amd import _lib

U = 2.0 ** -24


def dev():
    return torch.device("cuda", torch.cuda.current_device())


def gpu(x):
    """a tensor or a numpy array on the device; None stays None"""
    if x is None:
        return None
    return (x if torch.is_tensor(x) else torch.from_numpy(np.ascontiguousarray(x))).to(dev())


def same_bits(a, b):
    return a.shape == b.shape and torch.equal(a.contiguous().view(torch.int32), b.contiguous().view(torch.int32))


def T(a):
    return torch.from_numpy(np.asarray(a))


def err(a, b):
    return float((a.double() - b.double()).abs().max())


def rel_l2(a, b, ref=None, *, keep=None):
    """relative L2 of a - b in units of |ref| (|b| without one); with `keep`, over the elements it keeps, and 0 where both vanish there"""
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    if keep is None:
        return float((a - b).norm() / (b if ref is None else ref.detach().cpu().double()).norm())
    assert ref is None
    a, b = a * keep, b * keep
    return float((a - b).norm() / b.norm().clamp_min(1e-300))


def stage_bar(dev, peak):
    return max(4.0 * dev, 16.0 * U * peak)


def fp32_bar(g, name):
    """an fp32 run against fp64, from a fixture's dev_* and max_* (tests/test_mbconv_cpu.py's docstring)"""
    return max(2.0 * float(g["dev_" + name]), 16.0 * U * float(g["max_" + name]))


def fp32_rel_bar(g, name):
    return max(2.0 * float(g["rel_" + name]), 1e-6)


class Parity:
    """One test module's report: every line is printed and, with the environment variable `env` set, appended to the file it names."""

    def __init__(self, env, width=64):
        self.env, self.width = env, width

    def report(self, line):
        print(line)
        path = os.environ.get(self.env)
        if path:
            with open(path, "a") as fh:
                fh.write(line + "\n")

    def check(self, name, got, want, bar):
        """max over the elements of |got - want| / bar <= 1 (bar a scalar or a tensor)."""
        err = (got.double().cpu() - want.double().cpu()).abs()
        bar = torch.as_tensor(bar, dtype=torch.float64)
        ratio = float((err / bar).max()) if bar.numel() > 1 else float(err.max()) / float(bar)
        self.report("%-*s max |err| %.3e  bar %.3e  err / bar %.3f" % (self.width, name, float(err.max()), float(bar.max()), ratio))
        assert ratio <= 1.0, name

    def check_rel(self, name, got, want, ref, bar):
        """relative L2 of got - want, in units of |ref|"""
        err = rel_l2(got, want, ref)
        self.report("%-*s rel L2    %.3e  bar %.3e  err / bar %.3f" % (self.width, name, err, bar, err / bar))
        assert err <= bar, name

    def against_fp64(self, name, got, fn, args):
        """`got` against fn(*args) in fp64, the bar from fn in fp32 (both on the CPU)."""
        w64 = fn(*[a.double() if torch.is_tensor(a) and a.is_floating_point() else a for a in args])
        w32 = fn(*args)
        self.check(name, got, w64, stage_bar(float((w32.double() - w64).abs().max()), float(w64.abs().max())))
        return w64


def null_sweep(fn, args, pointers, what):
    """NULL in every required pointer position -> -1."""
    for i in pointers:
        a = list(args)
        a[i] = None
        assert fn(*a) == -1 and b"NULL" in _lib.lib().ts_last_error_string(), (what, i)
