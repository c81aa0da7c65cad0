"""Bit digest of the convolution autograd nodes of temporalstereo_amd.functional over a fixed list of small cases.

One line per case: the case's name, then `what=<digest>` for the output, every gradient the case has (x, weight, bias, gamma, beta,
addend, up, skip) and, where a BatchNorm is involved, its running statistics and num_batches_tracked.  A digest is the first 16 hex
digits of the SHA-256 of the tensor's bytes (shape and dtype included).  The tool goes through the public functions only (conv3d,
conv_transpose3d, conv_transpose2d_k4s2, conv3d_k333, conv_bn_act, decoder_conv, conv_gru, mbconv_eval, depthwise_conv3x3, conv3x3_bn_act,
fused_mbconv_eval, the layers wrappers), so two trees can be compared line by line: a refactor must leave every line as it was.  The
2-D nodes run at the shapes of their batch-grouping tests, which reach every MT instantiation of the two fp32-MFMA cores.

    python tools/conv_nodes_digest.py [--out FILE]
"""
import argparse
import hashlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import synth  # noqa: E402
from temporalstereo_amd import functional as TF, layers  # noqa: E402

DEV = torch.device("cuda:0")
LINES = []


def digest(v):
    if v is None:
        return "-"
    a = v.detach().contiguous().cpu().numpy()
    h = hashlib.sha256(("%s %s " % (a.dtype, a.shape)).encode())
    h.update(a.tobytes())
    return h.hexdigest()[:16]


def emit(name, items):
    LINES.append("%-44s %s" % (name, " ".join("%s=%s" % (k, digest(v)) for k, v in items)))
    print(LINES[-1], flush=True)


def gpu(a, grad=False):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV).requires_grad_(grad)


def bn_state(bn):
    return [("rmean", bn.running_mean), ("rvar", bn.running_var), ("count", bn.num_batches_tracked)]


def seeded_bn(bn, seed):
    c = bn.num_features
    with torch.no_grad():
        bn.weight.copy_(torch.from_numpy(synth.uniform(seed, "g", (c,), 0.5, 1.5)))
        bn.bias.copy_(torch.from_numpy(synth.normal(seed, "b", (c,), 0.2)))
        bn.running_mean.copy_(torch.from_numpy(synth.normal(seed, "rm", (c,), 0.2)))
        bn.running_var.copy_(torch.from_numpy(synth.uniform(seed, "rv", (c,), 0.5, 1.5)))
    return bn


def backward(y, seed):
    y.backward(gpu(synth.normal(seed, "gy", tuple(y.shape))))


# ------------------------------------------------------------------ the ten layers of test_fused_conv_batchnorm_activation_matches_framework
def fused_layer(case):
    rng = np.random.RandomState(40 + case)
    act = [None, "SiLU", "ReLU"][case % 3]
    B = int(rng.choice([1, 2, 3]))
    kind = ["hw", "hw_s2", "hw_d2", "d3", "d5", "d_s2", "hwT", "dT", "2d", "2d_s2"][case]
    cin, cout = int(rng.choice([3, 8, 16])), int(rng.choice([4, 8, 32]))
    D, H, W = int(rng.randint(2, 6)), int(rng.randint(5, 20)), int(rng.randint(6, 40))
    bias = bool(case % 2)
    if kind in ("2d", "2d_s2"):
        m = layers.Conv2d(cin, cout, 3, 2 if kind == "2d_s2" else 1, 1, bias=bias, norm=("BN", cout), activation=act)
        shape = (B, cin, H, W)
    elif kind == "hwT":
        m = layers.ConvTranspose3d(cin, cout, (1, 3, 3), (1, 2, 2), (0, 1, 1), (0, 1, 1), bias=bias, norm=("BN3d", cout), activation=act)
        shape = (B, cin, D, H, W)
    elif kind == "dT":
        m = layers.ConvTranspose3d(cin, cout, (3, 1, 1), (2, 1, 1), (1, 0, 0), (1, 0, 0), bias=bias, norm=("BN3d", cout), activation=act)
        shape = (B, cin, D, H, W)
    else:
        args = {"hw": ((1, 3, 3), (1, 1, 1), (0, 1, 1), (1, 1, 1)), "hw_s2": ((1, 3, 3), (1, 2, 2), (0, 1, 1), (1, 1, 1)),
                "hw_d2": ((1, 3, 3), (1, 1, 1), (0, 2, 2), (1, 2, 2)), "d3": ((3, 1, 1), (1, 1, 1), (1, 0, 0), (1, 1, 1)),
                "d5": ((5, 1, 1), (1, 1, 1), (2, 0, 0), (1, 1, 1)), "d_s2": ((3, 1, 1), (2, 1, 1), (1, 0, 0), (1, 1, 1))}[kind]
        m = layers.Conv3d(cin, cout, args[0], args[1], args[2], args[3], bias=bias, norm=("BN3d", cout), activation=act)
        shape = (B, cin, D, H, W)
    torch.manual_seed(100 + case)
    for p in (m.weight, m.bias):
        if p is not None:
            with torch.no_grad():
                p.normal_(0, 0.1)
    seeded_bn(m.norm, 60 + case)
    return kind, m.to(DEV), synth.normal(60 + case, "x", shape)


def fused_cases():
    for case in range(10):
        for mode in ("train", "eval", "folded"):
            kind, m, x = fused_layer(case)
            m.train(mode == "train")
            if mode == "folded":
                with TF.BNFolds(), torch.no_grad():
                    y = m(gpu(x))
                emit("fused/%d/%s/folded" % (case, kind), [("out", y)] + bn_state(m.norm))
                continue
            xa = gpu(x, True)
            y = m(xa)
            backward(y, 70 + case)
            emit("fused/%d/%s/%s" % (case, kind, mode), [("out", y), ("x", xa.grad), ("weight", m.weight.grad),
                                                        ("bias", m.bias.grad if m.bias is not None else None),
                                                        ("gamma", m.norm.weight.grad), ("beta", m.norm.bias.grad)] + bn_state(m.norm))


# ------------------------------------------------------------------ the raw functions
def raw(name, fn, x, w, cout):
    for with_bias in (False, True):
        xa, wa = gpu(x, True), gpu(w, True)
        b = gpu(synth.normal(9, "bias", (cout,), 0.3), True) if with_bias else None
        y = fn(xa, wa, b)
        backward(y, 77)
        emit("raw/%s/%s" % (name, "bias" if with_bias else "nobias"), [("out", y), ("x", xa.grad), ("weight", wa.grad),
                                                                         ("bias", b.grad if b is not None else None)])


def raw_cases():
    for cin, cout, stride, dil, (B, D, H, W) in [
            (24, 8, 1, 1, (2, 5, 21, 37)), (16, 32, 2, 1, (2, 3, 20, 36)), (16, 32, 2, 1, (1, 3, 17, 31)), (8, 16, 1, 2, (2, 4, 19, 33)),
            (40, 64, 1, 1, (1, 2, 9, 15)), (304, 8, 1, 1, (1, 5, 17, 40)), (64, 64, 2, 1, (1, 6, 17, 30))]:
        s, p, d = (1, stride, stride), (0, dil, dil), (1, dil, dil)
        raw("hw/%d-%d/s%d/d%d/%dx%dx%dx%d" % (cin, cout, stride, dil, B, D, H, W), lambda a, b, c: TF.conv3d(a, b, c, s, p, d),
            synth.normal(1, "x", (B, cin, D, H, W)), synth.normal(2, "w", (cout, cin, 1, 3, 3), 0.1), cout)
    for k, stride, dil, pad, din in [(3, 1, 1, 1, 7), (3, 2, 1, 1, 7), (3, 2, 1, 1, 12), (3, 1, 2, 2, 9), (5, 1, 1, 2, 14), (1, 1, 1, 0, 5)]:
        s, p, d = (stride, 1, 1), (pad, 0, 0), (dil, 1, 1)
        raw("d/k%d/s%d/d%d/p%d/D%d" % (k, stride, dil, pad, din), lambda a, b, c: TF.conv3d(a, b, c, s, p, d),
            synth.normal(3, "x", (2, 16, din, 11, 23)), synth.normal(4, "w", (32, 16, k, 1, 1), 0.2), 32)
    x = synth.normal(5, "x", (2, 32, 3, 9, 15))
    a = ((1, 2, 2), (0, 1, 1), (0, 1, 1))
    raw("hwT", lambda u, v, c: TF.conv_transpose3d(u, v, c, *a), x, synth.normal(6, "w", (32, 16, 1, 3, 3), 0.1), 16)
    a2 = ((2, 1, 1), (1, 0, 0), (1, 0, 0))
    raw("dT", lambda u, v, c: TF.conv_transpose3d(u, v, c, *a2), x, synth.normal(7, "w", (32, 16, 3, 1, 1), 0.1), 16)
    raw("dc", TF.conv_transpose2d_k4s2, synth.normal(11, "x", (2, 8, 5, 7)), synth.normal(12, "w", (8, 16, 4, 4), 0.1), 16)
    for shape in ((2, 8, 1, 5, 7), (1, 8, 3, 6, 9)):             # D = 1: no depth sum
        xa, wa = gpu(synth.normal(13, "x", shape), True), gpu(synth.normal(14, "w", (8, 8, 3, 3, 3), 0.1), True)
        y = TF.conv3d_k333(xa, wa)
        backward(y, 77)
        emit("raw/hw3/%dx%dx%dx%dx%d" % shape, [("out", y), ("x", xa.grad), ("weight", wa.grad)])


# ------------------------------------------------------------------ conv_bn_act, called directly
def node(name, x, w, cout, family, geom, bn_cls=torch.nn.BatchNorm3d, bias=True, act="SiLU", addend=None, few_values=False, modes=("train", "eval", "folded"),
         defer=False):
    for mode in modes:
        bn = seeded_bn(bn_cls(cout), 21).to(DEV).train(mode == "train")
        grad = mode != "folded"
        xa, wa = gpu(x, grad), gpu(w, grad)
        b = gpu(synth.normal(9, "bias", (cout,), 0.3), grad) if bias else None
        ad = gpu(addend, grad) if addend is not None else None
        kw = {}
        if ad is not None:
            kw["addend"] = ad
        if few_values:
            kw["few_values"] = True
        if mode == "folded":
            with TF.BNFolds(), torch.no_grad():
                y = TF.conv_bn_act(xa, wa, b, bn, act, family, geom, **kw)
            emit("node/%s/folded" % name, [("out", y)] + bn_state(bn))
            continue
        if defer:
            with TF.WgradDefer() as wd:
                y = TF.conv_bn_act(xa, wa, b, bn, act, family, geom, **kw)
                backward(y, 78)
                wd.flush()
        else:
            y = TF.conv_bn_act(xa, wa, b, bn, act, family, geom, **kw)
            backward(y, 78)
        emit("node/%s/%s" % (name, mode), [("out", y), ("x", xa.grad), ("weight", wa.grad), ("bias", b.grad if b is not None else None),
                                            ("gamma", bn.weight.grad), ("beta", bn.bias.grad),
                                            ("addend", ad.grad if ad is not None else None)] + bn_state(bn))


def node_cases():
    node("dc", synth.normal(11, "x", (2, 8, 5, 7)), synth.normal(12, "w", (8, 16, 4, 4), 0.1), 16, "dc", None, torch.nn.BatchNorm2d)
    for shape in ((2, 8, 1, 5, 7), (1, 8, 3, 6, 9)):
        node("hw3/%dx%dx%dx%dx%d" % shape, synth.normal(13, "x", shape), synth.normal(14, "w", (8, 8, 3, 3, 3), 0.1), 8, "hw3", (1, 1, False))
    # an addend, as first_layer_split passes it: one [B, Cout, 1, H, W] plane per item, added to every depth plane
    node("hw/addend", synth.normal(15, "x", (2, 12, 3, 9, 13)), synth.normal(16, "w", (16, 12, 1, 3, 3), 0.1), 16, "hw", (1, 1, False),
         addend=synth.normal(17, "a", (2, 16, 1, 9, 13)))
    # 32 input channels and a grid of 256 tiles: the bf16-split route of the stride-1 (1,3,3) layers
    node("hw/cin32", synth.normal(18, "x", (2, 32, 8, 64, 64)), synth.normal(19, "w", (16, 32, 1, 3, 3), 0.1), 16, "hw", (1, 1, False))
    # at most 4096 values per channel: the fp64 BatchNorm backward of SPP3D's coarse levels
    node("d/few_values", synth.normal(20, "x", (2, 8, 2, 3, 4)), synth.normal(22, "w", (8, 8, 1, 1, 1), 0.3), 8, "d", (1, 1, 0, False), bias=False,
         act="ReLU", few_values=True, modes=("train",))
    # the deferred weight-gradient finish of a training step
    node("hw/wgrad_defer", synth.normal(23, "x", (2, 16, 3, 12, 20)), synth.normal(24, "w", (16, 16, 1, 3, 3), 0.1), 16, "hw", (1, 1, False),
         modes=("train",), defer=True)
    node("d/wgrad_defer", synth.normal(23, "x", (2, 16, 3, 12, 20)), synth.normal(25, "w", (16, 16, 3, 1, 1), 0.1), 16, "d", (1, 1, 1, False),
         modes=("train",), defer=True)


# ------------------------------------------------------------------ decoder_conv
def decoder_cases():
    for with_up in (True, False):
        cin = 16 if with_up else 8
        for mode in ("train", "eval", "folded"):
            bn = seeded_bn(torch.nn.BatchNorm2d(16), 31).to(DEV).train(mode == "train")
            grad = mode != "folded"
            up = gpu(synth.normal(32, "up", (2, 8, 5, 7)), grad) if with_up else None
            skip = gpu(synth.normal(33, "skip", (2, 8, 9, 13)), grad)
            w = gpu(synth.normal(34, "w", (16, cin, 3, 3), 0.1), grad)
            name = "decoder/%s/%s" % ("up" if with_up else "plain", mode)
            if mode == "folded":
                with torch.no_grad():
                    y = TF.decoder_conv(up, skip, w, None, bn, "SiLU")
                emit(name, [("out", y)] + bn_state(bn))
                continue
            y = TF.decoder_conv(up, skip, w, None, bn, "SiLU")
            backward(y, 79)
            emit(name, [("out", y), ("up", up.grad if up is not None else None), ("skip", skip.grad), ("weight", w.grad),
                        ("gamma", bn.weight.grad), ("beta", bn.bias.grad)] + bn_state(bn))


# ------------------------------------------------------------------ the 2-D f32-MFMA nodes
def he(seed, name, shape, fan_in):
    return (synth.normal(seed, name, shape).astype(np.float64) * (2.0 / np.sqrt(fan_in))).astype(np.float32)


def fold(seed, n):
    return gpu(synth.uniform(seed, "scale", (n,), 0.5, 1.5)), gpu(synth.normal(seed, "shift", (n,), 0.1))


def gru_cases():
    def cell(seed, Ch, Cx, grad):
        C = Ch + Cx
        return [gpu(a, grad) for a in (he(seed, "wz", (Ch, C, 3, 3), 9 * C), synth.normal(seed, "bz", (Ch,), 0.1), he(seed, "wr", (Ch, C, 3, 3), 9 * C),
                                       synth.normal(seed, "br", (Ch,), 0.1), he(seed, "wq", (Ch, C, 3, 3), 9 * C), synth.normal(seed, "bq", (Ch,), 0.1))]
    # test_conv_gru_gpu.py::test_bits_do_not_depend_on_the_batch_grouping: gru_conv_kernel<8 | 4 | 2 | 1, true> and <4 | 2 | 1, false>
    B, Ch, Cx, H, W = 8, 64, 5, 31, 63
    h, x, params = gpu(synth.normal(41, "h", (B, Ch, H, W))), gpu(synth.normal(41, "x", (B, Cx, H, W))), cell(41, Ch, Cx, False)
    for n in (8, 4, 2, 1):
        with torch.no_grad():
            out = TF.conv_gru(h[:n], x[:n], *params, return_gates=True)
        emit("gru/64-5/31x63/B%d" % n, list(zip(("out", "z", "r", "q"), out)))
    for B, Ch, Cx, H, W in ((2, 12, 5, 9, 13), (1, 64, 64, 6, 7)):
        h, x, params = gpu(synth.normal(42, "h", (B, Ch, H, W)), True), gpu(synth.normal(42, "x", (B, Cx, H, W)), True), cell(42, Ch, Cx, True)
        out = TF.conv_gru(h, x, *params)
        backward(out, 80)
        emit("gru/%d-%d/%dx%d/grad" % (Ch, Cx, H, W), [("out", out), ("h", h.grad), ("x", x.grad)] +
             [(k, p.grad) for k, p in zip(("wz", "bz", "wr", "br", "wq", "bq"), params)])


def mbconv_cases():
    # test_mbconv_gpu.py::test_pointwise_bits_do_not_depend_on_the_batch_grouping, as a block: expand 130 -> 300 rows, project 300 -> 130
    # rows on a 24 x 24 plane; B = 32 | 20 | 12 | 8 | 4 reach expand_kernel and project_kernel <8 | 4 | 2 | 1>
    B, C, Cmid, Cr, H, W, mc = 32, 130, 300, 8, 24, 24, 33
    x, mem = gpu(synth.normal(43, "x", (B, C, H, W))), gpu(synth.normal(43, "m", (B, mc, H, W)))
    w = [gpu(a) for a in (he(43, "pw", (Cmid, C, 1, 1), C), he(43, "dw", (Cmid, 1, 3, 3), 9), he(43, "red", (Cr, Cmid, 1, 1), Cmid),
                          synth.normal(43, "bred", (Cr,), 0.1), he(43, "exp", (Cmid, Cr, 1, 1), Cr), synth.normal(43, "bexp", (Cmid,), 0.1),
                          he(43, "pwl", (C, Cmid, 1, 1), Cmid))]
    f1, f2, f3 = fold(44, Cmid), fold(45, Cmid), fold(46, C)
    for n, memory in ((32, True), (20, True), (12, True), (8, True), (4, True), (4, False), (1, False)):
        with torch.no_grad():
            y, e, d, gate = TF.mbconv_eval(x[:n], mem[:n] if memory else None, w[0], f1, w[1], f2, w[2], w[3], w[4], w[5], w[6], f3, return_stages=True)
        emit("mbconv/130-300/24x24/B%d/%s" % (n, "memory" if memory else "first"), [("out", y), ("act1", e), ("act2", d), ("gate", gate)])


def depthwise_cases():
    for shape in ((2, 12, 9, 13), (2, 8, 8, 16), (1, 5, 17, 70)):          # scalar staging; 16-byte staging; more than one tile along both axes
        for with_bias in (False, True):
            x, w = gpu(synth.normal(47, "x", shape), True), gpu(he(47, "w", (shape[1], 1, 3, 3), 9), True)
            b = gpu(synth.normal(47, "b", (shape[1],), 0.3), True) if with_bias else None
            y = TF.depthwise_conv3x3(x, w, b)
            backward(y, 81)
            emit("depthwise/%dx%dx%dx%d/%s" % (shape + ("bias" if with_bias else "nobias",)),
                 [("out", y), ("x", x.grad), ("weight", w.grad), ("bias", b.grad if b is not None else None)])


def conv3x3_cases():
    # test_decoder_gpu.py::test_bits_do_not_depend_on_the_batch_grouping's plane: 128 rows on 31 x 63, B = 16 | 8 | 4 | 2 reach
    # conv3x3_kernel<8 | 4 | 2 | 1, S>; stride 2 from an odd 61 x 125 plane
    Cout = 128
    sc = fold(48, Cout)
    for stride, Cin, H, W in ((1, 24, 31, 63), (2, 6, 61, 125)):
        x, w = gpu(synth.normal(49, "x", (16, Cin, H, W))), gpu(he(49, "w", (Cout, Cin, 3, 3), 9 * Cin))
        res = gpu(synth.normal(49, "r", (16, Cout, 31, 63)))
        for n in (16, 8, 4, 2):
            for residual in ((False, True) if stride == 1 else (False,)):
                with torch.no_grad():
                    y = TF.conv3x3_bn_act(x[:n], w, sc, stride, "SiLU", residual=res[:n] if residual else None)
                emit("conv3x3/s%d/%d-%d/%dx%d/B%d/%s" % (stride, Cin, Cout, H, W, n, "residual" if residual else "plain"), [("out", y)])
    for stride in (1, 2):                   # a small odd plane, no fold, no activation, 130 rows (a ragged second row group)
        x, w = gpu(synth.normal(50, "x", (2, 5, 9, 13))), gpu(he(50, "w", (130, 5, 3, 3), 45))
        with torch.no_grad():
            y = TF.conv3x3_bn_act(x, w, None, stride, None)
        emit("conv3x3/s%d/5-130/9x13/B2/raw" % stride, [("out", y)])


def fused_mbconv_cases():
    # the pointwise grouping again: 130 rows on 24 x 24, B = 32 | 20 | 12 | 4 reach fused_project_kernel<8 | 4 | 2 | 1>
    B, Cin, Cmid, Cout, H, W = 32, 24, 96, 130, 24, 24
    x, res = gpu(synth.normal(51, "x", (B, Cin, H, W))), gpu(synth.normal(51, "r", (B, Cout, H, W)))
    w_exp, w_pwl = gpu(he(51, "exp", (Cmid, Cin, 3, 3), 9 * Cin)), gpu(he(51, "pwl", (Cout, Cmid, 1, 1), Cmid))
    f1, f2 = fold(52, Cmid), fold(53, Cout)
    for n in (32, 20, 12, 4):
        with torch.no_grad():
            y, mid = TF.fused_mbconv_eval(x[:n], w_exp, f1, 1, w_pwl, f2, res[:n], return_stages=True)
        emit("fused_mbconv/s1/24-96-130/24x24/B%d" % n, [("out", y), ("mid", mid)])
    xs = gpu(synth.normal(54, "x", (2, Cin, 9, 13)))
    w_same = gpu(he(54, "pwl", (Cin, Cmid, 1, 1), Cmid))
    with torch.no_grad():
        y, mid = TF.fused_mbconv_eval(xs, w_exp, f1, 2, w_pwl, f2, None, return_stages=True)
        emit("fused_mbconv/s2/24-96-130/9x13/B2", [("out", y), ("mid", mid)])
        y, mid = TF.fused_mbconv_eval(xs, w_exp, f1, 1, w_same, fold(55, Cin), xs, return_stages=True)      # the block's own input as the residual
        emit("fused_mbconv/s1/24-96-24/9x13/B2/skip", [("out", y), ("mid", mid)])


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--out", help="also write the lines to this file")
    args = ap.parse_args()
    fused_cases(); raw_cases(); node_cases(); decoder_cases()
    gru_cases(); mbconv_cases(); depthwise_cases(); conv3x3_cases(); fused_mbconv_cases()
    torch.cuda.synchronize()
    if args.out:
        with open(args.out, "w") as fh:
            fh.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
