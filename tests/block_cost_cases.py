"""Test infrastructure: the cases of tests/test_block_cost_forms_gpu.py -- shapes, contents, references, yardsticks -- and a restatement
of the launch rules of csrc/block_cost.hip (launch_fwd / launch_bwd), shared with tests/test_block_cost_ref_cpu.py.  No GPU in here.

Launch forms.  `fwd_form` / `bwd_form` restate which kernel a call reaches; the table below is `form_table()` and the CPU test pins
the text to the functions, so that it changes when they do.  `vec` needs W % 4 == 0 and every base pointer on 16 bytes; a ragged width,
or an aligned width with the pointers one element off, is `scalar`.  Lane counts are left out of the table: they move every few
widths and the sweep over 4..136 walks all of 64..512 (the CPU test checks that).  `main<..>xN` is block_cost_main in N passes of
items.  TRANSITIONS are the aligned widths above 136 at or just below which a kernel family changes (any entry, any D of the table,
aligned or one element off); `derive_transitions()` finds them and the CPU test pins the list.

FORM TABLE BEGIN
forward  int|sampled|warped D=2  vec   : 4..32 fast<vec,2>  36..48 fast<vec,3>  52..64 fast<vec,4>  68..252 fast<vec,8>  256.. main<vec>
forward  int|sampled|warped D=2  scalar: 4..32 fast<scalar,2>  33..64 fast<scalar,4>  65..252 fast<scalar,8>  253.. main<scalar>
forward  int|sampled|warped D=3  vec   : 4..32 fast<vec,2>  36..48 fast<vec,3>  52..64 fast<vec,4>  68..84 fast<vec,8>  88..96 fast<vec,3>  100..128 fast<vec,4>  132..168 fast<vec,8>  172..192 fast<vec,4>  196..252 fast<vec,8>  256..668 main<vec>  672.. main<vec>x2
forward  int|sampled|warped D=3  scalar: 4..32 fast<scalar,2>  33..64 fast<scalar,4>  65..84 fast<scalar,8>  85..128 fast<scalar,4>  129..168 fast<scalar,8>  169..192 fast<scalar,4>  193..252 fast<scalar,8>  253..668 main<scalar>  669.. main<scalar>x2
forward  int|sampled|warped D=5  vec   : 4..32 fast<vec,2>  36..48 fast<vec,3>  52..64 fast<vec,2>  68..96 fast<vec,3>  100 fast<vec,4>  104..144 fast<vec,3>  148..152 fast<vec,4>  156..192 fast<vec,3>  196..204 fast<vec,4>  208..240 fast<vec,3>  244..252 fast<vec,4>  256 main<vec>  260..288 fast<vec,3>  292..304 main<vec>  308..336 fast<vec,3>  340..408 main<vec>  412.. main<vec>x2
forward  int|sampled|warped D=5  scalar: 4..32 fast<scalar,2>  33..48 fast<scalar,4>  49..64 fast<scalar,2>  65..252 fast<scalar,4>  253..408 main<scalar>  409.. main<scalar>x2
forward  int|sampled|warped D=16 vec   : 4..128 fast<vec,2>  132..256 main<vec>x2  260..384 main<vec>x3  388..512 main<vec>x4  516..640 main<vec>x5  644..768 main<vec>x6  772.. main<vec>x7
forward  int|sampled|warped D=16 scalar: 4..128 fast<scalar,2>  129..256 main<scalar>x2  257..384 main<scalar>x3  385..512 main<scalar>x4  513..640 main<scalar>x5  641..768 main<scalar>x6  769.. main<scalar>x7
forward  int|sampled|warped D=17 vec   : 4..108 fast<vec,2>  112..220 main<vec>x2  224..360 main<vec>x3  364..444 main<vec>x4  448..600 main<vec>x5  604..668 main<vec>x6  672.. main<vec>x7
forward  int|sampled|warped D=17 scalar: 4..108 fast<scalar,2>  109..220 main<scalar>x2  221..360 main<scalar>x3  361..444 main<scalar>x4  445..600 main<scalar>x5  601..668 main<scalar>x6  669.. main<scalar>x7
forward  corr               D=2  vec   : 4..32 corr_rows<1,256>  36..256 corr_rows<2,256>  260..504 corr_rows<2,512>  508.. main<vec>
forward  corr               D=2  scalar: 4..32 fast<scalar,2>  33..64 fast<scalar,4>  65..252 fast<scalar,8>  253.. main<scalar>
forward  corr               D=3  vec   : 4..32 corr_rows<1,256>  36..256 corr_rows<2,256>  260..504 corr_rows<2,512>  508..668 main<vec>  672.. main<vec>x2
forward  corr               D=3  scalar: 4..32 fast<scalar,2>  33..64 fast<scalar,4>  65..84 fast<scalar,8>  85..128 fast<scalar,4>  129..168 fast<scalar,8>  169..192 fast<scalar,4>  193..252 fast<scalar,8>  253..668 main<scalar>  669.. main<scalar>x2
forward  corr               D=5  vec   : 4..32 corr_rows<1,256>  36..256 corr_rows<2,256>  260..504 corr_rows<2,512>  508.. main<vec>x2
forward  corr               D=5  scalar: 4..32 fast<scalar,2>  33..48 fast<scalar,4>  49..64 fast<scalar,2>  65..252 fast<scalar,4>  253..408 main<scalar>  409.. main<scalar>x2
forward  corr               D=16 vec   : 4..32 corr_rows<1,256>  36..256 corr_rows<2,256>  260..504 corr_rows<2,512>  508..512 main<vec>x4  516..640 main<vec>x5  644..768 main<vec>x6  772.. main<vec>x7
forward  corr               D=16 scalar: 4..128 fast<scalar,2>  129..256 main<scalar>x2  257..384 main<scalar>x3  385..512 main<scalar>x4  513..640 main<scalar>x5  641..768 main<scalar>x6  769.. main<scalar>x7
forward  corr               D=17 vec   : 4..32 corr_rows<1,256>  36..256 corr_rows<2,256>  260..504 corr_rows<2,512>  508..600 main<vec>x5  604..668 main<vec>x6  672.. main<vec>x7
forward  corr               D=17 scalar: 4..108 fast<scalar,2>  109..220 main<scalar>x2  221..360 main<scalar>x3  361..444 main<scalar>x4  445..600 main<scalar>x5  601..668 main<scalar>x6  669.. main<scalar>x7
backward int                D=3  vec   : 4..368 bwd_tile<vec>  372..504 bwd_main<vec,staged>  508.. bwd_main<vec,unstaged>
backward int                D=3  scalar: 4..368 bwd_tile<scalar>  369..504 bwd_main<scalar,staged>  505.. bwd_main<scalar,unstaged>
backward int                D=16 vec   : 4..128 bwd_tile<vec>  132..504 bwd_main<vec,staged>  508.. bwd_main<vec,unstaged>
backward int                D=16 scalar: 4..128 bwd_tile<scalar>  129..504 bwd_main<scalar,staged>  505.. bwd_main<scalar,unstaged>
backward int                D=17 vec   : 4..504 bwd_main<vec,staged>  508.. bwd_main<vec,unstaged>
backward int                D=17 scalar: 4..504 bwd_main<scalar,staged>  505.. bwd_main<scalar,unstaged>
backward sampled|warped     D=3  vec   : 4..252 bwd_rows<256>  256 bwd_rows<256> lds>64K  260..316 bwd_rows<512> lds>64K  320..368 bwd_tile<vec>  372..504 bwd_main<vec,staged>  508.. bwd_main<vec,unstaged>
backward sampled|warped     D=3  scalar: 4..368 bwd_tile<scalar>  369..504 bwd_main<scalar,staged>  505.. bwd_main<scalar,unstaged>
backward sampled|warped     D=16 vec   : 4..252 bwd_rows<256>  256 bwd_rows<256> lds>64K  260..316 bwd_rows<512> lds>64K  320..504 bwd_main<vec,staged>  508.. bwd_main<vec,unstaged>
backward sampled|warped     D=16 scalar: 4..128 bwd_tile<scalar>  129..504 bwd_main<scalar,staged>  505.. bwd_main<scalar,unstaged>
backward sampled|warped     D=17 vec   : 4..252 bwd_rows<256>  256 bwd_rows<256> lds>64K  260..316 bwd_rows<512> lds>64K  320..504 bwd_main<vec,staged>  508.. bwd_main<vec,unstaged>
backward sampled|warped     D=17 scalar: 4..504 bwd_main<scalar,staged>  505.. bwd_main<scalar,unstaged>
FORM TABLE END

Shapes.  C = 8 (one group), B = 1, scales = 3, H alternating 5 | 9 (a partial last row block; H / 4 = 1 | 2), with C = 16, B = 2 and
scales 1 | 2 at the widths `vary` picks by W % 12 and W % 24.  Every width 4..136 (D = 2, 5, 16 forward; 3, 16, 17 backward: 17 leaves
the tile form); {T-4, T-3, T-1, T, T+1, T+4} around every transition and every pass step (D = 3, 17; forward also 5, the non-monotonic
corner); all aligned widths of both once more with every base one element off 16 bytes; one int and one sampled backward with
B C/8 D > 65535 planes at H, W <= 6 (the generic adjoint; the expansion's folded plane grid); NULLS, one backward case per form for
the gradient pointers NULL in turn; GRADS_OFF, aligned inputs with the gradient buffers one element off; SPLIT_W x SPLIT_STRIDES for
the split-input entry.

Contents.  N(0,1) features; candidates uniform over [-3, W + 3], plane 0 rounded to integers and plane D - 1 exactly 0 (D = 2: the
even rows of plane 0 and the odd rows of plane 1); `far` cases with the six candidate planes +-(W + 2), +-1e6, +-3e9.

Metric and bound.  `err_planes` / `err_tensor` of tests/pyramid_cases.py (an all-zero reference plane demands exact zeros);
bound = max(base, 4 x yardstick), base 5e-6 for outputs and 2e-5 for gradients (bn_cases.BASE), the yardstick being
tests/block_cost_ref.py on fp32 inputs in fp32 arithmetic against its float64 run -- for the mixed reference on the shared fp32
position, for the exact one with the fp32 position against the float64 position.  It is computed from the reference alone.
"""
import collections
import functools
import re

import numpy as np
import torch

import block_cost_ref as ref
import synth
from bn_cases import BASE
from pyramid_cases import err_planes, err_tensor      # noqa: F401

TS_OK, TS_ERR_NULL, TS_ERR_SHAPE, TS_ERR_UNSUPPORTED = 0, -1, -2, -3
FWD_ENTRIES = ("int", "sampled", "warped", "corr")
BWD_ENTRIES = ("int", "sampled", "warped")


# ---- the launch rules of csrc/block_cost.hip, restated ---------------------------------------------------------------------------
def _cdiv(a, b):
    return (a + b - 1) // b


def _geom(W):
    nbx = (W + 3) // 4
    wq, wqp, nbxp = nbx, (nbx + 1) | 1, nbx
    for q in (8, 16, 32, 64, 128, 192, 256, 320, 384, 448, 512):
        if q >= nbx:
            if (q - nbx) * 8 <= q:
                nbxp = q
            break
    return nbx, wq, wqp, nbxp


def fwd_form(entry, W, D, aligned=True, lanes=False):
    """launch_fwd: the kernel an entry reaches (the expansion of the pooled maps follows whenever scales > 1)"""
    nbx, wq, wqp, nbxp = _geom(W)
    vec = W % 4 == 0 and aligned
    nitems = nbxp * D
    passes = _cdiv(nitems, 512)
    threads = min(512, _cdiv(_cdiv(nitems, passes), 64) * 64)
    np_ = _cdiv(8 * 2 * wq, threads)
    inst = 2 if np_ <= 2 else (3 if vec and np_ == 3 else (4 if np_ <= 4 else 8))
    lds = 8 * (4 * 4 * wqp + (2 if inst <= 3 else 4) * 4 * wq) * 4
    if entry == "corr" and vec:
        cthreads = _cdiv(4 * nbx, 64) * 64
        nrp = _cdiv(2 * 4 * wq, cthreads)
        if cthreads <= 512 and nrp <= 2 and 2 * 4 * 4 * wqp * 16 <= 64 * 1024:
            return "corr_rows<%d,%d>" % (nrp, 256 if cthreads <= 256 else 512) + ("@%d" % cthreads if lanes else "")
    kind = "vec" if vec else "scalar"
    if lds <= 64 * 1024 and passes == 1 and np_ <= 8:
        return "fast<%s,%d>" % (kind, inst) + ("@%d" % threads if lanes else "")
    return "main<%s>%s" % (kind, "x%d" % passes if passes > 1 else "") + ("@%d" % threads if lanes else "")


def bwd_form(entry, W, D, aligned=True, lanes=False, grads_aligned=True):
    """launch_bwd: the kernel behind the adjoint of the pooled maps.  `aligned`: left, right, candidates, grad_out on 16 bytes;
    `grads_aligned`: grad_left and grad_right too -- the row and tile kernels store them 16 bytes at a time, block_cost_bwd_main
    adds element by element"""
    nbx, wq, wqp, _ = _geom(W)
    vec = W % 4 == 0 and aligned
    grads16 = aligned and grads_aligned
    tile_lds = (8 * 4 * 4 * wqp + 3 * 4 * 4 * wq + 4) * 4
    tile_threads = _cdiv(nbx, 64 // D) * 64 if D <= 16 else 1 << 30
    rthreads = _cdiv(4 * nbx, 64) * 64
    rlds = (8 * 4 * 4 * wqp + 8 * 4 * 4 * wq) * 4
    if entry != "int" and vec and grads16 and rthreads <= 512 and rlds <= 80 * 1024:
        return "bwd_rows<%d>%s" % (256 if rthreads <= 256 else 512, " lds>64K" if rlds > 64 * 1024 else "") + ("@%d" % rthreads if lanes else "")
    if tile_lds <= 64 * 1024 and tile_threads <= 512:
        return "bwd_tile<%s>" % ("vec" if vec and grads16 else "scalar") + ("@%d" % tile_threads if lanes else "")
    passes = _cdiv(nbx * D, 256)
    threads = min(256, _cdiv(_cdiv(nbx * D, passes), 64) * 64)
    kind = "vec" if vec else "scalar"
    return "bwd_main<%s,%s>" % (kind, "staged" if 8 * 4 * 4 * wqp * 4 <= 64 * 1024 else "unstaged") + ("@%d" % threads if lanes else "")


def adjoint_form(B, C, H, W, D, scales):
    if scales < 2:
        return "none"
    alds = (2 * 2 * (W // 2) + 2 * (W // 4)) * 8
    return "adjoint_rows" if B * (C // 8) * D <= 65535 and alds <= 64 * 1024 else "adjoint_generic"


TABLE_D = {"forward": (2, 3, 5, 16, 17), "backward": (3, 16, 17)}
TABLE_MAX_W = 800


def _runs(widths, form):
    """[(first, last, form)] of consecutive widths with one form"""
    out = []
    for w in widths:
        f = form(w)
        if out and out[-1][2] == f:
            out[-1][1] = w
        else:
            out.append([w, w, f])
    return out


def form_table():
    lines = []
    for side, entries, fn in (("forward", (("int|sampled|warped", "sampled"), ("corr", "corr")), fwd_form),
                              ("backward", (("int", "int"), ("sampled|warped", "sampled")), bwd_form)):
        for label, entry in entries:
            for D in TABLE_D[side]:
                for kind, widths, al in (("vec", range(4, TABLE_MAX_W + 1, 4), True), ("scalar", range(4, TABLE_MAX_W + 1), False)):
                    runs = _runs(widths, lambda w: fn(entry, w, D, al))
                    text = "  ".join("%s %s" % ("%d..%s" % (a, b if b < widths[-1] else "") if a != b else str(a), f) for a, b, f in runs)
                    lines.append("%-8s %-18s D=%-2d %-6s: %s" % (side, label, D, kind, text))
    return "\n".join(lines)


def _family(form):
    """a form without what the sweep over 4..136 already walks: block_cost_fast's NP, and how many passes `several` is"""
    form = re.sub(r"fast<(\w+),\d>", r"fast<\1>", form)
    return re.sub(r"x\d+$", "x", form)


def derive_transitions(lo=137, hi=TABLE_MAX_W):
    """aligned widths T > 136 at which some kernel family differs from the one 4 columns before (vec), or changes at a width in
    (T-4, T] (scalar) -- any entry, any D of the table"""
    found = set()
    for side, fn, entries in (("forward", fwd_form, FWD_ENTRIES), ("backward", bwd_form, BWD_ENTRIES)):
        for D in TABLE_D[side]:
            for e in entries:
                for w in range(lo, hi + 1):
                    if _family(fn(e, w, D, False)) != _family(fn(e, w - 1, D, False)):
                        found.add(_cdiv(w, 4) * 4)
                    if w % 4 == 0 and _family(fn(e, w, D, True)) != _family(fn(e, w - 4, D, True)):
                        found.add(w)
    return sorted(found)


# what derive_transitions() gives: fast | main at D = 2, 3 (256) and through the non-monotonic corner of D = 5 (256, 260, 292, 308, 340),
# one | several passes (412 at D = 5, 672 at D = 3), corr_rows 256 | 512 | main (260, 508), bwd_rows at more than 64 KB of LDS (256, 260),
# bwd_rows | bwd_tile or bwd_main (320), bwd_tile | bwd_main (372), staged | unstaged (508)
TRANSITIONS = (256, 260, 292, 308, 320, 340, 372, 412, 508, 672)
PASS_STEPS = (516, 604)          # one more pass of block_cost_main at D = 16 and D = 17: no other family, run all the same
FWD_TRANSITION_D = (3, 5, 17)    # 5: the non-monotonic corner
BWD_TRANSITION_D = (3, 17)


# ---- cases -----------------------------------------------------------------------------------------------------------------------
Case = collections.namedtuple("Case", "name side B C H W D scales aligned content")


def vary(W, D):
    """-> B, C, H, scales: C = 8, B = 1, scales = 3 but for the widths picked here; aligned and ragged widths get every variation"""
    m, H = W % 12, 9 if (W + W // 4 + D) % 2 else 5
    return (2 if m in (4, 5) else 1), (16 if m in (0, 1) else 8), H, ((1 if W % 24 < 12 else 2) if m in (8, 9) else 3)


def _case(side, W, D, aligned=True, content="std", **over):
    B, C, H, scales = vary(W, D)
    d = dict(B=B, C=C, H=H, scales=scales)
    d.update(over)
    name = "%s_w%d_d%d_h%d_c%d_b%d_s%d_%s%s" % (side, W, D, d["H"], d["C"], d["B"], d["scales"], "al" if aligned else "off1", "" if content == "std" else "_" + content)
    return Case(name, side, d["B"], d["C"], d["H"], W, D, d["scales"], aligned, content)


def _around(ts):
    return sorted({w for t in ts for w in (t - 4, t - 3, t - 1, t, t + 1, t + 4)})


def _cases(side, sweep_d, transition_d):
    grid = [(w, d) for w in range(4, 137) for d in sweep_d] + [(w, d) for w in _around(TRANSITIONS + PASS_STEPS) for d in transition_d]
    cs = [_case(side, w, d) for w, d in grid]
    cs += [_case(side, w, d, aligned=False) for w, d in grid if w % 4 == 0]
    cs += [_case(side, w, 6, aligned=a, content="far") for w, a in ((7, True), (40, True), (40, False), (256, True))]
    return cs


FWD = _cases("fwd", (2, 5, 16), FWD_TRANSITION_D)
BWD = _cases("bwd", (3, 16, 17), BWD_TRANSITION_D)
# more planes of the pooled maps than one grid dimension holds: the adjoint's generic form, the expansion's folded plane grid
MANY_PLANES = [_case("bwd", 6, 4097, B=2, C=64, H=4, scales=3), _case("bwd", 5, 8193, B=1, C=64, H=5, scales=3)]
# each gradient pointer NULL in turn: one case per backward form
NULLS = [c for c in BWD if (c.W, c.D) in ((9, 3), (40, 16), (40, 17), (256, 3), (320, 3), (320, 17), (673, 3), (676, 17)) and c.content == "std" and c.aligned]
# inputs on 16 bytes, grad_left / grad_right / grad_disp one element off: no 16-byte store may go to them (tile scalar; main as it is)
GRADS_OFF = [c for c in BWD if (c.W, c.D) in ((40, 3), (40, 16), (128, 16), (132, 17), (256, 3), (320, 3), (372, 3)) and c.content == "std" and c.aligned]
SPLIT_W = (8, 38, 64, 260, 512, 600)        # corr_rows<.,256>, fast<scalar>, corr_rows, corr_rows<.,512>, corr_rows<.,512>, main
SPLIT_STRIDES = ((0, 0, 0, 0), (4, 8, 12, 16), (64, 0, 4, 32), (8, 100, 36, 4))     # extra elements per batch item: left, left2, right, right2


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def candidates(seed, B, D, H, W, content="std"):
    if content == "far":
        assert D == 6
        v = torch.tensor([W + 2.0, -(W + 2.0), 1e6, -1e6, 3e9, -3e9], dtype=torch.float32)
        return v.view(1, D, 1, 1).expand(B, D, H, W).contiguous()
    d = _t(synth.uniform(seed, "d", (B, D, H, W), -3.0, W + 3.0))
    if D >= 3:
        d[:, 0] = torch.round(d[:, 0])
        d[:, D - 1] = 0.0
    else:
        d[:, 0, 0::2] = torch.round(d[:, 0, 0::2])
        d[:, 1, 1::2] = 0.0
    return d


@functools.lru_cache(maxsize=2)
def inputs(case):
    """fp32: left, right, candidates, and for a backward case grad_out of the int and of the full sampled volume (shared: read only)"""
    B, C, H, W, D, s = case.B, case.C, case.H, case.W, case.D, case.scales
    seed = 4100 + 31 * W + D
    L, R = _t(synth.normal(seed, "L", (B, C, H, W))), _t(synth.normal(seed, "R", (B, C, H, W)))
    d = candidates(seed, B, D, H, W, case.content)
    if case.side == "fwd":
        return L, R, d, None, None
    G = C // 8
    return L, R, d, _t(synth.normal(seed, "gi", (B, C + s * G, D, H, W))), _t(synth.normal(seed, "gs", (B, 2 * C + s * G, D, H, W)))


def entry_slice(entry, C):
    """channels of the full sampled volume an entry writes"""
    return slice({"sampled": 0, "warped": C, "corr": 2 * C}[entry], None)


@functools.lru_cache(maxsize=2)
def fwd_reference(case):
    """-> {"int": (f64, fp32), "mixed": f64, "exact": f64, "fp32": fp32} of the int and the full sampled volume"""
    L, R, d, _, _ = inputs(case)
    with torch.no_grad():
        return {"int": (ref.block_cost(L.double(), R.double(), case.D, case.scales), ref.block_cost(L, R, case.D, case.scales)),
                "mixed": ref.block_cost(L.double(), R.double(), d.double(), case.scales, pos_dtype=torch.float32),
                "exact": ref.block_cost(L.double(), R.double(), d.double(), case.scales),
                "fp32": ref.block_cost(L, R, d, case.scales)}


def _grads(dt, case, entry, pos_dtype=None):
    L, R, d, gi, gs = inputs(case)
    L, R = L.to(dt).requires_grad_(), R.to(dt).requires_grad_()
    if entry == "int":
        return torch.autograd.grad(ref.block_cost(L, R, case.D, case.scales), (L, R), gi.to(dt))
    d = d.to(dt).requires_grad_()
    out = ref.block_cost(L, R, d, case.scales, pos_dtype=pos_dtype)
    gs = gs.to(dt)
    full = torch.autograd.grad(out, (L, R, d), gs)
    # the warped entry's grad_out is the volume without its reference half, a broadcast of `left` over D whose adjoint is the sum over D
    return full, (full[0] - gs[:, :case.C].sum(2), full[1], full[2])


@functools.lru_cache(maxsize=2)
def bwd_reference(case):
    """-> {entry: ((grad_left, grad_right[, grad_disp]) in f64 -- sampled entries on the fp32 position --, the same in fp32)}"""
    s64, w64 = _grads(torch.float64, case, "sampled", torch.float32)
    s32, w32 = _grads(torch.float32, case, "sampled")
    return {"int": (_grads(torch.float64, case, "int"), _grads(torch.float32, case, "int")), "sampled": (s64, s32), "warped": (w64, w32)}


def bound(base, yardstick):
    return max(base, 4.0 * yardstick)


if __name__ == "__main__":
    print(form_table())
    print("transitions", derive_transitions())
    print(len(FWD), "forward cases,", len(BWD), "backward cases")
