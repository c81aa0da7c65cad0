"""GPU: every launch form of csrc/block_cost.hip (K1) called through the C ABI against the float64 restatement tests/block_cost_ref.py,
at the shapes of tests/block_cost_cases.py (the table of forms, the shapes, the contents and the bound are in its docstring).

Every tensor is carved out of a sentinel-filled buffer with guard bands (tests/sentinel.py) -- the workspace of the pooled maps too, at
exactly ts_block_cost_workspace_bytes / ts_block_cost_bwd_workspace_bytes -- so every case asserts, besides the status code, that
nothing but the outputs and the workspace changed; that every output is finite; and, for the forward entries (no atomics), identical
bits on a second call.  The backward accumulates with atomics: no second call.

Comparisons: (a) outputs and gradients against the MIXED reference (the kernel's fp32 position, float64 after it), (b) forward outputs
also against the EXACT one (float64 throughout); what is a move -- the reference half of the full sampled entry, the zeros of the far
candidates -- bit for bit.  Bound: max(base, 4 x yardstick), the yardstick being the restatement in fp32 against the same float64
reference, computed here from the reference alone.

`-s` prints one line per case and entry: the launch form with its lane count, then per quantity error/yardstick/bound; with
TS_K1_PARITY_FILE set the same lines are appended to that file (profiles/block_cost_parity.txt).
"""
import os

import pytest
import torch

import block_cost_cases as K
import block_cost_ref as R
from sentinel import SENTINEL, Arena

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
_ids = lambda c: c.name


def _api():
    from temporalstereo_amd import _lib
    return _lib.lib(), _lib.current_stream_handle()


def _ptr(t):
    return None if t is None else t.data_ptr()


def _carve(shape, off=0, fill=None, out=False):
    """a tensor in an arena of its own, `off` elements past a 16-byte boundary -> (arena, view)"""
    n = 1
    for s in shape:
        n *= s
    a = Arena(n + off, DEV)
    return a, a.carve(tuple(shape), offset=off, fill=fill, out=out)


def _workspace(L, dims, bwd=False):
    """the pooled maps at exactly the size the library asks for: an overrun lands in the guard band"""
    nbytes = (L.ts_block_cost_bwd_workspace_bytes if bwd else L.ts_block_cost_workspace_bytes)(*dims)
    assert nbytes > 0 and nbytes % 4 == 0
    a = Arena(nbytes // 4, DEV)
    return a, a.carve((nbytes // 4,), out=True)


class _Report:
    """One line per case and entry -- `case entry form: quantity error/yardstick/bound ...`, `=bits` for what is compared bit for bit --
    printed (and appended to TS_K1_PARITY_FILE) before anything is asserted, so that a failing case still shows every figure."""

    def __init__(self, case, tag):
        self.head, self.items, self.bad = "%s %s:" % (case, tag), [], []

    def within(self, quantity, err, yard, base):
        bound = K.bound(base, yard)
        self.items.append("%s %.2g/%.2g/%.2g" % (quantity, err, yard, bound))
        if not err <= bound:
            self.bad.append(self.items[-1])

    def exact(self, quantity, got, ref):
        same = _same_bits(got, ref)
        self.items.append("%s %s" % (quantity, "=bits" if same else "DIFFERENT-bits"))
        if not same:
            self.bad.append(self.items[-1])

    def close(self):
        line = self.head + " " + "  ".join(self.items)
        print(line)
        if os.environ.get("TS_K1_PARITY_FILE"):
            with open(os.environ["TS_K1_PARITY_FILE"], "a") as f:
                f.write(line + "\n")
        assert not self.bad, self.head + " " + "  ".join(self.bad)


def _same_bits(got, ref):
    """fp32 tensors equal bit for bit (0.0 and -0.0 differ); ref may be float64 holding fp32 values"""
    return torch.equal(got.detach().cpu().contiguous().view(torch.int32), ref.float().contiguous().view(torch.int32))


def _run(arenas, call, want_rc=K.TS_OK, twice=True):
    """seal -> call -> nothing but the outputs changed; a second call on the restored buffers gives the same bits"""
    for a in arenas:
        a.seal()
    rc = call()
    torch.cuda.synchronize()
    assert rc == want_rc, "status %d, expected %d" % (rc, want_rc)
    assert all(a.intact() for a in arenas), "written outside the outputs and the workspace"
    if twice and want_rc == K.TS_OK:
        first = [a.buf.clone() for a in arenas]
        for a in arenas:
            a.restore()
        assert call() == K.TS_OK
        torch.cuda.synchronize()
        assert all(torch.equal(a.buf.view(torch.int32), f.view(torch.int32)) for a, f in zip(arenas, first)), "a second call gives other bits"


def _finite(*ts):
    assert all(bool(torch.isfinite(t).all()) for t in ts), "non-finite output"


def _dims(c):
    return c.B, c.C, c.H, c.W, c.D, c.scales


def _out_channels(entry, C, scales):
    return {"int": C, "sampled": 2 * C, "warped": C, "corr": 0}[entry] + scales * (C // 8)


def _fwd_call(L, stream, entry, c, vL, vR, vd, vo, vws):
    fn = {"int": L.ts_block_cost_int_fwd, "sampled": L.ts_block_cost_sampled_fwd, "warped": L.ts_block_cost_sampled_warped_fwd,
          "corr": L.ts_block_cost_sampled_corr_fwd}[entry]
    if entry == "int":
        return lambda: fn(_ptr(vL), _ptr(vR), _ptr(vo), _ptr(vws), *_dims(c), stream)
    return lambda: fn(_ptr(vL), _ptr(vR), _ptr(vd), _ptr(vo), _ptr(vws), *_dims(c), stream)


def _bwd_call(L, stream, entry, c, vL, vR, vd, vg, gL, gR, gD, vws):
    if entry == "int":
        return lambda: L.ts_block_cost_int_bwd(_ptr(vL), _ptr(vR), _ptr(vg), _ptr(gL), _ptr(gR), _ptr(vws), *_dims(c), stream)
    fn = L.ts_block_cost_sampled_bwd if entry == "sampled" else L.ts_block_cost_sampled_warped_bwd
    return lambda: fn(_ptr(vL), _ptr(vR), _ptr(vd), _ptr(vg), _ptr(gL), _ptr(gR), _ptr(gD), _ptr(vws), *_dims(c), stream)


def _forward(L, stream, c, entry, ins, off):
    """one forward entry on sentinel arenas -> its output on the host"""
    (aL, vL), (aR, vR), (ad, vd) = ins
    ao, vo = _carve((c.B, _out_channels(entry, c.C, c.scales), c.D, c.H, c.W), off, out=True)
    aws, vws = _workspace(L, _dims(c))
    _run([aL, aR, ad, ao, aws], _fwd_call(L, stream, entry, c, vL, vR, vd, vo, vws))
    _finite(vo)
    return vo.cpu()


def _check_forward(c, entry, got, refs, left):
    rep = _Report(c.name, entry + " " + K.fwd_form(entry, c.W, c.D, c.aligned, lanes=True))
    if entry == "int":
        f64, f32 = refs["int"]
        rep.within("out", K.err_planes(got, f64), K.err_planes(f32, f64), K.BASE["out"])
    else:
        sl = K.entry_slice(entry, c.C)
        f32 = refs["fp32"][:, sl]
        rep.within("mixed", K.err_planes(got, refs["mixed"][:, sl]), K.err_planes(f32, refs["mixed"][:, sl]), K.BASE["out"])
        rep.within("exact", K.err_planes(got, refs["exact"][:, sl]), K.err_planes(f32, refs["exact"][:, sl]), K.BASE["out"])
        if entry == "sampled":
            rep.exact("reference-half", got[:, :c.C], left.unsqueeze(2).expand(c.B, c.C, c.D, c.H, c.W))
        if c.content == "far" and entry != "corr":
            w0 = c.C if entry == "sampled" else 0
            rep.exact("far-zeros", got[:, w0:w0 + c.C], torch.zeros(c.B, c.C, c.D, c.H, c.W))
    rep.close()


@pytest.mark.parametrize("case", K.FWD, ids=_ids)
def test_forward_entries(case):
    L, stream = _api()
    c, off = case, 0 if case.aligned else 1
    left, right, d, _, _ = K.inputs(c)
    refs = K.fwd_reference(c)
    ins = [_carve(t.shape, off, fill=t) for t in (left, right, d)]
    for entry in K.FWD_ENTRIES:
        _check_forward(c, entry, _forward(L, stream, c, entry, ins, off), refs, left)


def _backward(L, stream, c, entry, ins, gout, off, null=None, grads_off=None):
    """one backward entry on sentinel arenas, the gradient pointer `null` (0, 1, 2) NULL, the gradient buffers `grads_off` elements past
    16 bytes (default: as the inputs) -> (grad_left, grad_right[, grad_disp])"""
    grads_off = off if grads_off is None else grads_off
    (aL, vL), (aR, vR), (ad, vd) = ins
    ag, vg = _carve(gout.shape, off, fill=gout)
    shapes = [(c.B, c.C, c.H, c.W)] * 2 + ([(c.B, c.D, c.H, c.W)] if entry != "int" else [])
    outs = [(None, None) if i == null else _carve(s, grads_off, out=True) for i, s in enumerate(shapes)]
    gv = [v for _, v in outs] + [None] * (3 - len(outs))
    aws, vws = _workspace(L, _dims(c), bwd=True)
    _run([aL, aR, ad, ag, aws] + [a for a, _ in outs if a is not None], _bwd_call(L, stream, entry, c, vL, vR, vd, vg, gv[0], gv[1], gv[2], vws), twice=False)
    _finite(*[v for _, v in outs if v is not None])
    return [None if v is None else v.cpu() for _, v in outs]


def _check_backward(c, entry, got, ref64, ref32, note="", grads_aligned=True):
    rep = _Report(c.name, entry + " " + K.bwd_form(entry, c.W, c.D, c.aligned, lanes=True, grads_aligned=grads_aligned) + note)
    for q, g, r64, r32 in zip(("grad_left", "grad_right", "grad_disp"), got, ref64, ref32):
        if g is not None:
            rep.within(q, K.err_tensor(g, r64), K.err_tensor(r32, r64), K.BASE["grad"])
    if c.content == "far" and entry != "int":               # every tap outside the row: nothing reaches the right map or the candidates
        if got[1] is not None:
            rep.exact("far-grad_right", got[1], torch.zeros(c.B, c.C, c.H, c.W))
        if got[2] is not None:
            rep.exact("far-|grad_disp|", got[2].abs(), torch.zeros(c.B, c.D, c.H, c.W))
    rep.close()


def _grad_out(c, entry, gi, gs):
    return gi if entry == "int" else (gs if entry == "sampled" else gs[:, c.C:].contiguous())


@pytest.mark.parametrize("case", K.BWD, ids=_ids)
def test_backward_entries(case):
    L, stream = _api()
    c, off = case, 0 if case.aligned else 1
    left, right, d, gi, gs = K.inputs(c)
    refs = K.bwd_reference(c)
    ins = [_carve(t.shape, off, fill=t) for t in (left, right, d)]
    for entry in K.BWD_ENTRIES:
        got = _backward(L, stream, c, entry, ins, _grad_out(c, entry, gi, gs), off)
        _check_backward(c, entry, got, *refs[entry])


@pytest.mark.parametrize("case", K.NULLS, ids=_ids)
def test_backward_with_each_gradient_pointer_null(case):
    """a NULL gradient pointer leaves the other gradients what they were"""
    L, stream = _api()
    c = case
    left, right, d, gi, gs = K.inputs(c)
    refs = K.bwd_reference(c)
    ins = [_carve(t.shape, 0, fill=t) for t in (left, right, d)]
    for entry in K.BWD_ENTRIES:
        for null in range(2 if entry == "int" else 3):
            got = _backward(L, stream, c, entry, ins, _grad_out(c, entry, gi, gs), 0, null=null)
            assert got[null] is None
            _check_backward(c, entry, got, *refs[entry], note=" no " + ("grad_left", "grad_right", "grad_disp")[null])


@pytest.mark.parametrize("case", K.GRADS_OFF, ids=_ids)
def test_backward_into_gradient_buffers_off_16_bytes(case):
    """aligned inputs of an aligned width, grad_left / grad_right / grad_disp one element off 16 bytes: the row and tile kernels store
    the feature gradients 16 bytes at a time, so the launch rule has to leave the row form and take the tile form's scalar
    instantiation (it used to decide by the inputs alone); block_cost_bwd_main adds element by element either way"""
    L, stream = _api()
    c = case
    left, right, d, gi, gs = K.inputs(c)
    refs = K.bwd_reference(c)
    ins = [_carve(t.shape, 0, fill=t) for t in (left, right, d)]
    for entry in K.BWD_ENTRIES:
        got = _backward(L, stream, c, entry, ins, _grad_out(c, entry, gi, gs), 0, grads_off=1)
        _check_backward(c, entry, got, *refs[entry], note=" grads-off1", grads_aligned=False)


@pytest.mark.parametrize("case,entry", list(zip(K.MANY_PLANES, ("int", "sampled"))), ids=lambda v: v if isinstance(v, str) else v.name)
def test_more_planes_than_a_grid_dimension(case, entry):
    """B C/8 D > 65535 planes of the pooled maps: the backward takes the adjoint's generic form, the forward's expansion folds the planes
    over two grid dimensions"""
    L, stream = _api()
    c = case
    left, right, d, gi, gs = K.inputs(c)
    ins = [_carve(t.shape, 0, fill=t) for t in (left, right, d)]
    with torch.no_grad():
        f64 = R.block_cost(left.double(), right.double(), c.D if entry == "int" else d.double(), c.scales, pos_dtype=torch.float32)
        f32 = R.block_cost(left, right, c.D if entry == "int" else d, c.scales)
    got = _forward(L, stream, c, entry, ins, 0)
    rep = _Report(c.name, entry + " " + K.fwd_form(entry, c.W, c.D, lanes=True))
    rep.within("out" if entry == "int" else "mixed", K.err_planes(got, f64), K.err_planes(f32, f64), K.BASE["out"])
    rep.close()
    del got, f64, f32
    if entry == "int":
        r64, r32 = K._grads(torch.float64, c, "int"), K._grads(torch.float32, c, "int")
    else:
        r64, r32 = K._grads(torch.float64, c, "sampled", torch.float32)[0], K._grads(torch.float32, c, "sampled")[0]
    got = _backward(L, stream, c, entry, ins, _grad_out(c, entry, gi, gs), 0)
    _check_backward(c, entry, got, r64, r32, note=" " + K.adjoint_form(*_dims(c)))


@pytest.mark.parametrize("W", K.SPLIT_W)
def test_split_input_is_the_plain_entry_on_the_concatenation(W):
    """ts_block_cost_sampled_corr_split_fwd, C = 64 = 32 | 32, four batch strides of their own: bit for bit"""
    L, stream = _api()
    B, C, cs, H, D, scales = 2, 64, 32, 5, 3, 3
    c = K.Case("split_w%d" % W, "fwd", B, C, H, W, D, scales, True, "std")
    left, right, d, _, _ = K.inputs(c)
    ins = [_carve(t.shape, 0, fill=t) for t in (left, right, d)]
    plain = _forward(L, stream, c, "corr", ins, 0)
    rep = _Report(c.name, "corr split 32|32")
    for extra in K.SPLIT_STRIDES:
        parts, strides = [], []
        for t, lo, e in ((left, 0, extra[0]), (left, cs, extra[1]), (right, 0, extra[2]), (right, cs, extra[3])):
            bs = cs * H * W + e
            a = Arena(B * bs, DEV)
            parts.append((a, a.carve((B, cs, H, W), (bs, H * W, W, 1), 0, fill=t[:, lo:lo + cs])))
            strides.append(bs)
        ao, vo = _carve((B, scales * (C // 8), D, H, W), 0, out=True)
        aws, vws = _workspace(L, _dims(c))
        (_, l1), (_, l2), (_, r1), (_, r2) = parts
        _run([a for a, _ in parts] + [ins[2][0], ao, aws],
             lambda: L.ts_block_cost_sampled_corr_split_fwd(_ptr(l1), _ptr(l2), _ptr(r1), _ptr(r2), _ptr(ins[2][1]), _ptr(vo), _ptr(vws), B, C, cs, H, W, D,
                                                            scales, *strides, stream))
        _finite(vo)
        rep.exact("strides+%d+%d+%d+%d/%s" % (extra + (K.fwd_form("corr", W, D, all(e % 4 == 0 for e in extra)),)), vo, plain)
    rep.close()


# ---- refusals: the documented status, no launch, every buffer as it was ----------------------------------------------------------
_OK = dict(B=1, C=8, H=5, W=9, D=3, scales=3)
REFUSALS = [("C=12", dict(C=12), K.TS_ERR_SHAPE, None), ("C=4", dict(C=4), K.TS_ERR_SHAPE, None), ("H=3", dict(H=3), K.TS_ERR_UNSUPPORTED, None),
            ("W=3", dict(W=3), K.TS_ERR_UNSUPPORTED, None), ("D=1", dict(D=1), K.TS_ERR_UNSUPPORTED, "sampled"), ("scales=0", dict(scales=0), K.TS_ERR_UNSUPPORTED, None),
            ("scales=4", dict(scales=4), K.TS_ERR_UNSUPPORTED, None)]
REFUSALS += [("null_%s" % p, dict(null=p), K.TS_ERR_NULL, None) for p in ("left", "right", "disp", "out", "workspace")]


@pytest.mark.parametrize("name,change,want,only", REFUSALS, ids=[r[0] for r in REFUSALS])
def test_refusals(name, change, want, only):
    """C % 8 != 0, H or W < 4, sampled D = 1, scales 0 and 4, a NULL required pointer (`out` = grad_out for the backward): every entry.
    The buffers are sized for the largest of the refused and the valid shape, so that a launch would show."""
    L, stream = _api()
    dims = dict(_OK)
    dims.update({k: v for k, v in change.items() if k != "null"})
    null = change.get("null")
    big = {k: max(_OK[k], dims[k]) for k in _OK}
    B, C, H, W, D = big["B"], 16, big["H"], big["W"], big["D"]
    c = K.Case(name, "fwd", dims["B"], dims["C"], dims["H"], dims["W"], dims["D"], dims["scales"], True, "std")
    tens = lambda shape: _carve(shape, 0, fill=torch.zeros(shape))
    for side, entries in (("fwd", K.FWD_ENTRIES), ("bwd", K.BWD_ENTRIES)):
        for entry in entries:
            sampled = entry != "int"
            if (only == "sampled" and not sampled) or (null == "disp" and not sampled):
                continue
            (aL, vL), (aR, vR), (ad, vd) = tens((B, C, H, W)), tens((B, C, H, W)), tens((B, D, H, W))
            ao, vo = _carve((B, 2 * C + 3 * (C // 8), D, H, W), 0, out=(side == "fwd"))
            aws = Arena(L.ts_block_cost_workspace_bytes(B, C, H, W, D, 3) // 4, DEV)
            vws = aws.carve((aws.span,), out=True)
            p = {"left": vL, "right": vR, "disp": vd, "out": vo, "workspace": vws}
            if null:
                p[null] = None
            arenas = [aL, aR, ad, ao, aws]
            if side == "fwd":
                call = _fwd_call(L, stream, entry, c, p["left"], p["right"], p["disp"], p["out"], p["workspace"])
            else:
                grads = [_carve((B, C, H, W), 0, out=True), _carve((B, C, H, W), 0, out=True), _carve((B, D, H, W), 0, out=True)]
                arenas += [a for a, _ in grads]
                call = _bwd_call(L, stream, entry, c, p["left"], p["right"], p["disp"], p["out"], grads[0][1], grads[1][1], grads[2][1], p["workspace"])
            _run(arenas, call, want_rc=want)
            for a in arenas:
                assert torch.equal(a.buf, a.snap), "%s %s %s: a refused call wrote" % (name, side, entry)
            assert bool((aws.buf == SENTINEL).all()) and (side == "bwd" or bool((ao.buf == SENTINEL).all()))
