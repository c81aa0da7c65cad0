"""Disparity evaluation on the device (temporalstereo_amd/evaluation.py, csrc/evaluation.hip) against the reference's own
calc_error / do_evaluation / do_occlusion_evaluation and log_metric (tests/golden/eval_*.npz, tools/gen_golden.py --only-eval),
against a CPU restatement at full size, and end to end on a planted scene."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import parity_tools as PT
import synth
from temporalstereo_amd import _lib, evaluation as ev
from temporalstereo_amd.losses import rescale_to_full

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
CASES = ("eval_dense", "eval_sparse", "eval_none_valid", "eval_no_bounds", "eval_ragged", "eval_nonfinite", "eval_occlusion")
KEYS = ('1px', '2px', '3px', '5px', 'epe')
DEV = torch.device("cuda:0")


def _load(name):
    """The fixture's inputs rebuilt exactly (int16 / int8 storage, see tools/gen_golden.py eval_cases) + the reference's outputs."""
    g = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
    gl = g["gt_left_q128"].astype(np.float32) / np.float32(128)
    gr = g["gt_right_q128"].astype(np.float32) / np.float32(128)
    e0 = gl + (g["est0_off_q16"].astype(np.float32) + np.float32(0.5)) / np.float32(16)
    if g["nonfinite_at"][0] >= 0:
        e0.reshape(-1)[g["nonfinite_at"][0]] = np.nan
        e0.reshape(-1)[g["nonfinite_at"][1]] = np.inf
    ests = [e0] + [g["est%d" % i] for i in range(1, len(g["levels"]))]
    lb = float(g["lb"]) if int(g["has_lb"]) else None
    ub = float(g["ub"]) if int(g["has_ub"]) else None
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return g, d(gl), d(gr), [d(e) for e in ests], lb, ub


def _check(got, ref, n, what):
    """got / ref: [5] = {1px, 2px, 3px, 5px, epe}; n = the split's valid count.  Counts exact, epe to rtol 2e-6, NaN where NaN."""
    got = np.asarray(got, dtype=np.float64)
    ref = np.asarray(ref, dtype=np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), "%s: NaN pattern %s vs reference %s" % (what, got, ref)
    if n > 0:
        np.testing.assert_array_equal(np.round(got[:4] * n / 100), np.round(ref[:4] * n / 100), err_msg=what + ": counts")
    np.testing.assert_allclose(got[:4], ref[:4], rtol=1e-6, atol=0, err_msg=what + ": percentages")
    ok = ~np.isnan(ref[4:])
    np.testing.assert_allclose(got[4:][ok], ref[4:][ok], rtol=2e-6, atol=0, err_msg=what + ": epe")


def _vec(dct, prefix=''):
    return [float(dct[prefix + k].item()) for k in KEYS]


@pytest.mark.parametrize("name", CASES)
def test_drop_ins_against_reference_fixtures(name):
    g, gl, gr, ests, lb, ub = _load(name)
    assert float(g["margin"]) >= 1e-3, "fixture too close to a threshold to be ulp-robust"
    n_all, n_occ, n_noc = (int(v) for v in g["n_valid"])
    ce = ev.calc_error(ests[0], gl, lb=lb, ub=ub)
    de = ev.do_evaluation(ests[0], gl, lb, ub)
    oe = ev.do_occlusion_evaluation(ests[0], gl, gr, lb, ub)
    assert sorted(ce) == sorted(de) == sorted(KEYS)
    assert sorted(oe) == sorted(['occ_' + k for k in KEYS] + ['noc_' + k for k in KEYS])
    for v in list(ce.values()) + list(oe.values()):
        assert v.shape == (1,) and v.dtype == torch.float32 and v.is_cuda
    _check(_vec(ce), g["calc_error"], n_all, name + " calc_error")
    _check(_vec(de), g["do_evaluation"], n_all, name + " do_evaluation")
    _check(_vec(oe, 'occ_'), g["occ"][0], n_occ, name + " occ")
    _check(_vec(oe, 'noc_'), g["occ"][1], n_noc, name + " noc")


@pytest.mark.parametrize("name", CASES)
def test_validation_metrics_against_composed_log_metric(name):
    """validation_metrics on the native-resolution levels vs validation_step's F.interpolate + log_metric of the reference.
    eval_nonfinite level 0 is left to the drop-in test: the reference's same-size F.interpolate turns the planted inf into NaN
    (a zero weight times inf), where the fused form reads a full-size level as it is."""
    g, gl, gr, ests, lb, ub = _load(name)
    assert float(g["margin"]) >= 1e-3
    got = ev.validation_metrics(ests, gl, gr, lb=lb, ub=ub)
    assert sorted(got) == sorted(str(k) for k in g["log_metric_keys"])
    assert list(got) == ev.metric_keys(len(ests))
    for i in range(len(ests)):
        if name == "eval_nonfinite" and i == 0:
            continue
        for si, s in enumerate(("all", "occ", "noc")):
            _check(_vec(got, 'metric_disparity_{}/{}_'.format(i, s)), g["log_metric"][i, si], int(g["n_valid"][si]),
                   "%s level %d %s" % (name, i, s))


def _scene(B, H, W, seed):
    """A smooth left disparity, a right one consistent with it up to small noise, an occluder band, some out-of-range pixels;
    four native-resolution estimates (full, 1/4, 1/4, 1/8)."""
    yy = torch.arange(H, dtype=torch.float64).view(1, 1, H, 1)
    xx = torch.arange(W, dtype=torch.float64).view(1, 1, 1, W)
    ph = torch.from_numpy(synth.uniform(seed, "ph", (B, 1, 1, 1), 0.0, 6.283)).double()
    d = lambda y, x: 20.0 + 15.0 * y / H + 8.0 * torch.sin(2 * np.pi * x / W + ph) + 4.0 * torch.cos(2 * np.pi * y / H + ph)
    xl = xx + d(yy, xx)
    for _ in range(30):
        xl = xx + d(yy, xl)
    gl = d(yy, xx).float()
    gr = (d(yy, xl) + torch.from_numpy(synth.normal(seed, "nr", (B, 1, H, W), 0.3)).double()).float()
    gr[..., W // 3:W // 3 + W // 10] += 25.0
    r = torch.from_numpy(synth.uniform(seed, "oor", (B, 1, H, W)))
    gl = torch.where(r < 0.02, torch.full_like(gl, 250.0), torch.where(r > 0.98, torch.zeros_like(gl), gl))
    ests = []
    for li, (h, w) in enumerate([(H, W), (H // 4, W // 4), (H // 4, W // 4), (H // 8, W // 8)]):
        base = F.interpolate(gl, size=(h, w), mode='bilinear', align_corners=True) * (w / W)
        ests.append((base + torch.from_numpy(synth.normal(seed, "e%d" % li, (B, 1, h, w), 2.5 * w / W))).contiguous())
    return gl.contiguous(), gr.contiguous(), ests


def test_fused_equals_rescale_then_drop_ins_bit_for_bit():
    B, H, W = 4, 544, 960
    gl, gr, ests = _scene(B, H, W, synth.SEED0 + 700)
    gl, gr, ests = gl.to(DEV), gr.to(DEV), [e.to(DEV) for e in ests]
    got = ev.validation_metrics(ests, gl, gr, lb=0, ub=192)
    for i, e in enumerate(ests):
        full = rescale_to_full(e, (H, W))
        ref = dict(ev.do_evaluation(full, gl, 0, 192))
        ref.update({k: v for k, v in ev.do_occlusion_evaluation(full, gl, gr, 0, 192).items()})
        for s in ("all", "occ", "noc"):
            for k in KEYS:
                a = got['metric_disparity_{}/{}_{}'.format(i, s, k)]
                b = ref[k if s == "all" else s + '_' + k]
                assert torch.equal(a, b), "level %d %s %s: %r vs %r" % (i, s, k, a.item(), b.item())


def _cpu_metrics(ests, gl, gr, lb, ub, tol=1e-4):
    """torch-CPU restatement of validation_step's resize + log_metric (TemporalStereo.py:183, :463-486; pixel_error.py; eval.py;
    inverse_warp.py): -> per level [3 splits][5], N per split, and how many pixels sit within `tol` of a decision threshold
    (per level x split for the counts, and of the occlusion test)."""
    B, _, H, W = gl.shape
    x = torch.arange(W, dtype=torch.float32).view(1, W).expand(H, W)
    y = torch.arange(H, dtype=torch.float32).view(H, 1).expand(H, W)
    X = x.unsqueeze(0) + (-gl[:, 0])
    Y = y.unsqueeze(0).expand_as(X)
    grid = torch.stack((2 * X / (W - 1) - 1, 2 * Y / (H - 1) - 1), dim=3)
    warp = F.grid_sample(gr, grid, mode='bilinear', padding_mode='zeros', align_corners=True)
    occ = ((warp - gl).abs() > 1.0) | (warp.abs() < 1e-6)
    occ_border = int(((((warp - gl).abs() - 1.0).abs() < tol) | ((warp != 0) & ((warp.abs() - 1e-6).abs() < tol))).sum())
    masks = [torch.ones_like(occ), occ, ~occ]
    res, border, ns = [], [], []
    for e in ests:
        full = F.interpolate(e * W / e.shape[-1], size=(H, W), mode='bilinear', align_corners=True)
        lv, bv = [], []
        for m in masks:
            mf = m.float()
            g, d = gl * mf, full * mf
            v = torch.ones_like(m)
            if lb is not None:
                v &= g > lb
            if ub is not None:
                v &= g < ub
            a = (g - d).abs()[v]
            n = int(v.sum())
            row = [float((a > t).sum()) / n * 100 if n else 0.0 for t in (1, 2, 3, 5)] + [float(a.double().mean()) if n else 0.0]
            lv.append(row)
            bv.append(int(sum(((a - t).abs() < tol).sum() for t in (1, 2, 3, 5))))
            if len(ns) < 3:
                ns.append(n)
        res.append(lv)
        border.append(bv)
    return res, ns, border, occ_border


@pytest.mark.parametrize("B", [1, 4])
def test_full_size_against_cpu_restatement(B):
    H, W = 544, 960
    gl, gr, ests = _scene(B, H, W, synth.SEED0 + 710 + B)
    torch.set_num_threads(16)
    ref, ns, border, occ_border = _cpu_metrics(ests, gl, gr, 0, 192)
    got = ev.validation_metrics([e.to(DEV) for e in ests], gl.to(DEV), gr.to(DEV), lb=0, ub=192)
    for i in range(len(ests)):
        for si, s in enumerate(("all", "occ", "noc")):
            v = _vec(got, 'metric_disparity_{}/{}_'.format(i, s))
            n = ns[si]
            allow = border[i][si] + occ_border
            for k in range(4):
                assert abs(round(v[k] * n / 100) - round(ref[i][si][k] * n / 100)) <= allow, (i, s, KEYS[k], v[k], ref[i][si][k], allow)
            # a pixel that changes side of the occlusion test moves |e| / N between the splits' means
            assert abs(v[4] - ref[i][si][4]) <= 1e-5 * abs(ref[i][si][4]) + occ_border * 200.0 / max(n, 1), (i, s, v[4], ref[i][si][4])


def test_end_to_end_planted_sequence():
    """The engine's disparities of a planted scene, scored by validation_metrics: level 0's all_epe is parity_tools.epe."""
    from temporalstereo_amd.aggregation.engine import InferenceEngine
    c = PT.CONFIGS["configs[1] things 544x960 D=192 single B=1"]
    case = PT.PlantedCase(c, synth.SEED0 + 3, DEV)
    eng = InferenceEngine(case.net, backend="native", replay="plan")
    out = eng(*case.frames_gpu[0], {})
    disps = [d.detach().clone() for d in out[0]]
    gt = case.gt[0].to(DEV).reshape(disps[0].shape).contiguous()
    got = ev.validation_metrics(disps, gt, lb=0, ub=case.max_disp)
    assert list(got) == ev.metric_keys(len(disps), occlusion=False)
    e = PT.epe(disps[0], case.gt[0].reshape(disps[0].shape), case.max_disp)
    assert abs(got['metric_disparity_0/all_epe'].item() - e) <= 1e-5 * abs(e), (got['metric_disparity_0/all_epe'].item(), e)


def test_bit_identical_from_run_to_run():
    gl, gr, ests = _scene(2, 136, 240, synth.SEED0 + 720)
    gl, gr, ests = gl.to(DEV), gr.to(DEV), [e.to(DEV) for e in ests]
    a = ev._metrics(ests, gl, gr, 0, 192)
    b = ev._metrics(ests, gl, gr, 0, 192)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))


def test_recorded_plan_replays_on_new_ground_truth():
    gl, gr, ests = _scene(2, 136, 240, synth.SEED0 + 730)
    gl, gr, ests = gl.to(DEV), gr.to(DEV), [e.to(DEV) for e in ests]
    six = ests + ests[1:3]
    with _lib.Recorder() as rec:
        got = ev.validation_metrics(six, gl, gr, lb=0, ub=192)
    assert len(rec) == 2 and [n for n, _ in rec.log] == ["ts_disp_metrics_fwd"] * 2     # two groups (4 + 2), two launches each
    before = {k: v.clone() for k, v in got.items()}
    gl2, gr2, _ = _scene(2, 136, 240, synth.SEED0 + 731)
    gl.copy_(gl2.to(DEV))
    gr.copy_(gr2.to(DEV))
    rec.run()
    fresh = ev.validation_metrics(six, gl, gr, lb=0, ub=192)
    torch.cuda.synchronize()
    assert list(got) == list(fresh)
    for k in fresh:
        assert torch.equal(got[k], fresh[k]), k
    assert not torch.equal(before['metric_disparity_0/all_epe'], got['metric_disparity_0/all_epe'])


def test_refusals():
    gl, gr, ests = _scene(2, 32, 64, synth.SEED0 + 740)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ev.validation_metrics(ests, gl, gr)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ev.calc_error(ests[0], gl)
    gl, gr, ests = gl.to(DEV), gr.to(DEV), [e.to(DEV) for e in ests]
    with pytest.raises(ValueError):
        ev.validation_metrics([ests[1][:1]], gl)                       # batch 1 against 2
    with pytest.raises(ValueError):
        ev.do_occlusion_evaluation(ests[0], gl, gr[..., :-1], 0, 192)
    with pytest.raises(ValueError):
        ev.validation_metrics(ests, gl, gr[:1])
    with pytest.raises(ValueError):
        ev.calc_error(ests[0], gl[..., :-1])
    with pytest.raises(ValueError):
        ev._metrics([], gl, None, 0, 192)
    L = _lib.lib()
    out = torch.empty((4, 3, 5), device=DEV)
    ws = torch.empty(int(L.ts_disp_metrics_workspace_bytes(2, 32, 64)), device=DEV, dtype=torch.uint8)
    args = lambda n: [_lib.ptr(ests[0])] * 4 + [n] + [32, 64] * 4 + [_lib.ptr(gl), _lib.ptr(gr), 2, 32, 64, 0.0, 192.0, 3,
                                                                       _lib.ptr(out), _lib.ptr(ws), None]
    assert L.ts_disp_metrics_fwd(*args(0)) == -2
    assert L.ts_disp_metrics_fwd(*args(5)) == -2
    assert L.ts_disp_metrics_fwd(*args(1)) == 0
    torch.cuda.synchronize()
