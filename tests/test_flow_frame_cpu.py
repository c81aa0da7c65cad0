"""CPU: the optical-flow metrics, colour maps and KITTI decode (temporalstereo_amd/evaluation.py, visualization.py, preprocess.py;
csrc/flow_frame.hip) without a GPU -- tests/flow_frame_ref.py, the float32 restatement the device follows, is pinned to the
reference-made fixtures tests/golden/flow_frame_*.npz (tools/gen_golden.py --only-flow-frame); the colour wheel, the flag words
and the signature table agree with include/ts_hip.h; the entry points refuse bad arguments before any launch."""
import os
import re

import numpy as np
import pytest
import torch

import flow_frame_ref as R
from temporalstereo_amd import _lib, evaluation as ev, preprocess as pp, visualization as vz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
VARIANTS = ((0.0, 400, False), (-1.0, 400, True), (2.0, 30.0, False), (-1.0, 400, False))        # (lb, ub, sparse) of a fixture's metrics[0..3]
ENTRIES = ("ts_flow_metrics_workspace_bytes", "ts_flow_metrics_fwd", "ts_flow_render_workspace_bytes", "ts_flow_render_fwd",
           "ts_flow_u16_decode_fwd")


def _full(g):
    return g["est_full"] if "est_full" in g else g["est"]


@pytest.mark.parametrize("name", R.CASES)
def test_restatement_reproduces_the_metrics(name):
    g = R.load_fixture(name)
    full = _full(g)
    for i, (lb, ub, sparse) in enumerate(VARIANTS):
        got, n = R.calc_error(full, g["gt"], lb, ub, sparse)
        ref = g["metrics"][i]
        assert n == int(g["n_valid"][i])
        assert np.array_equal(got[:4], ref[:4]), (name, i, got, ref)
        assert np.array_equal(np.isnan(got), np.isnan(ref))
        if np.isfinite(ref[4]):
            assert abs(float(got[4]) - float(ref[4])) <= 2e-6 * abs(float(ref[4]))
    assert np.array_equal(g["do_flow_evaluation"], g["metrics"][0], equal_nan=True)      # called with lb=2, ub=30: not passed on


def test_restatement_rescale_is_the_torch_composition_to_a_few_ulp():
    g = R.load_fixture("rescaled")
    mine = R.rescale(g["est"], g["gt"].shape[-2:])
    assert mine.shape == g["est_full"].shape
    assert float(np.abs(mine.astype(np.float64) - g["est_full"]).max()) <= float(g["tau"])
    assert int(g["tie_class"].sum()) <= 0.005 * g["tie_class"].size


@pytest.mark.parametrize("name", R.CASES)
def test_restatement_reproduces_radii_classes_and_colours(name):
    g = R.load_fixture(name)
    full, gt = _full(g), g["gt"]
    fh, gh = R.hwc(full), R.hwc(gt)
    B = full.shape[0]
    assert np.array_equal(g["max_rad_est"], np.array([R.max_rad(fh[b]) for b in range(B)]))
    assert np.array_equal(g["max_rad_gt"], np.array([R.max_rad(gh[b]) for b in range(B)]))
    if "class_idx" in g:
        assert np.array_equal(g["class_idx"], R.err_class(full, gt))
    if "class_val_idx" in g:
        assert np.array_equal(g["class_val_idx"], R.err_class(full, gt, g["gt_val_half"].astype(np.float32) / np.float32(2)))
    jobs = []       # (the reference's image, the map, its maxima or None, the pixels where the two may take different branches, dev)
    if "color_est" in g:
        jobs.append((g["color_est"], fh, None, g["bright_est"], g["dev_own"], True))
    if "color_gt" in g:
        jobs.append((g["color_gt"], gh, None, g["bright_gt"], g["dev_own"], True))
    if "color_est_given" in g:
        jobs.append((g["color_est_given"], fh, g["given_max"], g["tie_est_given"], g["dev_given"], False))
    if "color_shared_est" in g:
        jobs.append((g["color_shared_est"], fh, g["shared_max"], g["tie_shared_est"], g["dev_given"], True))
        jobs.append((g["color_shared_gt"], gh, g["shared_max"], g["tie_shared_gt"], g["dev_given"], True))
    for ref, maps, maxima, skip, dev, data_max in jobs:
        mine = np.stack([R.flow_to_color(maps[b], None if maxima is None else maxima[b], data_max=data_max) for b in range(B)])
        d = np.abs(mine.astype(np.float64) - ref)
        assert float(d[~skip].max(initial=0.0)) <= float(dev), (name, float(d[~skip].max()), float(dev))
        unk = np.stack([R.unknown(maps[b]) for b in range(B)])
        assert (mine[unk] == 0).all() and (ref[unk] == 0).all()


def test_reference_properties_the_kernels_must_keep():
    g = R.load_fixture("dense")
    # the planted pixels: E exactly on the end points 0.1875, 3 and 48 falls into the LATER class; err exactly 1, 2, 3, 5
    assert g["class_idx"][0, 5, 10:13].tolist() == [1, 5, 9]
    err = R.flow_error(g["est"], g["gt"])[0, 5, 10:16]
    assert err.tolist() == [0.1875, 3.0, 48.0, 1.0, 2.0, 5.0]
    # the wheel does not close: (3, +0.0) and (3, -0.0) differ
    a, b = g["color_est"][0, 7, 20], g["color_est"][0, 7, 21]
    assert np.signbit(g["est"][0, 1, 7, 21]) and not np.signbit(g["est"][0, 1, 7, 20])
    assert abs(float(a[2]) - float(b[2])) > 1e-3 and a[0] == b[0]        # 300 x the colour tolerance
    # the reference darkens the pixel that set the maximum; the restatement (and the device) keep it inside the disc
    y, x = (int(v[0]) for v in np.nonzero(g["bright_est"][0]))
    mine = R.flow_to_color(R.hwc(g["est"])[0])[y, x]
    assert np.allclose(g["color_est"][0, y, x], 0.75 * mine, rtol=0, atol=1e-5) and float(mine.max()) > 0.99
    # a given maximum leaves a share of the pixels outside
    assert 0.03 <= float(R.load_fixture("given_max")["outside_share"]) <= 0.8
    nf = R.load_fixture("nonfinite")
    assert np.isnan(nf["metrics"][0, 4]) and np.isfinite(nf["metrics"][0, :4]).all()
    nv = R.load_fixture("none_valid")          # a ground truth of zeros: nothing valid, unless lb < 0 and the map is not sparse
    assert (nv["metrics"][:3] == 0).all() and nv["n_valid"].tolist() == [0, 0, 0, 16 * 24] and nv["metrics"][3, 4] > 0
    sp = R.load_fixture("sparse")
    assert (sp["gt"][:, :, 10:20, 8:32] == 0).all() and int(sp["n_valid"][3]) - int(sp["n_valid"][1]) == 2 * 10 * 24       # lb < 0: only `sparse` drops the zeros


def test_decode_restatement_and_quantisation():
    g = dict(np.load(os.path.join(R.GOLDEN, "flow_frame_kitti.npz")))
    flow, valid = R.decode_kitti(g["raw"])
    assert np.array_equal(flow, g["flow"]) and np.array_equal(valid, g["valid"])
    assert 0.1 < float((~valid).mean()) < 0.5 and (flow[:, 0][~valid[:, 0]] == 0).all()
    assert flow[0, 0, 0, 0] == -512.0 and flow[0, 1, 0, 0] == np.float32(32767) / np.float32(64)
    assert R.q8(np.array([np.nan, -1.0, 0.5, 2.0], dtype=np.float32)).tolist() == [0, 0, 128, 255]


def test_color_wheel_is_the_references():
    g = R.load_fixture("dense")
    wheel = vz.make_color_wheel()
    assert wheel.dtype == np.float64 and wheel.shape == (55, 3)
    assert np.array_equal(wheel, g["wheel"]) and np.array_equal(R.make_color_wheel(), g["wheel"])


def test_flag_words_and_signature_table_match_the_header():
    header = open(os.path.join(ROOT, "include", "ts_hip.h")).read()
    for flag in ("EST_COLOR", "GT_COLOR", "ERR_CLASS", "STATS", "UINT8", "CHW", "MAX_SHARED", "MAX_GIVEN", "EST_HWC", "GT_HWC"):
        assert int(re.search(r"#define TS_FLOW_RENDER_%s (\d+)" % flag, header).group(1)) == getattr(vz, "FLOW_" + flag), flag
    for flag in ("SPARSE", "EST_HWC", "GT_HWC"):
        assert int(re.search(r"#define TS_FLOW_%s (\d+)" % flag, header).group(1)) == getattr(ev, "FLOW_" + flag), flag
    assert int(re.search(r"#define TS_FLOW_STATS_FLOATS (\d+)", header).group(1)) == vz.FLOW_STATS_FLOATS
    assert int(re.search(r"#define TS_FLOW_U16_CHW (\d+)", header).group(1)) == pp.CHW
    for name in ENTRIES:
        assert name in _lib.SIGNATURES and name in header
        assert (name in _lib._QUERIES) == name.endswith("_bytes")


def test_entry_points_refuse_bad_arguments_without_a_gpu():
    L = _lib.lib()
    assert L.ts_version() >= 17
    assert L.ts_flow_metrics_workspace_bytes(1, 544, 960) > 0 and L.ts_flow_metrics_workspace_bytes(4, 544, 960) % 256 == 0
    assert L.ts_flow_render_workspace_bytes(2, 1, 1) > 0 and L.ts_flow_render_workspace_bytes(4, 544, 960) % 256 == 0
    for args in ((0, 8, 8), (1, 0, 8), (1, 8, -1), (1 << 15, 1 << 15, 8)):
        assert L.ts_flow_metrics_workspace_bytes(*args) == 0 and L.ts_flow_render_workspace_bytes(*args) == 0, args
    one = 256                                    # a non-NULL, aligned address that is never dereferenced: the checks come first
    m = lambda n, flags=0, gt=one: L.ts_flow_metrics_fwd(one, one, one, one, n, 8, 8, 8, 8, 8, 8, 8, 8, gt, 1, 8, 8, 0.0, 400.0, flags,
                                                         one, one, None)
    assert m(0) == -2 and m(5) == -2 and m(1, flags=8) == -2 and m(1, gt=None) == -1
    assert b"n_est" in (m(5), L.ts_last_error_string())[1]
    r = lambda flags, est=one, B=1: L.ts_flow_render_fwd(est, None, None, None, None, B, 8, 8, 8, 8, flags, None, None, None, None, None)
    assert r(0) == -2                                                    # no output selected
    assert r(1 << 10) == -2                                              # unknown flag
    assert r(vz.FLOW_EST_COLOR | vz.FLOW_MAX_SHARED | vz.FLOW_MAX_GIVEN) == -2
    assert r(vz.FLOW_EST_COLOR, est=None) == -1 and r(vz.FLOW_EST_COLOR) == -1 and r(vz.FLOW_ERR_CLASS) == -1
    assert r(vz.FLOW_STATS, B=0) == -2
    d = lambda raw=one, flow=one, H=8, flags=0: L.ts_flow_u16_decode_fwd(raw, 1, H, 8, flags, flow, None, None)
    assert d(raw=None) == -1 and d(flow=None) == -1 and d(H=0) == -2 and d(flags=2) == -2 and d(raw=257) == -4


def test_ops_refuse_cpu_tensors_and_bad_shapes():
    f = torch.zeros(2, 2, 8, 12)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ev.flow_calc_error(f, f)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ev.flow_validation_metrics([f], f)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        vz.flow_to_color(f, layout='CHW')
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        vz.render_flow_frame(f, f)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        pp.decode_kitti_flow(torch.zeros(8, 12, 3, dtype=torch.int16))
    # the reference's early returns
    z = ev.flow_calc_error(None, f)
    assert sorted(z) == sorted(R.KEYS) and all(v.shape == (1,) and not v.is_cuda and float(v) == 0 for v in z.values())
    with pytest.warns(UserWarning):
        assert ev.do_flow_evaluation(None, f) == {}
    with pytest.warns(UserWarning):
        assert ev.do_flow_evaluation(f, None) == {}
    assert ev.flow_validation_metrics([f], None) == {}
    assert ev.flow_metric_keys(2) == ['metric_flow_%d/all_%s' % (i, k) for i in range(2) for k in R.KEYS]
