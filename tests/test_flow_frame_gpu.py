"""Optical-flow metrics, colour maps and the KITTI decode on the device (temporalstereo_amd/evaluation.py, visualization.py,
preprocess.py; csrc/flow_frame.hip) against the reference's own flow_calc_error / do_flow_evaluation / flow_max_rad / flow_to_color /
flow_err_to_color / load_png (tests/golden/flow_frame_*.npz, tools/gen_golden.py --only-flow-frame).

Tolerances, all from tests/golden/PROVENANCE_flow_frame.txt: percentages, maximum radii, class maps and the decode are bit-exact
(every pixel count is far below 2^24, so the reference's float32 counting is exact); epe to the 2e-6 relative of
tests/test_evaluation_gpu.py (an fp64 sum against the reference's float32 mean); colours to 4 x the distance the generator measured
between the float32 restatement and the reference (dev_own / dev_given), outside the generator's near-tie masks; the rescaled case
against the torch composition, the counts within the generator's number of pixels within tau of a threshold."""
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import flow_frame_ref as R
from temporalstereo_amd import _lib, evaluation as ev, preprocess as pp, visualization as vz

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
VARIANTS = ((0.0, 400, False), (-1.0, 400, True), (2.0, 30.0, False), (-1.0, 400, False))      # (lb, ub, sparse) of metrics[0..3]
SAME_SIZE = tuple(n for n in R.CASES if n != "rescaled")
_CACHE = {}


def d(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def load(name):
    """the fixture (shared, never modified) with est / gt on the device as [B,2,H,W]"""
    if name not in _CACHE:
        g = R.load_fixture(name)
        g["est_d"], g["gt_d"] = d(g["est"]), d(g["gt"])
        _CACHE[name] = g
    return _CACHE[name]


def vec(dct, prefix=''):
    return np.array([float(dct[prefix + k].item()) for k in R.KEYS], dtype=np.float32)


def check_metrics(got, ref, what):
    assert np.array_equal(got[:4], ref[:4]), "%s: percentages %s vs the reference's %s" % (what, got, ref)
    assert np.array_equal(np.isnan(got), np.isnan(ref)), "%s: NaN pattern %s vs %s" % (what, got, ref)
    if np.isfinite(ref[4]):
        assert abs(float(got[4]) - float(ref[4])) <= 2e-6 * abs(float(ref[4])), "%s: epe %r vs %r" % (what, got[4], ref[4])
    else:
        assert np.array_equal(got[4:], ref[4:], equal_nan=True), what


# ----------------------------------------------------------------------------------------------------------------------- metrics
@pytest.mark.parametrize("name", SAME_SIZE)
def test_metrics_against_reference_fixtures(name):
    g = load(name)
    est, gt = g["est_d"], g["gt_d"]
    for i, (lb, ub, sparse) in enumerate(VARIANTS):
        res = ev.flow_calc_error(est, gt, lb=lb, ub=ub, sparse=sparse)
        assert sorted(res) == sorted(R.KEYS)
        for v in res.values():
            assert v.shape == (1,) and v.dtype == torch.float32 and v.is_cuda
        check_metrics(vec(res), g["metrics"][i], "%s variant %d" % (name, i))
    # the quirk: lb / ub are accepted and not passed on
    check_metrics(vec(ev.do_flow_evaluation(est, gt, lb=2.0, ub=30.0)), g["do_flow_evaluation"], name + " do_flow_evaluation")
    fused = ev.flow_validation_metrics([est, est], gt, lb=2.0, ub=30.0)
    assert list(fused) == ev.flow_metric_keys(2)
    for i in range(2):
        check_metrics(vec(fused, 'metric_flow_%d/all_' % i), g["metrics"][2], "%s fused level %d" % (name, i))
    if est.shape[0] == 1:                                                          # the reference's [2,H,W] form
        check_metrics(vec(ev.flow_calc_error(est[0], gt[0])), g["metrics"][0], name + " unbatched")


def test_metrics_of_rescaled_levels_against_the_torch_composition():
    g = load("rescaled")
    est, gt = g["est_d"], g["gt_d"]
    Hg, Wg = gt.shape[-2:]
    scale = torch.tensor([Wg / est.shape[-1], Hg / est.shape[-2]], device=DEV, dtype=torch.float32).view(1, 2, 1, 1)
    full = (F.interpolate(est, size=(Hg, Wg), mode='bilinear', align_corners=True) * scale).contiguous()
    assert float((full.cpu() - torch.from_numpy(g["est_full"])).abs().max()) <= float(g["tau"])
    for i, (lb, ub, sparse) in enumerate(VARIANTS):
        n = int(g["n_valid"][i])
        fused = ev.flow_validation_metrics([est, full, est, est], gt, lb=lb, ub=ub, sparse=sparse)
        ref_dev = vec(ev.flow_calc_error(full, gt, lb=lb, ub=ub, sparse=sparse))
        # a level at the ground truth's size is read as it is: the drop-in's bits
        assert np.array_equal(vec(fused, 'metric_flow_1/all_'), ref_dev)
        for ref, what in ((ref_dev, "torch composition on the device"), (g["metrics"][i], "torch composition, fixture")):
            for lvl in (0, 2, 3):
                got = vec(fused, 'metric_flow_%d/all_' % lvl)
                for k in range(4):
                    diff = abs(int(round(float(got[k]) * n / 100)) - int(round(float(ref[k]) * n / 100)))
                    assert diff <= int(g["near_thr"][i][k]), (what, i, lvl, R.KEYS[k], got[k], ref[k], int(g["near_thr"][i][k]))
                # err moves by at most tau per pixel
                assert abs(float(got[4]) - float(ref[4])) <= 2e-6 * abs(float(ref[4])) + float(g["tau"]), (what, i, lvl, got[4], ref[4])


# ----------------------------------------------------------------------------------------------------------------------- colours
def color_jobs(g):
    """(key, map on the device [B,2,H,W], numpy map [B,H,W,2], maxima or None, pixels left to the restatement, dev, data_max)"""
    fh, gh = R.hwc(g["est"]), R.hwc(g["gt"])
    jobs = []
    if "color_est" in g:
        jobs.append(("color_est", g["est_d"], fh, None, g["bright_est"], g["dev_own"], True))
    if "color_gt" in g:
        jobs.append(("color_gt", g["gt_d"], gh, None, g["bright_gt"], g["dev_own"], True))
    if "color_est_given" in g:
        jobs.append(("color_est_given", g["est_d"], fh, g["given_max"], g["tie_est_given"], g["dev_given"], False))
    return jobs


@pytest.mark.parametrize("name", [n for n in SAME_SIZE if n != "sparse"])
def test_flow_colours_against_reference_fixtures(name):
    g = load(name)
    B = g["est"].shape[0]
    assert torch.equal(vz.flow_max_rad(g["est_d"], layout='CHW'), d(g["max_rad_est"]))
    assert torch.equal(vz.flow_max_rad(g["gt_d"], layout='CHW'), d(g["max_rad_gt"]))
    for key, dev_map, np_map, maxima, skip, dev, data_max in color_jobs(g):
        mx = None if maxima is None else d(maxima)
        got = vz.flow_to_color(dev_map, max_rad=mx, layout='CHW')
        assert got.dtype == torch.float32 and tuple(got.shape) == g[key].shape
        got = got.cpu().numpy()
        tol = 4 * float(dev)
        diff = np.abs(got.astype(np.float64) - g[key])
        assert float(diff[~skip].max(initial=0.0)) <= tol, (name, key, float(diff[~skip].max()), tol)
        mine = np.stack([R.flow_to_color(np_map[b], None if maxima is None else maxima[b], data_max=data_max) for b in range(B)])
        assert float(np.abs(got.astype(np.float64) - mine)[skip].max(initial=0.0)) <= tol, (name, key, "near-tie / brightest pixels")
        unk = np.stack([R.unknown(np_map[b]) for b in range(B)])
        assert (got[unk] == 0).all(), (name, key, "unknown pixels are black")
        if maxima is None:
            # no mask: the pixel that sets a map's own maximum is inside the disc, so its held channel is 1 (darkened: 0.75)
            for b in range(B):
                kn = R.known(np_map[b])
                r0 = R.radius(kn[..., 0], kn[..., 1])
                if r0.max() > 0:
                    y, x = np.unravel_index(int(r0.argmax()), r0.shape)
                    assert float(got[b, y, x].max()) > 0.99, (name, key, b, got[b, y, x])
        if maxima is not None and B > 1:
            one = vz.flow_to_color(dev_map, max_rad=float(maxima[0]), layout='CHW')          # a number: every image's maximum
            assert np.array_equal(one[0].cpu().numpy(), got[0])


def test_shared_maximum_and_the_signed_zero_pair():
    g = load("shared")
    est, gt = g["est_d"], g["gt_d"]
    H = est.shape[-2]
    both = vz.render_flow_frame(est, gt, outputs=('flow_color',), dtype=torch.float32)['flow_color'].cpu().numpy()
    assert both.shape == (1, 2 * H, est.shape[-1], 3)
    tol = 4 * float(g["dev_given"])
    for part, key, tie, maps in ((both[:, :H], "color_shared_est", g["tie_shared_est"], R.hwc(g["est"])),
                                 (both[:, H:], "color_shared_gt", g["tie_shared_gt"], R.hwc(g["gt"]))):
        diff = np.abs(part.astype(np.float64) - g[key])
        assert float(diff[~tie].max(initial=0.0)) <= tol, (key, float(diff[~tie].max()))
        mine = R.flow_to_color(maps[0], g["shared_max"][0], data_max=True)[None]
        assert float(np.abs(part.astype(np.float64) - mine)[tie].max(initial=0.0)) <= tol, key
    stats = vz.flow_render_stats(est, gt)
    assert torch.equal(stats[:, 2], d(g["shared_max"])) and torch.equal(stats[:, 0], d(g["max_rad_est"]))
    # (3, +0.0) and (3, -0.0): the wheel does not close, atan2 must see the sign of the zero
    g = load("dense")
    got = vz.flow_to_color(g["est_d"], layout='CHW')[0].cpu().numpy()
    a, b, ra, rb = got[7, 20], got[7, 21], g["color_est"][0, 7, 20], g["color_est"][0, 7, 21]
    assert abs(float(ra[2]) - float(rb[2])) > 1e-3
    assert np.abs(a - ra).max() <= 4 * float(g["dev_own"]) and np.abs(b - rb).max() <= 4 * float(g["dev_own"])


@pytest.mark.parametrize("name", ["dense", "ragged"])          # row quads / single pixels
def test_uint8_and_chw_forms(name):
    g = load(name)
    est, gt = g["est_d"], g["gt_d"]
    f32 = vz.flow_to_color(est, layout='CHW')
    u8 = vz.flow_to_color(est, layout='CHW', dtype=torch.uint8)
    assert u8.dtype == torch.uint8 and np.array_equal(u8.cpu().numpy(), R.q8(f32.cpu().numpy()))
    for dt in (torch.float32, torch.uint8):
        hwc = vz.flow_to_color(est, layout='CHW', dtype=dt)
        chw = vz.flow_to_color(est, layout='CHW', dtype=dt, format='CHW')
        assert tuple(chw.shape) == (est.shape[0], 3) + tuple(est.shape[-2:]) and torch.equal(chw, hwc.permute(0, 3, 1, 2))
        e_hwc = vz.flow_err_to_color(est, gt, layout='CHW', dtype=dt)
        e_chw = vz.flow_err_to_color(est, gt, layout='CHW', dtype=dt, format='CHW')
        assert torch.equal(e_chw, e_hwc.permute(0, 3, 1, 2))
    e8 = vz.flow_err_to_color(est, gt, layout='CHW', dtype=torch.uint8).cpu().numpy()
    assert np.array_equal(e8, R.q8(vz.flow_err_to_color(est, gt, layout='CHW').cpu().numpy()))
    fr = vz.render_flow_frame(est, gt, format='CHW')
    assert fr['flow_color'].dtype == torch.uint8 and tuple(fr['flow_color'].shape) == (est.shape[0], 3, 2 * est.shape[-2], est.shape[-1])


# ------------------------------------------------------------------------------------------------------------------- class maps
def class_of(img):
    """colours [..., 3] -> class index, -1 for black; every colour must be a table entry, bit for bit"""
    table = np.concatenate([R.CLASS_RGB / np.float32(255), np.zeros((1, 3), dtype=np.float32)])
    idx = np.abs(img[..., None, :] - table).sum(axis=-1).argmin(axis=-1)
    assert np.array_equal(table[idx], img), "a colour that is not in the class table"
    return np.where(idx == 10, -1, idx).astype(np.int8)


@pytest.mark.parametrize("name", ["dense", "sparse", "none_valid", "nonfinite", "ragged", "tiny1", "tiny35", "rescaled"])
def test_error_class_maps_are_the_references(name):
    g = load(name)
    est, gt = g["est_d"], g["gt_d"]
    if name == "rescaled":
        got = class_of(vz.render_flow_frame(est, gt, outputs=('error_map',), dtype=torch.float32)['error_map'].cpu().numpy())
        tie = g["tie_class"]
        assert tie.mean() <= 0.005 and np.array_equal(got[~tie], g["class_idx"][~tie])
        assert (np.abs(got.astype(int) - g["class_idx"])[tie] <= 1).all()
    else:
        got = class_of(vz.flow_err_to_color(est, gt, layout='CHW').cpu().numpy())
        assert np.array_equal(got, g["class_idx"]), name
    if name == "dense":                                   # E exactly 0.1875, 3.0 and 48.0: the later class wins the end point
        assert got[0, 5, 10:13].tolist() == [1, 5, 9]
    counts = vz.flow_class_counts(vz.flow_render_stats(est, gt)).cpu().numpy()
    assert counts.dtype == np.int32 and np.array_equal(counts, R.class_counts(got)), name
    if "class_val_idx" in g:
        for val in (g["gt_val_half"].astype(np.float32) / np.float32(2), g["gt_val_half"] > 0):
            want = g["class_val_idx"] if val.dtype != bool else R.err_class(g["est"], g["gt"], val)
            got = class_of(vz.flow_err_to_color(est, gt, d(val), layout='CHW').cpu().numpy())
            assert np.array_equal(got, want)
        val = d(g["gt_val_half"].astype(np.float32) / np.float32(2))
        counts = vz.flow_class_counts(vz.flow_render_stats(est, gt, valid=val)).cpu().numpy()
        assert np.array_equal(counts, R.class_counts(g["class_val_idx"]))

# ----------------------------------------------------------------------------------------------------------------------- decode
def test_kitti_decode_both_layouts():
    g = dict(np.load(os.path.join(R.GOLDEN, "flow_frame_kitti.npz")))
    raw = torch.from_numpy(g["raw"].view(np.int16)).to(DEV)
    flow, valid = pp.decode_kitti_flow(raw)
    assert flow.dtype == torch.float32 and valid.dtype == torch.bool and tuple(valid.shape) == (2, 1, 20, 31)
    assert np.array_equal(flow.cpu().numpy(), g["flow"]) and np.array_equal(valid.cpu().numpy(), g["valid"])
    f2, v2 = pp.decode_kitti_flow(raw.permute(0, 3, 1, 2).contiguous(), layout='CHW')
    assert torch.equal(f2, flow) and torch.equal(v2, valid)
    f1, v1 = pp.decode_kitti_flow(raw[1])
    assert torch.equal(f1, flow[1]) and torch.equal(v1, valid[1])
    if hasattr(torch, "uint16"):
        f3, _ = pp.decode_kitti_flow(raw.view(torch.uint16))
        assert torch.equal(f3, flow)
    sl = raw[:, :, 1:].contiguous()                        # 30 columns: rows that start off the 8-byte grid
    f4, v4 = pp.decode_kitti_flow(sl)
    assert torch.equal(f4, flow[..., 1:]) and torch.equal(v4, valid[..., 1:])


# ------------------------------------------------------------------------------------------------------------------ consistency
@pytest.mark.parametrize("name", ["nonfinite", "batch3", "ragged"])
def test_consistency_runs_images_and_layouts(name):
    g = load(name)
    est, gt = g["est_d"], g["gt_d"]
    keep_e, keep_g = est.clone(), gt.clone()
    B = est.shape[0]
    as_bits = lambda t: t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t

    def everything(e, t, layout):
        out = dict(vz.render_flow_frame(e, t, dtype=torch.float32, layout=layout))
        out['own'] = vz.flow_to_color(e, layout=layout)
        out['rad'] = vz.flow_max_rad(e, layout=layout)
        out['stats'] = vz.flow_render_stats(e, t, layout=layout)
        if layout == 'CHW':
            out['metrics'] = ev._flow_metrics([e], t, 0.0, 400, True)
        return out
    a, b = everything(est, gt, 'CHW'), everything(est, gt, 'CHW')
    for k in a:
        assert torch.equal(as_bits(a[k]), as_bits(b[k])), (name, k, "two calls differ")
    # image i alone is image i of the batch (the maximum is per image)
    for i in range(B):
        one = everything(est[i:i + 1].contiguous(), gt[i:i + 1].contiguous(), 'CHW')
        for k in ('flow_color', 'error_map', 'own', 'rad', 'stats'):
            assert torch.equal(as_bits(one[k]), as_bits(a[k][i:i + 1])), (name, k, i)
    # the reference's [B,H,W,2] layout, read in place
    c = everything(est.permute(0, 2, 3, 1).contiguous(), gt.permute(0, 2, 3, 1).contiguous(), 'HWC')
    for k in c:
        assert torch.equal(as_bits(c[k]), as_bits(a[k])), (name, k, "HWC input differs from CHW input")
    assert torch.equal(as_bits(vz.flow_color(est, layout='CHW')), as_bits(a['own']))
    # render_flow_frame is the drop-ins one by one; without a ground truth: the estimate with its own maximum
    assert torch.equal(as_bits(a['error_map']), as_bits(vz.flow_err_to_color(est, gt, layout='CHW')))
    alone = vz.render_flow_frame(est, dtype=torch.float32)
    assert list(alone) == ['flow_color'] and torch.equal(as_bits(alone['flow_color']), as_bits(a['own']))
    H = est.shape[-2]
    shared = a['stats'][:, 2].contiguous()
    tau = float(g["tau_rad"])
    for part, m in ((a['flow_color'][:, :H], est), (a['flow_color'][:, H:], gt)):
        given = vz.flow_to_color(m, max_rad=shared, layout='CHW')
        hw = R.hwc(m.cpu().numpy())
        far = np.stack([np.abs(R.norm_radius(hw[i], shared[i].item()).astype(np.float64) - 1.0) > tau for i in range(B)])
        assert np.array_equal(part.cpu().numpy()[far], given.cpu().numpy()[far]), (name, "shared maximum vs the same maximum given")
    # inputs are never modified (the reference zeroes unknown pixels in the caller's array)
    assert torch.equal(as_bits(est), as_bits(keep_e)) and torch.equal(as_bits(gt), as_bits(keep_g))


def test_recorded_plan_replays():
    g = load("rescaled")
    est, gt = g["est_d"].clone(), g["gt_d"].clone()
    raw = torch.from_numpy(dict(np.load(os.path.join(R.GOLDEN, "flow_frame_kitti.npz")))["raw"].view(np.int16)).to(DEV)
    vz._wheel(DEV)                                          # the table's upload is not part of a plan
    with _lib.Recorder() as rec:
        pics = vz.render_flow_frame(est, gt)
        met = ev.flow_validation_metrics([est, est], gt)
        flow, valid = pp.decode_kitti_flow(raw)
    assert [n for n, _ in rec.log] == ["ts_flow_render_fwd", "ts_flow_metrics_fwd", "ts_flow_u16_decode_fwd"]
    before = {k: v.clone() for k, v in list(pics.items()) + list(met.items())}
    est.mul_(1.5)
    rec.run()
    fresh = dict(vz.render_flow_frame(est, gt))
    fresh.update(ev.flow_validation_metrics([est, est], gt))
    torch.cuda.synchronize()
    now = dict(pics)
    now.update(met)
    for k in fresh:
        assert torch.equal(now[k], fresh[k]), k
    assert not torch.equal(before['flow_color'], now['flow_color'])
    assert not torch.equal(before['metric_flow_0/all_epe'], now['metric_flow_0/all_epe'])


# -------------------------------------------------------------------------------------------------------------------- refusals
def test_refusals():
    g = load("tiny35")
    est, gt = g["est_d"], g["gt_d"]
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        ev.flow_calc_error(est.cpu(), gt.cpu())
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        vz.flow_err_to_color(est, gt.cpu(), layout='CHW')
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        vz.flow_to_color(est, max_rad=torch.ones(2), layout='CHW')
    three = torch.zeros(2, 3, 3, 5, device=DEV)
    with pytest.raises(ValueError):
        ev.flow_calc_error(three, three)                                  # channel count other than 2
    with pytest.raises(ValueError):
        vz.flow_to_color(three, layout='CHW')
    with pytest.raises(ValueError):
        vz.flow_to_color(est)                                             # [B,2,H,W] read as HWC: the last axis is not 2
    with pytest.raises(ValueError):
        ev.flow_calc_error(est, gt[..., :-1])                             # mismatched shapes
    with pytest.raises(ValueError):
        vz.flow_err_to_color(est, gt[..., :-1].contiguous(), layout='CHW')
    with pytest.raises(ValueError):
        ev.flow_validation_metrics([est[:1]], gt)                         # batch 1 against 2
    with pytest.raises(ValueError):
        ev._flow_metrics([est] * 5, gt, 0.0, 400, False)                  # more than four levels per call
    with pytest.raises(ValueError):
        ev._flow_metrics([], gt, 0.0, 400, False)
    with pytest.raises(ValueError):
        vz.flow_to_color(est, max_rad=torch.ones(3, device=DEV), layout='CHW')      # a maximum per image: 2
    with pytest.raises(ValueError):
        vz.flow_err_to_color(est, gt, torch.ones(2, 3, 4, device=DEV), layout='CHW')
    with pytest.raises(ValueError):
        vz.render_flow_frame(est, outputs=('error_map',))
    with pytest.raises(ValueError):
        vz.render_flow_frame(est, gt, size=(4, 4))
    with pytest.raises(TypeError):
        pp.decode_kitti_flow(torch.zeros(3, 5, 3, device=DEV))
    with pytest.raises(ValueError):
        pp.decode_kitti_flow(torch.zeros(3, 5, 2, device=DEV, dtype=torch.int16))
    assert len(ev.flow_validation_metrics([est] * 6, gt)) == 30          # six levels: two launch pairs
    L = _lib.lib()
    out = torch.empty((4, 5), device=DEV)
    ws = torch.empty(int(L.ts_flow_metrics_workspace_bytes(2, 3, 5)), device=DEV, dtype=torch.uint8)
    args = lambda n: [_lib.ptr(est)] * 4 + [n] + [3, 5] * 4 + [_lib.ptr(gt), 2, 3, 5, 0.0, 400.0, 0, _lib.ptr(out), _lib.ptr(ws), None]
    assert L.ts_flow_metrics_fwd(*args(0)) == -2 and L.ts_flow_metrics_fwd(*args(5)) == -2
    assert L.ts_flow_metrics_fwd(*args(1)) == 0
    torch.cuda.synchronize()
