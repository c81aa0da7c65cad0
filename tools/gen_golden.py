#!/usr/bin/env python
"""Generate tests/golden/*.npz by running the REAL reference (imported from /root/reference).

Run in the build container only:   PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden.py
The reference source never leaves /root/reference; only inputs / expected outputs are saved.
Inputs that are cheap to regenerate are stored as seeds (tests/synth.py) instead of bytes.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import ref_import  # noqa: E402
import synth  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")
T = torch.from_numpy


def save(name, **arrs):
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **{k: (v.detach().cpu().numpy() if torch.is_tensor(v) else np.asarray(v))
                                 for k, v in arrs.items()})
    print("wrote %-38s %8.1f KB" % (name + ".npz", os.path.getsize(path) / 1024))


# ----------------------------------------------------------------------------------------------
def functional_cases(M):
    from architecture.modeling.aggregation.utils.block_cost import block_cost
    from architecture.modeling.layers import inverse_warp_3d, project_to_3d
    from architecture.modeling.prediction.soft_argmin import SOFTARGMIN
    from architecture.modeling.prediction.argmin import ARGMIN
    from architecture.modeling.aggregation.TemporalStereo.coarse import CoarseAggregation

    seed = synth.SEED0
    # K1a integer path ---------------------------------------------------------------------
    for i, (B, C, H, W, D) in enumerate([(2, 16, 10, 14, 3), (1, 8, 8, 12, 5), (1, 8, 9, 13, 4)]):
        L = synth.normal(seed + i, "bcL", (B, C, H, W))
        R = synth.normal(seed + i, "bcR", (B, C, H, W))
        out = block_cost(T(L), T(R), D, block_cost_scale=3)
        save("block_cost_int_%d" % i, left=L, right=R, num_disp=D, scales=3, out=out)
    # K1b sampled path ---------------------------------------------------------------------
    for i, (B, C, H, W, D) in enumerate([(2, 16, 10, 14, 5), (1, 8, 8, 12, 3), (1, 8, 9, 13, 6)]):
        L = synth.normal(seed + 10 + i, "bcL", (B, C, H, W))
        R = synth.normal(seed + 10 + i, "bcR", (B, C, H, W))
        disp = synth.uniform(seed + 10 + i, "bcD", (B, D, H, W), -3.0, W + 2.0)
        disp[:, 0] = np.round(disp[:, 0])            # exact-integer candidates
        disp[:, 1, :, : W // 2] = 0.0                # zero shift
        out = block_cost(T(L), T(R), T(disp), block_cost_scale=3)
        save("block_cost_sampled_%d" % i, left=L, right=R, disp=disp, scales=3, out=out)
    # scale count 1 and 2
    L = synth.normal(seed + 20, "bcL", (1, 8, 8, 12)); R = synth.normal(seed + 20, "bcR", (1, 8, 8, 12))
    disp = synth.uniform(seed + 20, "bcD", (1, 4, 8, 12), 0.0, 6.0)
    for sc in (1, 2):
        save("block_cost_sampled_scale%d" % sc, left=L, right=R, disp=disp, scales=sc,
             out=block_cost(T(L), T(R), T(disp), block_cost_scale=sc))
        save("block_cost_int_scale%d" % sc, left=L, right=R, num_disp=4, scales=sc,
             out=block_cost(T(L), T(R), 4, block_cost_scale=sc))
    # the reference-authored 3x4 "value test" inputs (cat_fms.py:48-57 / dif_fms.py:56-65)
    H, W = 3, 4
    left = torch.linspace(1, H * W, H * W).reshape(1, 1, H, W)
    right = torch.linspace(H * W + 1, H * W * 2, H * W).reshape(1, 1, H, W)
    ds = torch.linspace(-2, 2, 5).repeat(1, H, W, 1).permute(0, 3, 1, 2).contiguous()
    save("value_test_warp", left=left, right=right, disp=ds, warped=inverse_warp_3d(right, -ds, padding_mode='zeros'))
    # K2a geometry --------------------------------------------------------------------------
    B, C, H, W = 2, 3, 6, 8
    depth = synth.uniform(seed + 30, "depth", (B, C, H, W), 1.0, 20.0)
    K = synth.sceneflow_intrinsics(B, 48, 64)
    K[:, 0] /= 8.0; K[:, 1] /= 8.0
    Tm = synth.small_motion(seed + 30, B)
    o = project_to_3d(T(depth), T(K), torch.inverse(T(K)), T(Tm))
    save("project_to_3d", depth=depth, K=K, T=Tm, triangular_depth=o['triangular_depth'],
         optical_flow=o['optical_flow'], flow_mask=o['flow_mask'], src_pixel_coord=o['src_pixel_coord'])
    o3 = project_to_3d(T(depth), T(K[:, :3, :3].copy()), None, T(Tm))
    save("project_to_3d_k3", depth=depth, K=K[:, :3, :3], T=Tm, triangular_depth=o3['triangular_depth'],
         optical_flow=o3['optical_flow'])
    # K4 regression -------------------------------------------------------------------------
    B, D, H, W = 2, 14, 6, 9
    cost = synth.normal(seed + 40, "cost", (B, D, H, W))
    samp = np.sort(synth.uniform(seed + 40, "samp", (B, D, H, W), 0, 30), axis=1)
    off = synth.uniform(seed + 40, "off", (B, D, H, W), -1, 1)
    tiny = CoarseAggregation(in_planes=8, C=8, num_sample=2)
    d, td, tc = tiny.predict_disp(T(cost), T(samp), T(off), k=2)
    save("topk_softargmax", cost=cost, samp=samp, off=off, disp=d, topk_disp=td, topk_cost=tc)
    d3, td3, tc3 = tiny.predict_disp(T(cost), T(samp), T(off), k=3)
    save("topk_softargmax_k3", cost=cost, samp=samp, off=off, disp=d3, topk_disp=td3, topk_cost=tc3)
    Dd = 48
    cost = synth.normal(seed + 41, "cost", (1, Dd, 5, 7), 3.0)
    samp = np.broadcast_to(np.arange(Dd, dtype=np.float32).reshape(1, Dd, 1, 1), (1, Dd, 5, 7)).copy()
    save("soft_argmin", cost=cost, samp=samp,
         disp=SOFTARGMIN(temperature=1.0, normalize=True)(T(cost), T(samp)),
         disp_t2=SOFTARGMIN(temperature=2.0, normalize=True)(T(cost), T(samp)),
         disp_argmin=ARGMIN(dim=1)(T(cost), T(samp)))


# ----------------------------------------------------------------------------------------------
def sibling_cases(M):
    """Dense siblings of block_cost: cat_fms / dif_fms."""
    from architecture.modeling.aggregation.utils.cat_fms import cat_fms
    from architecture.modeling.aggregation.utils.dif_fms import dif_fms
    seed = synth.SEED0 + 60
    # the reference-authored 3x4 value test (cat_fms.py:48-69, dif_fms.py:56-76): shifts -2..2
    H, W = 3, 4
    left = torch.linspace(1, H * W, H * W).reshape(1, 1, H, W)
    right = torch.linspace(H * W + 1, H * W * 2, H * W).reshape(1, 1, H, W)
    ds = torch.linspace(-2, 2, 5).repeat(1, H, W, 1).permute(0, 3, 1, 2).contiguous()
    save("fms_value_test", left=left, right=right, disp=ds, cat=cat_fms(left, right, ds), dif=dif_fms(left, right, ds))
    for i, (B, C, H, W, D, lo, hi) in enumerate([(2, 16, 10, 14, 6, -3.0, 16.0), (1, 8, 9, 13, 4, 0.0, 6.0), (1, 24, 6, 20, 9, -1.0, 21.0)]):
        L = synth.normal(seed + i, "fmL", (B, C, H, W))
        R = synth.normal(seed + i, "fmR", (B, C, H, W))
        if i == 1:
            L, R = np.abs(L), np.abs(R)                # post-ReLU style features: the (target > 0) mask is then the in-frame mask
        disp = synth.uniform(seed + i, "fmD", (B, D, H, W), lo, hi)
        disp[:, 0] = np.round(disp[:, 0])
        if i == 2:                                   # the dense use: integer candidates 0..D-1
            disp = np.broadcast_to(np.arange(D, dtype=np.float32).reshape(1, D, 1, 1), (B, D, H, W)).copy()
        save("fms_%d" % i, left=L, right=R, disp=disp, cat=cat_fms(T(L), T(R), T(disp)), dif=dif_fms(T(L), T(R), T(disp)))


# ----------------------------------------------------------------------------------------------
def build_reference_aggregator(dims):
    from architecture.modeling.aggregation.TemporalStereo.TemporalStereo import TEMPORALSTEREO
    from architecture.modeling.aggregation.TemporalStereo.coarse import CoarseAggregation
    from architecture.modeling.aggregation.TemporalStereo.fine import FineAggregation
    from architecture.modeling.aggregation.TemporalStereo.precise import PreciseAggregation
    c, f, p = dims['coarse'], dims['fine'], dims['precise']
    net = TEMPORALSTEREO(
        coarse=CoarseAggregation(in_planes=c['in_planes'], C=c['C'], num_sample=c['num_sample'], topk=2),
        fine=FineAggregation(in_planes=f['in_planes'], C=f['C'], num_sample=5, topk=2),
        precise=PreciseAggregation(in_planes=p['in_planes'], C=p['C'], num_sample=5, topk=2),
    )
    return net


def load_synth_weights(net, seed):
    shapes = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    import json
    tag = "x".join(str(v.shape[0]) for k, v in net.state_dict().items() if k.endswith("init3d.0.conv.0.weight"))
    with open(os.path.join(OUT, "state_shapes_%s.json" % tag), "w") as fh:
        json.dump({k: list(v) for k, v in shapes.items()}, fh, indent=0, sort_keys=True)
    vals = synth.state_values(shapes, seed)
    net.load_state_dict({k: T(v) for k, v in vals.items()}, strict=True)
    return shapes


class Recorder:
    """Records block_cost outputs and the permutations torch.sort produced inside the reference."""

    def __init__(self):
        self.raw, self.orders = [], []

    def __enter__(self):
        import architecture.modeling.aggregation.TemporalStereo.coarse as c
        import architecture.modeling.aggregation.TemporalStereo.fine as f
        import architecture.modeling.aggregation.TemporalStereo.precise as p
        self.mods = (c, f, p)
        self.orig_bc = c.block_cost
        self.orig_sort = torch.sort

        def bc(*a, **k):
            out = self.orig_bc(*a, **k)
            self.raw.append(out)
            return out

        def sort(x, *a, **k):
            r = self.orig_sort(x, *a, **k)
            self.orders.append(r[1])
            return r
        for m in self.mods:
            m.block_cost = bc
        torch.sort = sort
        return self

    def __exit__(self, *exc):
        for m in self.mods:
            m.block_cost = self.orig_bc
        torch.sort = self.orig_sort


TINY = dict(coarse=dict(in_planes=32, C=8, num_sample=4), fine=dict(in_planes=16, C=8),
            precise=dict(in_planes=8, C=8))
SCENEFLOW = dict(coarse=dict(in_planes=256, C=32, num_sample=12), fine=dict(in_planes=128, C=16),
                 precise=dict(in_planes=64, C=8))


def synthetic_prev_info(seed, B, H, W, local_maps=2):
    """A plausible temporal state at 1/8 resolution (what update_map would hand over)."""
    h, w = H // 8, W // 8
    base = synth.uniform(seed, "mem_base", (B, 1, h, w), 1.0, 6.0)
    ds = np.concatenate([base + 0.3, base - 0.4], axis=1).astype(np.float32)
    cv = synth.normal(seed, "mem_cost", (B, 2, h, w))
    lm = np.concatenate([base * 1.02 + 0.1 * k for k in range(local_maps)], axis=1).astype(np.float32)
    return ds, cv, lm


def aggregator_case(name, dims, seed, B, H, W, temporal, store_inputs, training=False):
    net = build_reference_aggregator(dims)
    load_synth_weights(net, seed)
    chans = (dims['precise']['in_planes'], dims['fine']['in_planes'], dims['coarse']['in_planes'])
    lf, rf = synth.feature_pyramid(seed, B, H, W, chans=chans)
    il, ir = synth.images(seed, B, H, W)
    prev = {}
    extra = {}
    if temporal:
        ds, cv, lm = synthetic_prev_info(seed, B, H, W)
        prev = {'cost_memory': {'disp_sample': T(ds), 'cost_volume': T(cv)}, 'use_past_cost': True,
                'local_map': T(lm), 'local_map_size': lm.shape[1]}
        extra.update(mem_disp_sample=ds, mem_cost_volume=cv, local_map=lm)
    bn_stats = {}
    if not training:
        # give the synthetic network BatchNorm statistics that match its activations (as a trained
        # network has): one calibration pass in train mode with momentum 1, then eval.
        bns = [m for m in net.modules() if isinstance(m, (torch.nn.BatchNorm2d, torch.nn.BatchNorm3d))]
        for m in bns:
            m.momentum = 1.0
        net.train(True)
        with torch.no_grad():
            net([T(x) for x in lf], [T(x) for x in rf], T(il), T(ir), dict(prev))
        for m in bns:
            m.momentum = 0.1
        bn_stats = {"bn::" + k: v.clone() for k, v in net.state_dict().items()
                    if k.endswith("running_mean") or k.endswith("running_var")}
    net.train(training)
    with torch.no_grad(), Recorder() as rec:
        disps, costs, samples, offs, ranges, info = net([T(x) for x in lf], [T(x) for x in rf], T(il), T(ir), prev)
    arrs = dict(seed=seed, B=B, H=H, W=W, temporal=int(temporal), training=int(training),
                dims=np.array([dims['coarse']['in_planes'], dims['coarse']['C'], dims['coarse']['num_sample'],
                               dims['fine']['in_planes'], dims['fine']['C'],
                               dims['precise']['in_planes'], dims['precise']['C']]))
    arrs.update(extra)
    arrs.update(bn_stats)
    if store_inputs:     # cross-check that synth regenerates the same bytes on the test side
        arrs.update(l16_probe=lf[2][:, :2], r16_probe=rf[2][:, :2])
        for i, nm in enumerate(("full", "precise", "fine_up", "coarse_up")):
            arrs["disp_" + nm] = disps[i]
        for i, nm in enumerate(("precise", "fine", "coarse")):
            arrs["cost_" + nm] = costs[i]
            arrs["samp_" + nm] = samples[i]
            arrs["off_" + nm] = offs[i]
        arrs.update(coarse_raw_b0=rec.raw[0][:1], fine_raw_b0=rec.raw[1][:1],
                    coarse_order=rec.orders[0].to(torch.int16), fine_order=rec.orders[1].to(torch.int16),
                    range_fine_low=ranges[0]['low'], range_coarse_low=ranges[1]['low'])
    else:                # big case: outputs only, full-res map sub-sampled
        arrs.update(disp_full_sub4=disps[0][:, :, ::4, ::4], disp_precise=disps[1], disp_fine_up=disps[2],
                    disp_coarse_up=disps[3], cost_coarse=costs[2], samp_fine=samples[1],
                    disp_full_mean=disps[0].double().mean(), disp_full_absmean=disps[0].double().abs().mean())
    arrs.update(prev_disp_sub=info['prev_disp'][:, :, ::4, ::4],
                mem_out_disp_sample=info['cost_memory']['disp_sample'],
                mem_out_cost_volume=info['cost_memory']['cost_volume'])
    save(name, **arrs)


def reference_update_map():
    """The reference's OWN `update_map` (projects/TemporalStereo/TemporalStereo.py:326-461), compiled from its file's syntax tree
    (the LightningModule around it needs packages this image lacks); FunctionSoftsplat (CUDA-only) is bound to oracle.splat."""
    import ast
    import torch.nn.functional as F
    from architecture.modeling.layers import project_to_3d
    sys.path.insert(0, ROOT)
    from oracle import splat as osplat
    path = os.path.join(ref_import.REFERENCE_ROOT, "projects", "TemporalStereo", "TemporalStereo.py")
    tree = ast.parse(open(path).read(), filename=path)
    cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "TemporalStereo")
    fn = next(n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name == "update_map")
    ns = {"torch": torch, "F": F, "project_to_3d": project_to_3d, "EXPMAX": 50,
          "FunctionSoftsplat": lambda tenInput, tenFlow, tenMetric, strType: osplat.softsplat(tenInput, tenFlow, tenMetric, strType)}
    exec(compile(ast.Module(body=[fn], type_ignores=[]), path, "exec"), ns)
    return ns["update_map"]


def planted_cases(M, only=None):
    """Full-size end-to-end fixtures: the REFERENCE aggregator with the committed contractive checkpoint
    (tests/golden/ckpt_planted.npz, trained by this repository's own TrainStep: tools/train_checkpoint.py) on planted-disparity
    scenes (tests/synth.stereo_sequence) at the BASELINE configurations' stated batches, sequences driven by the reference's own
    update_map.  Stored per frame: the full-resolution disparity sub-sampled, its EPE against the planted ground truth over ALL
    pixels (float64), the 1/4-resolution disparity, and a digest of the inputs so that the test side can tell whether it
    regenerated them bit for bit."""
    import types
    import parity_tools as PT
    update_map = reference_update_map()
    ckpt = PT.load_checkpoint()
    # (fixture name, configuration, seed offset, sub-sampling of the stored full-resolution map)
    plan = [("planted_c1_s0", 0, 0, 2), ("planted_c1_s1", 0, 1, 4), ("planted_c1_s2", 0, 2, 4),
            ("planted_c2_s0", 1, 0, 4), ("planted_c3_s0", 2, 0, 8), ("planted_c4_s0", 3, 0, 4),
            # round 4: a second reference-run seed for the temporal configurations, stored more sparsely
            ("planted_c2_s1", 1, 1, 8), ("planted_c3_s1", 2, 1, 12), ("planted_c4_s1", 3, 1, 6)]
    names = list(PT.CONFIGS)
    for name, ci, k, sub in plan:
        if only and name not in only:
            continue
        c = PT.CONFIGS[names[ci]]
        seed = synth.SEED0 + 500 + 10 * ci + k
        B, H, W, frames = c["B"], c["H"], c["W"], c["frames"]
        max_disp = 16 * c["num_sample"]
        dims = dict(SCENEFLOW); dims['coarse'] = dict(SCENEFLOW['coarse'], num_sample=c["num_sample"])
        net = build_reference_aggregator(dims)
        net.load_state_dict(ckpt, strict=True)
        net.eval()
        sc = synth.stereo_sequence(seed, B, H, W, frames=frames, max_disp=max_disp, fx=c["fx"], baseline=c["baseline"])
        me = types.SimpleNamespace(with_previous=True, use_past_cost=True, local_map_size=c["n_local"])
        eye = torch.eye(4).expand(B, 4, 4).contiguous()
        arrs = dict(config=names[ci], seed=seed, B=B, H=H, W=W, frames=frames, sub=sub, max_disp=max_disp, num_sample=c["num_sample"],
                    n_local=c["n_local"], fx=c["fx"], baseline=c["baseline"])
        info = {}
        for t in range(frames):
            lf, rf, il, ir = sc["frames"][t]
            arrs["input_checksum_%d" % t] = np.float64(synth.checksum([lf, rf, il, ir]))
            if t > 0:
                batch = {"baseline": torch.full((B, 1, 1, 1), float(c["baseline"])), ("color_aug", t, "l"): torch.zeros(B, 3, H, W),
                         ("K", 0): T(sc["K"]), ("inv_T", t - 1, "l"): eye, ("T", t, "l"): T(sc["T"][t])}
                with torch.no_grad():
                    _, info = update_map(me, batch, info, t)
            with torch.no_grad():
                disps, costs, samples, offs, ranges, info = net([T(x) for x in lf], [T(x) for x in rf], T(il), T(ir), info)
            gt = T(sc["gt"][t])
            arrs["epe_%d" % t] = np.float64(PT.epe(disps[0], gt, max_disp))
            arrs["epe_quarter_%d" % t] = np.float64(PT.epe(torch.nn.functional.interpolate(disps[1] * 4, size=(H, W), mode='bilinear', align_corners=True), gt, max_disp))
            arrs["disp_full_sub_%d" % t] = disps[0][:, :, ::sub, ::sub]
            arrs["disp_precise_sub_%d" % t] = disps[1][:, :, ::max(sub // 2, 1), ::max(sub // 2, 1)]
            arrs["disp_full_mean_%d" % t] = np.float64(disps[0].double().mean())
        arrs["mem_out_disp_sample"] = info['cost_memory']['disp_sample']
        if k == 0:            # (the later seeds stay below 1 MB: the test reads the candidates only)
            arrs["mem_out_cost_volume"] = info['cost_memory']['cost_volume']
        save(name, **arrs)
        print("   ", name, "EPE per frame", [float(arrs["epe_%d" % t]) for t in range(frames)])


def planted_gradient_case(M, full_size=False):
    """full_size: the same at BASELINE configs[1]'s size (544x960, D=192, B=1), stored as norms / projections only
    (planted_train_grads_c1, < 200 KB).
    Gradient fixture of the whole aggregator: the reference's aggregator in train() mode with the
    committed checkpoint on a small planted scene, the reference's OWN loss objects with the sceneflow.yaml weights behind the
    wrapper's full-resolution rescale (projects/TemporalStereo/TemporalStereo.py:305-309), loss.backward() by the framework's
    autograd -- run twice: in float32 (what the reference computes) and in float64 (the same modules and inputs cast to double:
    the exact gradient of the same function, the arbiter where fp32 backward passes through BatchNorm lose digits to
    cancellation).  Stored for both: the loss terms, the gradients of the six feature maps (every 8th channel), the gradients of
    a list of named weights, and for EVERY parameter the gradient's norm and its projection on a seeded random direction."""
    import torch.nn.functional as F
    import parity_tools as PT
    from architecture.modeling.losses import DispSmoothL1Loss, WarssersteinDistanceLoss
    B, H, W, ns = (1, 544, 960, 12) if full_size else (2, 128, 192, 4)
    max_disp = 16 * ns
    seed = synth.SEED0 + (610 if full_size else 600)
    fx = 1050.0 if full_size else 300.0
    dims = dict(SCENEFLOW); dims['coarse'] = dict(SCENEFLOW['coarse'], num_sample=ns)
    sc = synth.stereo_sequence(seed, B, H, W, frames=1, max_disp=max_disp, fx=fx, baseline=1.0)
    arrs = dict(seed=seed, B=B, H=H, W=W, num_sample=ns, max_disp=max_disp, fx=fx,
                input_checksum=np.float64(synth.checksum(list(sc["frames"][0]))))
    for tag, dt in (("", torch.float32), ("f64::", torch.float64)):
        torch.set_default_dtype(dt)                  # the reference creates constants (candidates, zero memory) in the default dtype
        net = build_reference_aggregator(dims)
        net.load_state_dict(PT.load_checkpoint(), strict=True)
        net = net.to(dt).train()
        lf, rf, il, ir = sc["frames"][0]
        lf = [T(x).to(dt).requires_grad_(True) for x in lf]
        rf = [T(x).to(dt).requires_grad_(True) for x in rf]
        gt = T(sc["gt"][0]).to(dt)
        disps, costs, samples, offs, ranges, info = net(lf, rf, T(il).to(dt), T(ir).to(dt), {})
        full = [F.interpolate(d * W / d.shape[-1], size=(H, W), mode='bilinear', align_corners=True) for d in disps]
        l1 = DispSmoothL1Loss(max_disp=max_disp, weights=[2.0, 1.0, 0.7, 0.5])(full, gt)
        wd = WarssersteinDistanceLoss(max_disp=max_disp, global_weight=2.0, weights=[1.0, 0.7, 0.5])(costs, offs, samples, gt)
        total = sum(l1.values()) + sum(wd.values())
        total.backward()
        arrs[tag + "total"] = total.detach()
        for k, v in list(l1.items()) + list(wd.items()):
            arrs[tag + "loss::" + k] = v.detach()
        for i in range(3):          # every eighth channel in full + norm and a seeded projection of the whole tensor
            for side, ts in (("left", lf), ("right", rf)):
                g = ts[i].grad
                if not full_size:
                    arrs[tag + "g_%s_%d" % (side, i)] = g[:, ::8]
                else:       # norms and a seeded projection only
                    pr = T(synth.normal(seed, "projf%s%d" % (side, i), tuple(g.shape))).double()
                    arrs[tag + "g_%s_%d_proj" % (side, i)] = np.float64((g.double() * pr).sum())
                arrs[tag + "g_%s_%d_norm" % (side, i)] = np.float64(g.double().norm())
        named = dict(net.named_parameters())
        picks = [k for k in named if k.endswith(("init3d.0.conv.0.weight", "init3d.0.conv.0.bias", "init3d.0.conv.1.weight", "past_conv.weight",
                                                 "pred_heads.cost_head.1.weight", "pred_heads.off_head.1.weight", "pred_heads.cost_head.0.weight",
                                                 "init3d.0.conv.1.norm.weight", "init3d.0.conv.1.norm.bias", "fuse.conv_5x5.weight"))]
        picks += [k for k in named if k.startswith("precise.refinement.") and k.endswith(("deconv4.weight", "deconv2.weight", "deconv2.bias", "conv4.0.weight",
                                                                                             "deconv4.norm.weight"))]
        picks += [k for k in named if "init3d.1." in k and k.endswith(".weight") and k.startswith("fine.")][:8]
        picks += [k for k in named if "convex_upsample" in k and k.endswith(".weight") and k.startswith("coarse.")][:4]
        picks = [k for k in dict.fromkeys(picks) if named[k].grad is not None and named[k].numel() <= 40000]
        if full_size:
            picks = [k for k in picks if named[k].numel() <= 600]          # a few small tensors element by element
        arrs["picked"] = np.array(picks)
        for k in picks:
            arrs[tag + "gw::" + k] = named[k].grad
        keys = sorted(k for k in named if named[k].grad is not None)
        arrs["all_keys"] = np.array(keys)
        arrs[tag + "all_norm"] = np.array([float(named[k].grad.double().norm()) for k in keys])
        arrs[tag + "all_proj"] = np.array([float((named[k].grad.double().flatten() * T(synth.normal(seed, "proj" + k, (named[k].numel(),))).double()).sum()) for k in keys])
        arrs["no_grad_keys"] = np.array(sorted(k for k in named if named[k].grad is None))
        print("    [%s] picked" % (tag or "f32"), len(picks), "of", len(keys), "parameters with gradients; total loss", float(total.detach()))
    torch.set_default_dtype(torch.float32)
    # how far the reference's fp32 backward is from its own exact (fp64) one: the floor of any fp32 comparison
    worst = 0.0
    for k in arrs["picked"]:
        a, b = arrs["gw::" + str(k)].double(), arrs["f64::gw::" + str(k)].double()
        worst = max(worst, float((a - b).norm() / b.norm().clamp_min(1e-30)))
    print("    reference fp32 vs fp64 backward, worst relative L2 over the picked weights: %.3g" % worst)
    save("planted_train_grads_c1" if full_size else "planted_train_grads", **arrs)


def temporal_update_cases(M):
    """K2c: the reference's OWN `update_map` (projects/TemporalStereo/TemporalStereo.py:326-461) executed here.

    The method lives inside a pytorch_lightning module whose import needs packages this image lacks, so its
    function definition is taken from the reference file's syntax tree and compiled as is (nothing is copied into
    this repository; the fixture holds inputs and outputs only).  It runs against the reference's real
    project_to_3d; the one foreign piece is FunctionSoftsplat, which exists only as cupy/CUDA kernels
    (softsplat.py:252,269-270) and is bound to oracle.splat.softsplat -- so these vectors pin the glue (intrinsics
    scaling, pose composition, disparity <-> depth, metric, plane selection, state bookkeeping), not the splat
    arithmetic, which stays pinned by the analytic tests of tests/test_oracle_splat.py."""
    import types
    update_map = reference_update_map()

    cases = [  # name, B, H, W, k, local maps in, local_map_size, use_past_cost, pre-composed pose, translation scale
        ("temporal_update_0", 2, 64, 96, 2, 2, 3, True, False, 1.0),
        ("temporal_update_1", 1, 72, 120, 2, 0, 3, True, False, 6.0),      # first temporal frame: no local map yet
        ("temporal_update_2", 2, 64, 96, 2, 3, 2, True, True, 1.0),        # cropped to local_map_size, T_past_to_now given
        ("temporal_update_3", 1, 80, 104, 3, 1, 0, True, False, 1.0),      # local maps off
        ("temporal_update_4", 2, 64, 96, 2, 2, 3, False, False, 1.0),      # past cost off
    ]
    for name, B, H, W, k, n_in, size, use_past, composed, tscale in cases:
        seed = synth.SEED0 + 300 + int(name[-1])
        h, w = H // 8, W // 8
        prev_disp = synth.uniform(seed, "pd", (B, 1, H, W), 2.0, 60.0)
        base = synth.uniform(seed, "mb", (B, 1, h, w), 1.0, 12.0)
        mem_s = (base + synth.uniform(seed, "ms", (B, k, h, w), -0.5, 0.5)).astype(np.float32)
        mem_c = synth.normal(seed, "mc", (B, k, h, w))
        lm = (base * synth.uniform(seed, "lm", (B, n_in, h, w), 0.9, 1.1)).astype(np.float32) if n_in else None
        K = synth.sceneflow_intrinsics(B, H, W)
        T_now = synth.small_motion(seed, B)
        T_now[:, :3, 3] *= tscale
        inv_T_past = np.linalg.inv(synth.small_motion(seed + 50, B)).astype(np.float32)
        baseline = synth.uniform(seed, "bl", (B, 1, 1, 1), 0.3, 1.2)
        me = types.SimpleNamespace(with_previous=True, use_past_cost=use_past, local_map_size=size)
        batch = {"baseline": T(baseline), ("color_aug", 0, "l"): torch.zeros(B, 3, H, W), ("K", 0): T(K),
                 ("inv_T", -1, "l"): T(inv_T_past), ("T", 0, "l"): T(T_now)}
        info = {"prev_disp": T(prev_disp), "cost_memory": {"disp_sample": T(mem_s), "cost_volume": T(mem_c)}}
        if lm is not None:
            info["local_map"] = T(lm)
        if composed:
            info["T_past_to_now"] = torch.bmm(T(T_now), T(inv_T_past))
        with torch.no_grad():
            outs, info = update_map(me, batch, info, 0)
        arrs = dict(prev_disp=prev_disp, mem_disp_sample=mem_s, mem_cost_volume=mem_c, K=K, T_now=T_now, inv_T_past=inv_T_past,
                    baseline=baseline, full_hw=np.array([H, W]), local_map_size=size, use_past_cost=int(use_past),
                    composed=int(composed), has_local_in=int(lm is not None), has_memory_out=int(info["cost_memory"] is not None),
                    has_local_out=int(size > 0))
        if lm is not None:
            arrs["local_map_in"] = lm
        if info["cost_memory"] is not None:
            arrs["out_disp_sample"] = info["cost_memory"]["disp_sample"]
            arrs["out_cost_volume"] = info["cost_memory"]["cost_volume"]
        if size > 0:
            arrs["out_local_map"] = info["local_map"]
        save(name, **arrs)


def loss_cases(M):
    """The reference's own loss objects (architecture/modeling/losses) on seeded outputs of the path's shape: three
    cost / offset / sample levels + four disparities at native resolution, rescaled to full size the way the model wrapper
    does (projects/TemporalStereo/TemporalStereo.py:305-309) before DispSmoothL1Loss sees them.  Values and autograd gradients."""
    import torch.nn.functional as F
    from architecture.modeling.losses import DispSmoothL1Loss, WarssersteinDistanceLoss
    cases = {"loss_dense": dict(hw=(64, 128), sparse=False, zeros=0.0, max_disp=48, levels=((16, 32, 5), (8, 16, 7), (4, 8, 14))),
             "loss_sparse": dict(hw=(64, 128), sparse=True, zeros=0.7, max_disp=48, levels=((16, 32, 5), (8, 16, 8), (4, 8, 14))),
             "loss_none_valid": dict(hw=(32, 64), sparse=False, zeros=1.0, max_disp=48, levels=((8, 16, 5), (4, 8, 7))),
             "loss_ragged": dict(hw=(50, 70), sparse=False, zeros=0.1, max_disp=64, levels=((13, 18, 5), (50, 70, 3)))}
    for ci, (name, c) in enumerate(cases.items()):
        seed = synth.SEED0 + 300 + ci
        B = 2
        H, W = c["hw"]
        gt = synth.uniform(seed, "gt", (B, 1, H, W), -4.0, 1.3 * c["max_disp"])
        gt = gt * (synth.uniform(seed, "keep", (B, 1, H, W)) >= c["zeros"])
        gt_t = torch.from_numpy(gt.astype(np.float32))
        arrs = dict(gt=gt, max_disp=c["max_disp"], sparse=int(c["sparse"]), n_levels=len(c["levels"]))
        costs, offs, samps, ests = [], [], [], []
        for li, (h, w, D) in enumerate(c["levels"]):
            costs.append(torch.from_numpy(synth.normal(seed, "cost%d" % li, (B, D, h, w), 2.0)).requires_grad_(True))
            offs.append(torch.from_numpy(synth.normal(seed, "off%d" % li, (B, D, h, w), 0.3)).requires_grad_(True))
            base = synth.uniform(seed, "base%d" % li, (B, 1, h, w), 0.0, c["max_disp"] * w / W)
            samps.append(torch.from_numpy((base + np.arange(D, dtype=np.float32).reshape(1, D, 1, 1) - D / 2).astype(np.float32)).requires_grad_(True))
            ests.append(torch.from_numpy(synth.uniform(seed, "est%d" % li, (B, 1, h, w), 0.0, c["max_disp"] * w / W)).requires_grad_(True))
        ests.append(torch.from_numpy(synth.uniform(seed, "estfull", (B, 1, H, W), 0.0, float(c["max_disp"]))).requires_grad_(True))
        wl = WarssersteinDistanceLoss(max_disp=c["max_disp"], sparse=c["sparse"])
        wd = wl(costs, offs, samps, gt_t)
        sl = DispSmoothL1Loss(max_disp=c["max_disp"], sparse=c["sparse"])
        full = [F.interpolate(d * W / d.shape[-1], size=(H, W), mode='bilinear', align_corners=True) for d in ests]
        sd = sl(full, gt_t)
        total = sum(wd.values()) + sum(sd.values())
        total.backward()
        for li in range(len(c["levels"])):
            arrs.update({"cost%d" % li: costs[li], "off%d" % li: offs[li], "sample%d" % li: samps[li],
                         "wars_loss%d" % li: wd["wars_loss_lvl%d" % li],
                         "g_cost%d" % li: costs[li].grad, "g_off%d" % li: offs[li].grad, "g_sample%d" % li: samps[li].grad})
        for li in range(len(ests)):
            arrs.update({"est%d" % li: ests[li], "l1_loss%d" % li: sd["l1_loss_lvl%d" % li],
                         "g_est%d" % li: ests[li].grad if ests[li].grad is not None else torch.zeros_like(ests[li]),
                         "full%d" % li: full[li]})
        arrs["n_est"] = len(ests)
        save(name, **arrs)


def backbone_memory_cases(M):
    """SURVEY 8(f)-4, last clause: the reference's OWN `_inverted_residual_forward`
    (architecture/modeling/backbone/TemporalStereo.py:183-218).  The module imports timm, which this image lacks, so the function's
    definition is taken from the reference file's syntax tree and compiled as is (nothing is copied; the fixture holds inputs and
    outputs only).  The timm block is replaced by identities and the values sit on a 1/8 grid, so that `out - input` is EXACTLY the
    tensor the block is fed -- these vectors pin the memory plumbing, which is all there is to pin."""
    import ast
    import types
    path = os.path.join(ref_import.REFERENCE_ROOT, "architecture", "modeling", "backbone", "TemporalStereo.py")
    tree = ast.parse(open(path).read(), filename=path)
    fn = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "_inverted_residual_forward")
    ns = {"torch": torch, "drop_path": lambda x, *a, **k: x}
    exec(compile(ast.Module(body=[fn], type_ignores=[]), path, "exec"), ns)
    ref = ns["_inverted_residual_forward"]
    ident = lambda x: x
    block = types.SimpleNamespace(conv_pw=ident, bn1=ident, act1=ident, conv_dw=ident, bn2=ident, act2=ident, se=ident, conv_pwl=ident,
                                  bn3=ident, drop_path_rate=0.0, training=False)
    cases = [("feature_memory_0", 2, 24, 6, 10, 0.25, True), ("feature_memory_1", 2, 24, 6, 10, 0.25, False),
             ("feature_memory_2", 1, 10, 5, 7, 0.5, True), ("feature_memory_3", 3, 20, 4, 9, 0.125, True)]
    for name, B, C, H, W, pct, with_mem in cases:
        seed = synth.SEED0 + 400 + int(name[-1])
        grid = lambda tag, shape: (np.round(synth.uniform(seed, tag, shape, -8.0, 8.0) * 8.0) / 8.0).astype(np.float32)
        x = grid("x", (B, C, H, W))
        mc = int(C * pct)
        mem = grid("m", (B, mc, H, W)) if with_mem else None
        with torch.no_grad():
            out, new_mem = ref(block, T(x), T(mem) if mem is not None else None, pct)
        arrs = dict(input=x, memory_percent=np.float64(pct), has_memory=int(with_mem), out=out.numpy(), new_memory=new_mem.numpy())
        if mem is not None:
            arrs["memory"] = mem
        save(name, **arrs)


def _reference_evaluation():
    """The reference's calc_error / do_evaluation / do_occlusion_evaluation (architecture/data/evaluation).  The package's
    __init__ imports the dataset readers (cv2 and more, absent from this image), so pixel_error.py is loaded by file path and
    eval.py's two functions are taken from its syntax tree and compiled as they are (nothing is copied)."""
    import ast
    import importlib.util
    import warnings
    from architecture.modeling.layers import inverse_warp
    base = os.path.join(ref_import.REFERENCE_ROOT, "architecture", "data", "evaluation")
    spec = importlib.util.spec_from_file_location("_ref_pixel_error", os.path.join(base, "pixel_error.py"))
    pe = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(pe)
    path = os.path.join(base, "eval.py")
    tree = ast.parse(open(path).read(), filename=path)
    fns = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in ("do_evaluation", "do_occlusion_evaluation")]
    ns = {"torch": torch, "warnings": warnings, "inverse_warp": inverse_warp, "calc_error": pe.calc_error}
    exec(compile(ast.Module(body=fns, type_ignores=[]), path, "exec"), ns)
    return pe.calc_error, ns["do_evaluation"], ns["do_occlusion_evaluation"], inverse_warp


EVAL_KEYS = ('1px', '2px', '3px', '5px', 'epe')
EVAL_MARGIN = 1e-3


def eval_cases(M):
    """Disparity evaluation (validation_step / test_step, projects/TemporalStereo/TemporalStereo.py:170-214): the reference's own
    calc_error, do_evaluation and do_occlusion_evaluation on seeded ground truths and estimates, and log_metric (:463-486) composed
    from them after validation_step's F.interpolate (:183), with LightningModule (pytorch_lightning) left out.

    Inputs are stored compactly: gt_left / gt_right as int16 in units of 1/128 px, the full-resolution estimate as gt_left plus an
    int8 offset in units of 1/16 px, shifted by 1/32 (so its error is never an integer), the low-resolution levels as float32.
    gt_left is then nudged (deterministically, in steps of 3/128, never a zero hole of a sparse map) until no pixel is within
    1e-3 of a decision threshold of any quantity that is computed rather than read: |e| vs 1/2/3/5 of every level and every
    valid pixel, |warp - gt| vs 1 and |warp| vs 1e-6 (an exact 0 is exact), gt vs lb/ub (an exact 0 hole is exact).  The
    smallest margin achieved is stored as `margin`."""
    import torch.nn.functional as F
    calc_error, do_evaluation, do_occlusion_evaluation, inverse_warp = _reference_evaluation()
    q = lambda hw: [hw, (hw[0] // 4, hw[1] // 4), (hw[0] // 4, hw[1] // 4), (hw[0] // 8, hw[1] // 8)]
    cases = {"eval_dense": dict(hw=(64, 128), lb=0, ub=192, sparse=0.0, band=False, out_of_range=True),
             "eval_sparse": dict(hw=(64, 128), lb=0, ub=192, sparse=0.6, band=False),
             "eval_none_valid": dict(hw=(64, 128), lb=0, ub=192, sparse=1.0, band=False),
             "eval_no_bounds": dict(hw=(64, 128), lb=None, ub=None, sparse=0.0, band=True),
             "eval_ragged": dict(hw=(50, 70), lb=0, ub=192, sparse=0.0, band=True, levels=[(50, 70), (13, 18), (13, 18), (7, 9)]),
             "eval_nonfinite": dict(hw=(64, 128), lb=0, ub=192, sparse=0.0, band=False, nonfinite=True),
             "eval_occlusion": dict(hw=(64, 128), lb=0, ub=192, sparse=0.0, band=True)}
    for ci, (name, c) in enumerate(cases.items()):
        seed = synth.SEED0 + 500 + ci
        B = 2
        H, W = c["hw"]
        levels = c.get("levels", q((H, W)))
        lb, ub = c["lb"], c["ub"]
        # a smooth left disparity, and the right view's disparity consistent with it (x_r = x_l - d(x_l), by fixed point)
        ph = synth.uniform(seed, "phase", (B, 1, 1, 1), 0.0, 6.283)
        yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
        d = lambda y, x: 9.0 + 5.0 * y / H + 3.0 * np.sin(2 * np.pi * x / W + ph) + 1.5 * np.cos(2 * np.pi * y / H + 0.5 * ph)
        dl = d(yy, xx)
        xl = xx + d(yy, xx)
        for _ in range(30):
            xl = xx + d(yy, xl)
        dr = d(yy, xl)
        if c["band"]:       # a foreground object seen only in the right view: the left pixels that land on it are occluded
            x0 = W // 3
            dr[..., :, x0:x0 + max(4, W // 8)] += 15.0
        if c.get("out_of_range"):
            r = synth.uniform(seed, "oor", (B, 1, H, W))
            dl = np.where(r < 0.03, 200.0, np.where(r > 0.97, -1.0, dl))
        ql = np.round(dl * 128).astype(np.int64)
        qr = np.round(dr * 128).astype(np.int64)
        if c["sparse"] > 0:
            ql = ql * (synth.uniform(seed, "keepl", (B, 1, H, W)) >= c["sparse"])
            # the right map's holes are whole columns: inverse_warp's Y round trip can land a hair off the row (a tap weight
            # of ~1e-7 on the next row), which next to a hole in the row itself would put |warp| at ~1e-6, on the threshold
            qr = qr * (synth.uniform(seed, "keepr", (B, 1, 1, W)) >= c["sparse"])
        ql = ql.astype(np.int16)
        qr = qr.astype(np.int16)
        off = np.clip(np.round(synth.normal(seed, "off", (B, 1, H, W), 40.0)), -127, 126).astype(np.int8)
        lows = [synth.normal(seed, "noise%d" % li, (B, 1, h, w), 2.0 * w / W) for li, (h, w) in enumerate(levels[1:], 1)]
        nonfinite = np.array([-1, -1], dtype=np.int64)
        if c.get("nonfinite"):
            nonfinite = np.array([(0 * H + 10) * W + 20, ((1 * 1) * H + 30) * W + 50], dtype=np.int64)   # NaN at [0,0,10,20], inf at [1,0,30,50]

        def inputs(ql):
            gl = ql.astype(np.float32) / np.float32(128)
            gr = qr.astype(np.float32) / np.float32(128)
            e0 = gl + (off.astype(np.float32) + np.float32(0.5)) / np.float32(16)
            if nonfinite[0] >= 0:
                e0.reshape(-1)[nonfinite[0]] = np.nan
                e0.reshape(-1)[nonfinite[1]] = np.inf
            ests = [e0]
            for li, (h, w) in enumerate(levels[1:], 1):
                iy = (np.arange(h) * H) // h
                ix = (np.arange(w) * W) // w
                ests.append((gl[:, :, iy][:, :, :, ix] * np.float32(w / W) + lows[li - 1]).astype(np.float32))
            return gl, gr, ests

        def margins(gl, gr, ests):
            g, gtr = T(gl), T(gr)
            full = [F.interpolate(T(e) * W / e.shape[-1], size=(H, W), mode='bilinear', align_corners=True) for e in ests]
            valid = torch.ones_like(g, dtype=torch.bool)
            if lb is not None:
                valid &= g > lb
            if ub is not None:
                valid &= g < ub
            relevant = valid if (lb is not None and lb >= 0) else torch.ones_like(valid)
            m = torch.full_like(g, np.inf)
            for f in full:
                a = (g - f).abs()
                for t in (1, 2, 3, 5):
                    m = torch.where(valid & torch.isfinite(a), torch.minimum(m, (a - t).abs()), m)
            warp = inverse_warp(gtr.clone(), -g.clone(), mode='disparity')
            m = torch.where(relevant, torch.minimum(m, ((warp - g).abs() - 1.0).abs()), m)
            m = torch.where(relevant & (warp != 0), torch.minimum(m, (warp.abs() - 1e-6).abs()), m)
            for bnd in (lb, ub):
                if bnd is not None:
                    m = torch.where(g != 0, torch.minimum(m, (g - bnd).abs()), m)
            occ = ((warp - g).abs() > 1.0) | (warp.abs() < 1e-6)
            return m, full, occ, valid

        for it in range(200):
            gl, gr, ests = inputs(ql)
            m, full, occ, valid = margins(gl, gr, ests)
            bad = (m < EVAL_MARGIN).numpy() & (ql != 0)
            if not bad.any():
                break
            ql = np.where(bad, ql + 3, ql).astype(np.int16)
        margin = float(m.min()) if torch.isfinite(m.min()) else 1e9
        if margin < EVAL_MARGIN:
            idx = np.argwhere((m < EVAL_MARGIN).numpy())
            print("BAD", name, idx[:5].tolist(), [float(m[tuple(i)]) for i in idx[:5]], [int(ql[tuple(i)]) for i in idx[:5]])
        assert margin >= EVAL_MARGIN, (name, margin)
        g, gtr, e0 = T(gl), T(gr), T(ests[0])
        stack = lambda dct, prefix='': np.array([float(dct[prefix + k]) for k in EVAL_KEYS], dtype=np.float32)
        ce = calc_error(e0, g, lb=lb, ub=ub)
        de = do_evaluation(e0, g, lb, ub)
        oe = do_occlusion_evaluation(e0, g, gtr, lb, ub)
        # log_metric after validation_step's resize (TemporalStereo.py:183, :463-486), VAL.EVAL_DISPARITY_IDS = [0, 1, 2, 3]
        whole = {}
        for i in range(len(full)):
            for k, v in do_evaluation(full[i], g, lb, ub).items():
                whole['metric_disparity_{}/all_'.format(i) + k] = v
            for k, v in do_occlusion_evaluation(full[i], g, gtr, lb, ub).items():
                whole['metric_disparity_{}/'.format(i) + k] = v
        lm = np.array([[[float(whole['metric_disparity_{}/{}_{}'.format(i, s, k)]) for k in EVAL_KEYS] for s in ("all", "occ", "noc")]
                       for i in range(len(full))], dtype=np.float32)
        gm = lambda mask: int((mask & (((g * mask) > lb) if lb is not None else True) & (((g * mask) < ub) if ub is not None else True)).sum())
        n_valid = np.array([gm(torch.ones_like(occ)), gm(occ), gm(~occ)], dtype=np.int64)
        arrs = dict(gt_left_q128=ql, gt_right_q128=qr, est0_off_q16=off, nonfinite_at=nonfinite,
                    has_lb=int(lb is not None), lb=np.float32(lb if lb is not None else 0), has_ub=int(ub is not None),
                    ub=np.float32(ub if ub is not None else 0), levels=np.array(levels, dtype=np.int64), margin=np.float64(margin),
                    calc_error=stack(ce), do_evaluation=stack(de), occ=np.stack([stack(oe, 'occ_'), stack(oe, 'noc_')]),
                    log_metric=lm, log_metric_keys=np.array(sorted(whole.keys())), n_valid=n_valid, nudge_rounds=it)
        for li in range(1, len(ests)):
            arrs["est%d" % li] = ests[li]
        save(name, **arrs)
        print("   margin %.4g after %d nudge rounds, N(all/occ/noc) = %s" % (margin, it, n_valid.tolist()))
    with open(os.path.join(OUT, "PROVENANCE_eval.txt"), "w") as fh:
        fh.write("eval_*.npz: tools/gen_golden.py --only-eval, torch %s CPU -- the reference's own calc_error / do_evaluation /\n"
                 "do_occlusion_evaluation (architecture/data/evaluation) and log_metric composed from them after validation_step's\n"
                 "F.interpolate, on seven seeded B=2 cases (dense, sparse, none valid, no bounds, ragged 50x70, NaN / inf estimate,\n"
                 "occluder band); inputs stored quantised (int16 / int8), ground truth nudged to a 1e-3 threshold margin.\n"
                 % torch.__version__)


RENDER_CAP_SAME, RENDER_CAP_RESCALED = 0.01, 0.08


def _reference_colormaps():
    """The reference's disparity_colormap.py, loaded by file path (the package __init__ imports more than this image has).  Its
    `plt` is wrapped so that the array handed to the colour map -- the re-valued error, the quantity that gets quantised -- can
    be read back; the colours still come from matplotlib's own jet."""
    import importlib.util
    import types
    os.environ.setdefault("MPLBACKEND", "Agg")
    path = os.path.join(ref_import.REFERENCE_ROOT, "architecture", "utils", "visualization", "disparity_colormap.py")
    spec = importlib.util.spec_from_file_location("_ref_disparity_colormap", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    real = mod.plt
    seen = []

    def get_cmap(name):
        cm = real.cm.get_cmap(name)

        def call(x):
            seen.append(np.array(x, copy=True))
            return cm(x)
        return call
    mod.plt = types.SimpleNamespace(cm=types.SimpleNamespace(get_cmap=get_cmap), xticks=lambda **k: None)
    return mod, seen, real


def render_cases(M):
    """Colour maps and the 16-bit map (architecture/utils/visualization/disparity_colormap.py, video_inference.py:169-227): the
    reference's own disp_to_color / disp_err_to_color / disp_err_to_colorbar on seeded maps, once on the float32 inputs (what the
    reference computes: the expected outputs) and once on the same values as float64 (how far its own rounding moves every
    quantity that gets quantised).  Per quantity tau = 4 x that deviation, taken over the same-size cases and over the rescaled
    case separately; a pixel within tau of a decision point is in the output's near-tie mask, where a test may accept the
    adjacent class / index / code.  A mask may hold at most 1 % of a case's pixels (8 % in the rescaled case): asserted here.
    Discrete outputs are stored as indices into the recorded tables (lossless), continuous ones as float32."""
    import warnings
    import matplotlib
    import torch.nn.functional as F
    warnings.filterwarnings("ignore")
    ref, seen, plt = _reference_colormaps()
    jet = plt.cm.get_cmap('jet')
    jet_table = jet(np.arange(256))[:, :3]
    class_bounds = np.array([0, 0.1875, 0.375, 0.75, 1.5, 3, 6, 12, 24, 48], dtype=np.float64) / 3.0
    class_rgb = np.array([[49, 54, 149], [69, 117, 180], [116, 173, 209], [171, 217, 233], [224, 243, 248], [254, 224, 144],
                          [253, 174, 97], [244, 109, 67], [215, 48, 39], [165, 0, 38]], dtype=np.float64) / 255.0
    breaks = [0, 1, 2, 4, 12, 16]
    # name: target size, estimate's size, batch, fraction of ground-truth zeros, error scale, options
    cases = {"render_dense": dict(hw=(48, 80), B=1, sparse=0.0, err=6.0),
             "render_sparse": dict(hw=(50, 78), B=1, sparse=0.7, err=6.0),
             "render_rescaled": dict(hw=(56, 88), low=(14, 22), B=1, sparse=0.0, err=3.0),
             "render_empty_range": dict(hw=(52, 92), B=1, sparse=0.0, err=6.0, hole=(12.0, 16.0)),
             "render_small_errors": dict(hw=(48, 80), B=1, sparse=0.1, err=0.25, clamp=0.95),
             "render_given_max": dict(hw=(49, 83), B=1, sparse=0.0, err=6.0, max_disp=60.0, below_zero=True),
             "render_batch3": dict(hw=(30, 50), B=3, sparse=0.3, err=5.0),
             "render_nonfinite": dict(hw=(40, 60), B=2, sparse=0.2, err=6.0, nonfinite=True)}
    runs = {}
    for ci, (name, c) in enumerate(cases.items()):
        seed = synth.SEED0 + 800 + ci
        B = c["B"]
        H, W = c["hw"]
        h, w = c.get("low", c["hw"])
        yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
        amp = synth.uniform(seed, "amp", (B, 1, 1), 20.0, 70.0).astype(np.float64)
        gt = 5.0 + amp * (0.55 + 0.3 * np.sin(2 * np.pi * xx / W + amp) + 0.15 * np.cos(2 * np.pi * yy / H))
        gt = (np.round((gt + synth.uniform(seed, "gtn", (B, H, W), -0.5, 0.5)) * 16) / 16).astype(np.float32)      # 1/16 px: compresses
        # errors spread over every range: a few large ones, many small ones
        u = synth.uniform(seed, "eu", (B, H, W))
        mag = np.where(u < 0.55, 1.0, np.where(u < 0.8, 4.0, np.where(u < 0.93, 12.0, 30.0))) * c["err"] / 6.0
        e = synth.normal(seed, "en", (B, H, W), 1.0).astype(np.float64) * mag
        if "clamp" in c:
            e = c["clamp"] * np.tanh(e)              # every error below 1, without a pile of equal values at the bound
        if "hole" in c:                               # no error inside (lo, hi]: pushed beyond hi
            lo, hi = c["hole"]
            e = np.where((np.abs(e) > lo - 0.2) & (np.abs(e) <= hi + 0.2), np.sign(e) * (hi + 0.2 + np.abs(e) - lo), e)
        full = (gt.astype(np.float64) + e).astype(np.float32)
        if c.get("below_zero"):
            full = np.where(synth.uniform(seed, "neg", (B, H, W)) < 0.03, -full * 0.1, full).astype(np.float32)
        gt = (gt * (synth.uniform(seed, "keep", (B, H, W)) >= c["sparse"])).astype(np.float32)
        if (h, w) != (H, W):
            iy, ix = (np.arange(h) * H) // h, (np.arange(w) * W) // w
            est = (full[:, iy][:, :, ix] * np.float32(w / W)).astype(np.float32)
        else:
            est = full
        if c.get("nonfinite"):
            est = est.copy()
            est[0, 10, 20] = np.nan          # on a valid pixel of image 0
            est[1, 30, 50] = np.inf          # image 1: an infinite error, no NaN
            gt[1, 30, 50] = max(gt[1, 30, 50], 7.0)
        runs[name] = dict(c=c, est=est, gt=gt)

    def rescale(est, H, W, dt):
        t = torch.from_numpy(est).to(dt).unsqueeze(1)
        if tuple(est.shape[-2:]) == (H, W):
            return t[:, 0].numpy()
        return F.interpolate(t * W / est.shape[-1], size=(H, W), mode='bilinear', align_corners=True)[:, 0].numpy()

    def run(est_full, gt, max_disp):
        """The reference on one image at one precision -> outputs and the quantised quantities."""
        r = {}
        with np.errstate(all="ignore"):
            r["disp_color"] = ref.disp_to_color(est_full, max_disp)
            r["cat_color"] = ref.disp_to_color(np.concatenate((est_full, gt), axis=0))
            r["err_class"] = ref.disp_err_to_color(est_full, gt)
            del seen[:]
            r["err_jet"] = ref.disp_err_to_colorbar(est_full, gt, with_bar=True, cmap='jet')
            r["x"], r["bar_x"] = seen[0], seen[1]
            del seen[:]
            assert np.array_equal(ref.disp_err_to_colorbar(est_full, gt), r["err_jet"][:-50], equal_nan=True)
            r["u16_q"] = est_full * 256
            # E of disp_err_to_color, restated (margins only; checked against the reference's classes below)
            a, b = est_full * 255.0, gt * 255.0
            E = np.abs(a - b)
            ok = b > 0
            tmp = np.zeros_like(b)
            tmp[ok] = E[ok] / b[ok] / 0.05
            r["E"] = np.minimum(E / 3.0, tmp)
            r["E_valid"] = ok
        return r

    # first pass: both precisions of every case, the deviations per group
    dev = {g: dict(E=0.0, x256=0.0, u16=0.0, c255=0.0, rescale=0.0) for g in ("same", "rescaled")}
    for name, r in runs.items():
        c = r["c"]
        H, W = c["hw"]
        grp = "rescaled" if "low" in c else "same"
        f32, f64 = rescale(r["est"], H, W, torch.float32), rescale(r["est"], H, W, torch.float64)
        r["full32"] = f32
        r["grp"] = grp
        r["r32"] = [run(f32[b], r["gt"][b], c.get("max_disp")) for b in range(c["B"])]
        r["r64"] = [run(f64[b], r["gt"][b].astype(np.float64), c.get("max_disp")) for b in range(c["B"])]
        d = dev[grp]
        fin = lambda a, b: np.isfinite(a) & np.isfinite(b)
        md = lambda a, b: float(np.abs(a.astype(np.float64) - b)[fin(a, b)].max()) if fin(a, b).any() else 0.0
        d["rescale"] = max(d["rescale"], md(f32, f64))
        for a, b in zip(r["r32"], r["r64"]):
            d["E"] = max(d["E"], md(np.where(a["E_valid"], a["E"], 0), np.where(b["E_valid"], b["E"], 0)))
            # the jet quantity is compared where both runs re-valued inside the same range (a pixel that changes range is a tie anyway)
            d["x256"] = max(d["x256"], md(a["x"] * 256.0, b["x"] * 256.0) if np.abs(a["x"].astype(np.float64) - b["x"])[fin(a["x"], b["x"])].max(initial=0) < 0.05 else d["x256"])
            d["u16"] = max(d["u16"], md(a["u16_q"], b["u16_q"]))
            for k in ("disp_color", "cat_color"):
                d["c255"] = max(d["c255"], md(np.clip(a[k], 0, 1) * 255.0, np.clip(b[k], 0, 1) * 255.0))
    tau = {g: {k: 4.0 * v for k, v in d.items()} for g, d in dev.items()}

    lines = ["render_*.npz: tools/gen_golden.py --only-render, numpy %s, matplotlib %s, torch %s CPU -- the reference's own disp_to_color /"
             % (np.__version__, matplotlib.__version__, torch.__version__),
             "disp_err_to_color / disp_err_to_colorbar (architecture/utils/visualization/disparity_colormap.py) on seeded maps; the rescaled",
             "case goes through F.interpolate(est * W / w, align_corners=True) as video_inference.py:182 does.  Expected outputs: the float32",
             "run.  Deviation = largest difference of a quantised quantity between that run and the same functions on float64 inputs",
             "(the rescale included); tau = 4 x deviation; near-tie mask = pixels within tau of a decision point."]
    for g in ("same", "rescaled"):
        lines.append("group %-8s deviation: E %.3g, jet x*256 %.3g, disp*256 %.3g, 255*colour %.3g, rescaled map %.3g" %
                     (g, dev[g]["E"], dev[g]["x256"], dev[g]["u16"], dev[g]["c255"], dev[g]["rescale"]))
        lines.append("group %-8s tau:       E %.3g, jet x*256 %.3g, disp*256 %.3g, 255*colour %.3g" %
                     (g, tau[g]["E"], tau[g]["x256"], tau[g]["u16"], tau[g]["c255"]))
    save("render_tables", jet=jet_table, class_rgb=class_rgb, class_bounds=class_bounds,
         versions=np.array([np.__version__, matplotlib.__version__, torch.__version__]))

    for name, r in runs.items():
        c, grp = r["c"], r["grp"]
        t = tau[grp]
        cap = RENDER_CAP_RESCALED if grp == "rescaled" else RENDER_CAP_SAME
        B = c["B"]
        H, W = c["hw"]
        arrs = dict(est=r["est"][:, None], gt=r["gt"][:, None], group=grp, cap=np.float64(cap),
                    has_max=int("max_disp" in c), max_disp=np.float32(c.get("max_disp", 0)),
                    tau=np.array([t["E"], t["x256"], t["u16"], t["c255"]]), rescale_dev=np.float64(dev[grp]["rescale"]))
        out = {k: [] for k in ("disp_color", "cat_color", "class_idx", "class_tie", "jet_idx", "jet_tie", "u16", "u16_tie",
                               "disp_color_u8_tie", "cat_color_u8_tie", "stats", "count_slack")}
        for a in r["r32"]:
            out["disp_color"].append(a["disp_color"].astype(np.float32))
            out["cat_color"].append(a["cat_color"].astype(np.float32))
            # classes: the index of the reference's colour (255: black), checked against the restated E
            img = a["err_class"]
            idx = np.full(img.shape[:2], 255, dtype=np.uint8)
            for k in range(10):
                idx[np.all(img == class_rgb[k], axis=-1)] = k
            assert np.all((idx == 255) == np.all(img == 0, axis=-1))
            E = a["E"].astype(np.float64)
            mine = np.where(a["E_valid"] & ~np.isnan(E), (E[..., None] >= class_bounds[1:]).sum(-1), 255)
            assert np.array_equal(mine, idx), name
            out["class_idx"].append(idx)
            out["class_tie"].append(a["E_valid"] & (np.abs(E[..., None] - class_bounds[1:]) <= t["E"]).any(-1))
            # jet: the index matplotlib took (x * 256 truncated, 1 -> 255), -1 for its `bad` colour
            x = a["x"]
            with np.errstate(all="ignore"):
                xi = x.astype(np.float32) * np.float32(256)
                ji = np.where(np.isnan(xi), -1, np.where(xi >= 256, 255, np.where(xi < 0, 0, xi.astype(np.int64)))).astype(np.int16)
            full = a["err_jet"]
            assert np.array_equal(np.where(ji[..., None] >= 0, jet_table[np.maximum(ji, 0)], 0.0), full[:-50]), name
            bi = np.where(a["bar_x"][0] * 256 >= 256, 255, (a["bar_x"][0] * 256).astype(np.int64)).astype(np.int16)
            assert np.array_equal(jet_table[bi], full[-1]), name
            out["jet_idx"].append(ji)
            with np.errstate(all="ignore"):
                frac = np.abs(xi.astype(np.float64) - np.round(xi.astype(np.float64)))
                out["jet_tie"].append(np.isfinite(xi) & (x != 0) & (frac <= t["x256"]))
                q = a["u16_q"].astype(np.float64)
                out["u16"].append(np.where(np.isnan(q), 0, np.clip(np.trunc(q), 0, 65535)).astype(np.uint16))
                out["u16_tie"].append(np.isfinite(q) & (np.abs(q - np.round(q)) <= t["u16"]) & (t["u16"] > 0))
                for k in ("disp_color", "cat_color"):
                    v = np.clip(a[k], 0, 1) * 255.0
                    out[k + "_u8_tie"].append(np.isfinite(v) & (np.abs(v - np.floor(v) - 0.5) <= t["c255"]))
            # statistics: maxima and the ranges of the error, from the reference's own arithmetic (|est - gt| * valid in float32)
            with np.errstate(all="ignore"):
                est_full = a["u16_q"] / 256
                g = r["gt"][len(out["stats"])]
                err = np.abs(est_full - g) * (g > 0)
                mx = err.max()
                ups = breaks[1:] + [max(192, mx)]
                st = [est_full.max(), g.max(), np.concatenate((est_full, g)).max(), mx]
                mn_, mx_, cn_, sl_ = [], [], [], []
                for lo, hi in zip(breaks, ups):
                    m = (err > lo) & (err <= hi)
                    mn_.append(err[m].min() if m.any() else np.inf)
                    mx_.append(err[m].max() if m.any() else -np.inf)
                    cn_.append(int(m.sum()))
                    sl_.append(int(((np.abs(err - lo) <= 4 * dev[grp]["rescale"]) | (np.abs(err - hi) <= 4 * dev[grp]["rescale"])).sum())
                               if grp == "rescaled" else 0)
            out["stats"].append(np.array(st + mn_ + mx_ + cn_, dtype=np.float64))
            out["count_slack"].append(np.array(sl_, dtype=np.int64))
        bar = np.where(r["r32"][0]["bar_x"][0] * 256 >= 256, 255, (r["r32"][0]["bar_x"][0] * 256).astype(np.int64)).astype(np.int16)
        arrs["bar_idx"] = bar
        shares = {}
        # disp_to_color with its own maximum is what cat_color's rows are (one map, one maximum): stored only where a maximum is given
        for k in (("cat_color", "cat_color_u8_tie") if "max_disp" in c else ("disp_color", "disp_color_u8_tie")):
            del out[k]
        for k, v in out.items():
            arrs[k] = np.stack(v)
            if k.endswith("_tie"):
                shares[k] = float(arrs[k].mean())
                assert shares[k] <= cap, "%s: near-tie share of %s is %.4f, above the cap %.2f -- change the case" % (name, k, shares[k], cap)
        arrs["tie_shares"] = np.array([shares[k] for k in sorted(shares)])
        arrs["tie_names"] = np.array(sorted(shares))
        save(name, **arrs)
        sz = os.path.getsize(os.path.join(OUT, name + ".npz"))
        assert sz <= 100 * 1024, (name, sz)
        lines.append("%-20s %s B=%d %dx%d est %s  near-tie shares: %s" % (name, grp, B, H, W, tuple(r["est"].shape[-2:]),
                     ", ".join("%s %.4f" % (k.replace("_tie", ""), shares[k]) for k in sorted(shares))))
        lines.append("%-20s range counts %s" % ("", [a[-6:].astype(int).tolist() for a in out["stats"]]))
    with open(os.path.join(OUT, "PROVENANCE_render.txt"), "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


# ----------------------------------------------------------------------------------------------
PREPARE_CASES = ("prepare_same", "prepare_ramp", "prepare_dataset_up", "prepare_video_up", "prepare_down", "prepare_train_crop",
                 "prepare_degenerate", "prepare_disp16")


def _torchvision_stand_in(state):
    """torchvision is not installed: a stand-in of the project's own writing, registered before the reference's dataset module is
    imported.  ToTensor of a PIL RGB image and functional.normalize as torchvision defines them (uint8 HWC -> float CHW / 255;
    (t - mean) / std with mean / std in the tensor's dtype).  state['dtype'] switches the float type, so that the reference's own
    functions can be run again on float64 inputs.  ColorJitter / adjust_gamma are never called (colour augmentation is pinned off)."""
    import types

    class ToTensor:
        def __call__(self, pic):
            return torch.from_numpy(np.array(pic, dtype=np.uint8, copy=True)).permute(2, 0, 1).contiguous().to(state["dtype"]).div(255)

    class Compose:
        def __init__(self, ts):
            self.transforms = ts

        def __call__(self, x):
            for t in self.transforms:
                x = t(x)
            return x

    class ColorJitter:
        def __init__(self, *a, **k):
            pass

        def __call__(self, x):
            raise RuntimeError("colour augmentation is pinned off in the fixtures")

    def normalize(tensor, mean, std, inplace=False):
        mean = torch.as_tensor(mean, dtype=tensor.dtype)
        std = torch.as_tensor(std, dtype=tensor.dtype)
        return (tensor - mean[:, None, None]) / std[:, None, None]

    def adjust_gamma(*a, **k):
        raise RuntimeError("colour augmentation is pinned off in the fixtures")

    fn = types.ModuleType("torchvision.transforms.functional")
    fn.normalize, fn.adjust_gamma = normalize, adjust_gamma
    tr = types.ModuleType("torchvision.transforms")
    tr.ToTensor, tr.Compose, tr.ColorJitter, tr.functional = ToTensor, Compose, ColorJitter, fn
    tv = types.ModuleType("torchvision")
    tv.transforms = tr
    sys.modules.setdefault("torchvision", tv)
    sys.modules.setdefault("torchvision.transforms", tr)
    sys.modules.setdefault("torchvision.transforms.functional", fn)
    return tr, fn


def _reference_prepare(state):
    """The reference's dataset base class (by file path: the package __init__ imports loaders this image lacks) and the top-level
    functions of video_inference.py by the AST route of reference_update_map (its module-level imports do not resolve here)."""
    import ast
    import importlib.util
    import types
    import torch.nn.functional as F
    from PIL import Image
    tr, fn = _torchvision_stand_in(state)
    path = os.path.join(ref_import.REFERENCE_ROOT, "architecture", "data", "datasets", "base.py")
    spec = importlib.util.spec_from_file_location("_ref_dataset_base", path)
    base = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(base)

    def imread(path, flags=None):                      # cv2.imread(IMREAD_ANYDEPTH): PIL's 16-bit reader
        with Image.open(path) as im:
            assert im.mode in ("I;16", "I;16B", "I"), im.mode
            return np.array(im).astype(np.uint16)
    cv2 = types.SimpleNamespace(imread=imread, IMREAD_ANYDEPTH=2, IMREAD_ANYCOLOR=4)
    path = os.path.join(ref_import.REFERENCE_ROOT, "projects", "TemporalStereo", "video_inference.py")
    tree = ast.parse(open(path).read(), filename=path)
    want = ("pil_loader", "read_image", "read_intrinsics", "read_disparity")
    fns = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in want]
    assert len(fns) == len(want)
    # the single-scale intrinsics of inference_stereo (:245-251): the assignments to norm_K / kh, kw / scale_K / inv_scale_K
    outer = next(n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "inference_stereo")
    names = {"norm_K", "baseline", "kh", "kw", "scale_K", "inv_scale_K"}
    k_stmts = [n for n in outer.body if isinstance(n, ast.Assign) and
               {x.id for t in n.targets for x in ast.walk(t) if isinstance(x, ast.Name)} & names]
    assert len(k_stmts) == 7, len(k_stmts)
    k_fn = ast.parse("def single_scale_K(resize_to_shape):\n    pass\n    return scale_K, inv_scale_K, baseline").body[0]
    k_fn.body[0:1] = k_stmts
    ns = {"Image": Image, "transforms": tr, "transF": fn, "F": F, "np": np, "cv2": cv2, "torch": torch}
    exec(compile(ast.fix_missing_locations(ast.Module(body=fns + [k_fn], type_ignores=[])), path, "exec"), ns)
    return base, ns


def prepare_cases(M):
    """Input preparation (video_inference.py:100-140, :245-251; datasets/base.py:99-187, :231-248): the reference's own
    StereoDatasetBase.__getitem__ / do_transform on a throw-away dataset (seeded uint8 PNGs, a JSON annotation file) and its
    read_image / read_disparity, once in float32 (the expected outputs) and, for the resized cases, once more on float64 inputs;
    dev32_64 = max |fp32 run - fp64 run| of a case is the distance the reference itself keeps from the float64 answer."""
    import json
    import random as pyrandom
    import tempfile
    import types
    import PIL
    from PIL import Image
    state = {"dtype": torch.float32}
    base, vi = _reference_prepare(state)
    K_of = {k: vi["read_intrinsics"](k)[0] for k in ("kitti", "tartanair")}
    full_res = {"kitti": (375, 1242), "tartanair": (480, 640)}

    class ThrowAway(base.StereoDatasetBase):
        camera = "kitti"
        resolution = None

        def Loader(self, image_path):
            return base.pil_loader(os.path.join(self.root, image_path))

        def intrinsicLoader(self, intrinsic_path):
            K = K_of[self.camera].copy()
            h, w = self.resolution
            full_K = K.copy()
            full_K[0] *= w
            full_K[1] *= h
            return K, full_K, (h, w)

    def noise(seed, tag, shape):
        return synth._rs(seed, tag).randint(0, 256, size=shape).astype(np.uint8)

    def ramp(H, W):
        """every byte value in every channel, the channels out of step"""
        idx = np.arange(H * W).reshape(H, W)
        return np.stack([(idx * 1 + 0) % 256, (idx * 3 + 85) % 256, (255 - idx) % 256], axis=-1).astype(np.uint8)

    def dataset_run(tmp, lefts, rights, size, is_train, camera, dtype, crops=None):
        """the reference's dataset over B stereo pairs -> stacked sample tensors"""
        state["dtype"] = dtype
        items = []
        for b, (l, r) in enumerate(zip(lefts, rights)):
            for side, img in (("left", l), ("right", r)):
                Image.fromarray(img, "RGB").save(os.path.join(tmp, "%s_%d.png" % (side, b)))
            items.append({"0": {"left_image_path": "left_%d.png" % b, "right_image_path": "right_%d.png" % b}})
        ann = os.path.join(tmp, "ann.json")
        with open(ann, "w") as fh:
            json.dump(items, fh)
        draws = iter([v for c in (crops or []) for v in c])
        taken = []

        def randint(lo, hi):
            v = next(draws)
            assert lo <= v <= hi
            taken.append(v)
            return v
        # pinned draws: no colour augmentation (random.random), the recorded crop origins (random.randint), no occlusion patch
        base.random = types.SimpleNamespace(random=lambda: 0.0, randint=randint, uniform=pyrandom.uniform)
        real_binomial = np.random.binomial
        np.random.binomial = lambda n, p: 0
        try:
            ThrowAway.camera, ThrowAway.resolution = camera, lefts[0].shape[:2]
            ds = ThrowAway(ann, tmp, size[0], size[1], [0], is_train=is_train)
            samples = [ds[b] for b in range(len(items))]
        finally:
            np.random.binomial = real_binomial
            base.random = pyrandom
        assert taken == [v for c in (crops or []) for v in c]
        S = min(int(np.log2(size[1])), int(np.log2(size[0])))
        out = {"color_l": torch.stack([s[("color", 0, "l")] for s in samples]), "color_r": torch.stack([s[("color", 0, "r")] for s in samples]),
               "aug_l": torch.stack([s[("color_aug", 0, "l")] for s in samples]), "aug_r": torch.stack([s[("color_aug", 0, "r")] for s in samples]),
               "K": torch.stack([torch.stack([s[("K", k)] for k in range(S)]) for s in samples]),
               "inv_K": torch.stack([torch.stack([s[("inv_K", k)] for k in range(S)]) for s in samples]),
               "baseline": torch.stack([s["baseline"] for s in samples])}
        assert all(("K", S) not in s for s in samples)
        return {k: v.numpy() for k, v in out.items()}

    def video_run(tmp, left, right, size, dtype):
        state["dtype"] = dtype
        out = {}
        for side, img in (("l", left), ("r", right)):
            path = os.path.join(tmp, "v_%s.png" % side)
            Image.fromarray(img, "RGB").save(path)
            image, proc = vi["read_image"](path, size)
            out["color_" + side], out["aug_" + side] = image[None].numpy(), proc[None].numpy()
        return out

    lines = ["prepare_*.npz: tools/gen_golden.py --only-prepare, numpy %s, PIL %s, torch %s CPU -- the reference's own" % (np.__version__, PIL.__version__, torch.__version__),
             "StereoDatasetBase.__getitem__ / do_transform (architecture/data/datasets/base.py) on a throw-away dataset of seeded uint8 PNGs,",
             "and read_image / read_intrinsics / read_disparity and the single-scale K of inference_stereo (projects/TemporalStereo/",
             "video_inference.py, taken by their syntax trees: the module's own imports do not resolve here).",
             "torchvision is not installed: ToTensor / functional.normalize / Compose come from a stand-in written for this generator",
             "(PIL RGB -> from_numpy(...).permute(2,0,1).contiguous().to(float).div(255); (t - mean[:,None,None]) / std[:,None,None] with",
             "mean / std in the tensor's dtype); cv2.imread is stood in by PIL's 16-bit reader.  Training cases pin random.random (no colour",
             "augmentation), random.randint (the recorded crop origins) and np.random.binomial (no occlusion patch).",
             "Expected outputs: the float32 run.  Resized cases also hold the same functions run on float64 inputs (stored as the float32",
             "run plus a float32 difference); dev32_64 = max |fp32 run - fp64 run| over the case."]
    seed0 = synth.SEED0 + 900

    def finish(name, subs):
        """subs: list of dicts of arrays; key<k> per sub-case"""
        arrs = {"subs": np.int64(len(subs))}
        dev = 0.0
        resized = False
        for k, sub in enumerate(subs):
            for key, v in sub.items():
                if key.startswith("aug64_"):
                    a32 = sub["aug_" + key[-1]]
                    d = v - a32.astype(np.float64)
                    dev = max(dev, float(np.abs(d).max()))
                    resized = True
                    arrs["d64_%s%d" % (key[-1], k)] = d.astype(np.float32)
                else:
                    arrs["%s%d" % (key, k)] = v
        if resized:
            assert dev > 0
            arrs["dev32_64"] = np.float64(dev)
        save(name, **arrs)
        sz = os.path.getsize(os.path.join(OUT, name + ".npz"))
        assert sz <= 110 * 1024, (name, sz)
        lines.append("%-20s %d sub-case(s), %s%s" % (name, len(subs), "; ".join(
            "%s -> %s B=%d" % (tuple(s["left"].shape[1:3]), tuple(s["aug_l"].shape[-2:]), s["left"].shape[0]) for s in subs if "left" in s),
            ("  dev32_64 %.3g" % dev) if resized else "  exact"))

    with tempfile.TemporaryDirectory() as tmp:
        # --- same size, through the dataset (evaluation form, source == target)
        L, R = noise(seed0, "sameL", (1, 31, 45, 3)), noise(seed0, "sameR", (1, 31, 45, 3))
        r = dataset_run(tmp, L, R, (31, 45), False, "kitti", torch.float32)
        finish("prepare_same", [dict(left=L, right=R, K_norm=K_of["kitti"], k_size=np.array([31, 45]), **r)])

        # --- every byte value in every channel, ragged widths
        subs = []
        for H, W in ((20, 13), (19, 14), (18, 15)):
            L = ramp(H, W)[None]
            R = L[:, ::-1, ::-1].copy()
            assert all(len(np.unique(L[..., c])) == 256 for c in range(3))
            r = dataset_run(tmp, L, R, (H, W), False, "kitti", torch.float32)
            subs.append(dict(left=L, right=R, color_l=r["color_l"], color_r=r["color_r"], aug_l=r["aug_l"], aug_r=r["aug_r"]))
        finish("prepare_ramp", subs)

        # --- "pad by resize" of base.py:183, B=2, and the K pyramid at the resized size
        L, R = noise(seed0 + 1, "upL", (2, 19, 33, 3)), noise(seed0 + 1, "upR", (2, 19, 33, 3))
        r = dataset_run(tmp, L, R, (24, 36), False, "kitti", torch.float32)
        r64 = dataset_run(tmp, L, R, (24, 36), False, "kitti", torch.float64)
        assert r64["aug_l"].dtype == np.float64
        finish("prepare_dataset_up", [dict(left=L, right=R, K_norm=K_of["kitti"], k_size=np.array([24, 36]), aug64_l=r64["aug_l"],
                                           aug64_r=r64["aug_r"], **r)])

        # --- read_image, the unsqueeze(dim=1) form, and inference_stereo's single-scale K
        for name, src, dst, sd in (("prepare_video_up", (30, 40), (34, 52), 2), ("prepare_down", (45, 77), (16, 30), 3)):
            L, R = noise(seed0 + sd, "vL", (1,) + src + (3,)), noise(seed0 + sd, "vR", (1,) + src + (3,))
            r = video_run(tmp, L[0], R[0], dst, torch.float32)
            r64 = video_run(tmp, L[0], R[0], dst, torch.float64)
            K, invK, baseline = vi["single_scale_K"](dst)
            finish(name, [dict(left=L, right=R, K_norm=K_of["tartanair"], k_size=np.array(dst),
                               K=torch.from_numpy(K).float()[None, None].numpy(), inv_K=torch.from_numpy(invK).float()[None, None].numpy(),
                               baseline=np.float32(baseline), aug64_l=r64["aug_l"], aug64_r=r64["aug_r"], **r)])

        # --- training crop: both outputs cropped, K at the un-cropped resolution
        L, R = noise(seed0 + 4, "cropL", (2, 37, 57, 3)), noise(seed0 + 4, "cropR", (2, 37, 57, 3))
        crops = [(0, 0), (37 - 24, 57 - 40)]
        r = dataset_run(tmp, L, R, (24, 40), True, "tartanair", torch.float32, crops=crops)
        assert r["color_l"].shape[-2:] == (24, 40)
        finish("prepare_train_crop", [dict(left=L, right=R, crop=np.array(crops, dtype=np.int32), K_norm=K_of["tartanair"],
                                           k_size=np.array([37, 57]), **r)])

        # --- degenerate sizes: a 1 x W and an H x 1 source, a target of height 1 (ac_scale's zero branch)
        subs = []
        for k, (src, dst) in enumerate((((1, 21), (5, 30)), ((17, 1), (20, 7)), ((9, 13), (1, 20)))):
            L, R = noise(seed0 + 5, "dgL%d" % k, (1,) + src + (3,)), noise(seed0 + 5, "dgR%d" % k, (1,) + src + (3,))
            r = video_run(tmp, L[0], R[0], dst, torch.float32)
            r64 = video_run(tmp, L[0], R[0], dst, torch.float64)
            subs.append(dict(left=L, right=R, aug64_l=r64["aug_l"], aug64_r=r64["aug_r"], **r))
        finish("prepare_degenerate", subs)

        # --- read_disparity on a 16-bit PNG
        raw = synth._rs(seed0 + 6, "d16").randint(0, 65536, size=(40, 61)).astype(np.uint16)
        raw[synth.uniform(seed0 + 6, "d16z", (40, 61)) < 0.3] = 0
        raw[0, :3] = (0, 1, 65535)
        path = os.path.join(tmp, "disp.png")
        Image.fromarray(raw).save(path)
        disp = vi["read_disparity"](path)
        assert disp.dtype == np.float64 and np.array_equal(disp.astype(np.float32).astype(np.float64), disp)
        save("prepare_disp16", subs=np.int64(1), raw0=raw[None], disp0=disp.astype(np.float32)[None, None], valid0=(raw > 0)[None, None])
        lines.append("%-20s 40x61, %.0f %% zeros, holds 0, 1 and 65535  exact" % ("prepare_disp16", 100 * (raw == 0).mean()))
    with open(os.path.join(OUT, "PROVENANCE_prepare.txt"), "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


# ----------------------------------------------------------------------------------------------
AUGMENT_CASES = ("augment_ops", "augment_orders", "augment_chain", "augment_occlusion", "augment_large", "augment_identity")


def augment_cases(M):
    """Colour augmentation, crop and occlusion of the training input (datasets/base.py:65-187): the reference's own
    StereoDatasetBase.do_transform (is_train=True) on a throw-away dataset of seeded uint8 PNGs with every random source pinned to
    recorded values.  torchvision is not installed: ColorJitter / adjust_gamma are stood in by the PIL calls torchvision's PIL path
    makes (ImageEnhance.Brightness / Contrast / Color, the HSV round trip with the numpy uint8 hue shift, Image.point with the
    truncating table); the stand-in takes its order and factors from the recorded list instead of torch's random stream."""
    import json
    import random as pyrandom
    import tempfile
    import types
    import PIL
    from PIL import Image, ImageEnhance
    state = {"dtype": torch.float32, "jitter": None, "stages": None}
    base, vi = _reference_prepare(state)
    K_of = {"tartanair": vi["read_intrinsics"]("tartanair")[0]}
    NAMES = ("brightness", "contrast", "saturation", "hue")

    class ColorJitter:                                   # the PIL path of torchvision's ColorJitter with pinned draws
        def __init__(self, *a, **k):
            pass

        def __call__(self, img):
            par = next(state["jitter"])
            for op in par["order"]:
                f = par[NAMES[op]]
                if op == 0:
                    img = ImageEnhance.Brightness(img).enhance(f)
                elif op == 1:
                    img = ImageEnhance.Contrast(img).enhance(f)
                elif op == 2:
                    img = ImageEnhance.Color(img).enhance(f)
                else:
                    h, s, v = img.convert("HSV").split()
                    np_h = np.array(h, dtype=np.uint8)
                    np_h = (np_h.astype(np.int64) + int(np.array(int(f * 255)).astype(np.uint8))).astype(np.uint8)    # uint8 wrap-around
                    img = Image.merge("HSV", (Image.fromarray(np_h, "L"), s, v)).convert("RGB")
            return img

    def adjust_gamma(img, gamma, gain=1):
        table = [min(255, int((255 + 1 - 1e-3) * gain * pow(e / 255.0, gamma))) for e in range(256)] * 3
        out = img.point(table)
        state["stages"].append(np.array(out, dtype=np.uint8))
        return out

    base.transforms.ColorJitter = ColorJitter
    base.transforms.functional.adjust_gamma = adjust_gamma

    class ThrowAway(base.StereoDatasetBase):
        def Loader(self, image_path):
            return base.pil_loader(os.path.join(self.root, image_path))

        def intrinsicLoader(self, intrinsic_path):
            K = K_of["tartanair"].copy()
            full_K = K.copy()
            return K, full_K, self.resolution

    def picture(seed, tag, H, W, block=2):
        """noise in block x block tiles (it keeps the files small) with greys, saturated primaries / secondaries, black, white and
        pixels with two equal channels planted"""
        tiles = synth._rs(seed, tag).randint(0, 256, size=((H + block - 1) // block, (W + block - 1) // block, 3)).astype(np.uint8)
        img = np.repeat(np.repeat(tiles, block, axis=0), block, axis=1)[:H, :W].copy()
        img[0] = img[0, :, :1]                                                   # greys
        prim = np.array([(255, 0, 0), (0, 255, 0), (0, 0, 255), (255, 255, 0), (0, 255, 255), (255, 0, 255), (0, 0, 0), (255, 255, 255)], dtype=np.uint8)
        img[1, :len(prim)] = prim[:min(len(prim), W)]
        img[2, :, 1] = img[2, :, 0]                                              # R == G
        img[3, :, 2] = img[3, :, 1]                                              # G == B
        img[4, :, 2] = img[4, :, 0]                                              # R == B
        return img

    def run(tmp, lefts, rights, size, rows, crops, rects, color=True):
        """rows[e][b]: dict(order, brightness, contrast, saturation, hue, gamma); rects[b]: list of (sh, sw, occh, occw) for the right
        eye.  One dataset object per image (do_color_aug and the pins are per object)."""
        B = len(lefts)
        Hs, Ws = lefts[0].shape[:2]
        out = {k: [] for k in ("color_l", "color_r", "aug_l", "aug_r", "stage_l", "stage_r")}
        for b in range(B):
            for side, img in (("left", lefts[b]), ("right", rights[b])):
                Image.fromarray(img, "RGB").save(os.path.join(tmp, "%s.png" % side))
            ann = os.path.join(tmp, "ann.json")
            with open(ann, "w") as fh:
                json.dump([{"0": {"left_image_path": "left.png", "right_image_path": "right.png"}}], fh)
            state["jitter"] = iter([rows[0][b], rows[1][b]])
            state["stages"] = []
            uni = iter([v for e in (0, 1) for v in (1.0, rows[e][b]["gamma"])])          # AdjustGamma: gain, then gamma
            ints = iter(list(crops[b]))
            base.random = types.SimpleNamespace(random=lambda: 1.0 if color else 0.0, randint=lambda lo, hi: next(ints),
                                                uniform=lambda lo, hi: next(uni))
            # occlusion: binomial 1 for every key (only the right eye's color_aug takes it), the count, then per rectangle occw, occh, sw, sh
            rc = rects[b]
            np_uni = iter([float(v) + 0.25 for (sh, sw, oh, ow) in rc for v in (ow, oh, sw, sh)])
            real = (np.random.binomial, np.random.randint, np.random.uniform)
            np.random.binomial = lambda n, p: 1 if rc else 0
            np.random.randint = lambda lo, hi: len(rc)
            np.random.uniform = lambda lo, hi: next(np_uni)
            np.random.seed(1234 + b)
            try:
                ThrowAway.resolution = (Hs, Ws)
                ds = ThrowAway(ann, tmp, size[0], size[1], [0], is_train=True)
                assert ds.do_color_aug == color
                sm = ds[0]
            finally:
                np.random.binomial, np.random.randint, np.random.uniform = real
                base.random = pyrandom
            assert next(np_uni, None) is None and next(ints, None) is None
            if color:
                assert len(state["stages"]) == 2 and next(state["jitter"], None) is None
                out["stage_l"].append(state["stages"][0]); out["stage_r"].append(state["stages"][1])
            else:
                out["stage_l"].append(lefts[b]); out["stage_r"].append(rights[b])
            for k, key in (("color_l", ("color", 0, "l")), ("color_r", ("color", 0, "r")), ("aug_l", ("color_aug", 0, "l")),
                           ("aug_r", ("color_aug", 0, "r"))):
                v = sm[key]
                assert v.dtype == torch.float32 and tuple(v.shape) == (3,) + tuple(size), (key, v.dtype, v.shape)
                out[k].append(v.numpy().copy())
        return {k: np.stack(v) for k, v in out.items()}

    def pack(lefts, rights, size, rows, crops, rects, r):
        B = len(lefts)
        order = np.full((2, B, 4), 4, dtype=np.int64)
        factors = np.zeros((2, B, 4), dtype=np.float64)
        gam = np.zeros((2, B), dtype=np.float64)
        for e in (0, 1):
            for b in range(B):
                order[e, b, :len(rows[e][b]["order"])] = rows[e][b]["order"]
                factors[e, b] = [rows[e][b][n] for n in NAMES]
                gam[e, b] = rows[e][b]["gamma"]
        rc = np.zeros((B, 4, 4), dtype=np.int64)
        for b in range(B):
            for k, q in enumerate(rects[b]):
                rc[b, k] = q
        return dict(left=np.stack(lefts), right=np.stack(rights), size=np.array(size), order=order, factors=factors, gamma=gam,
                    crop=np.array(crops, dtype=np.int64), rects=rc, nrect=np.array([len(q) for q in rects]), **r)

    def par(order=(), brightness=1.0, contrast=1.0, saturation=1.0, hue=0.0, gamma=1.0):
        return dict(order=list(order), brightness=brightness, contrast=contrast, saturation=saturation, hue=hue, gamma=gamma)

    lines = ["augment_*.npz: tools/gen_golden.py --only-augment, numpy %s, PIL %s, torch %s CPU -- the reference's own" % (np.__version__, PIL.__version__, torch.__version__),
             "StereoDatasetBase.do_transform (architecture/data/datasets/base.py:99-187, is_train=True) on a throw-away dataset of seeded",
             "uint8 PNGs, one dataset object per image.  torchvision is not installed: ToTensor / normalize / Compose are the stand-ins of",
             "PROVENANCE_prepare.txt; ColorJitter and functional.adjust_gamma are stood in by the PIL calls torchvision's PIL path makes --",
             "ImageEnhance.Brightness / Contrast / Color(img).enhance(f); img.convert('HSV'), H += uint8(int(f * 255)) with uint8 wrap-around,",
             "Image.merge('HSV', ...).convert('RGB'); img.point(table * 3) -- with the order and the factors taken from a recorded list",
             "instead of torch's random stream.  Gamma-table convention: the TRUNCATING integer table of torchvision's current PIL path,",
             "min(255, int((255 + 1 - 1e-3) * gain * (e / 255.0) ** gamma)); gamma = 1 is then the identity.  (Older torchvision versions hand",
             "Image.point a float table, which PIL 12 rounds: 113-127 of the 256 entries differ.  The reference pins no version.)",
             "Pinned: random.random (do_color_aug), random.uniform (gain 1.0, the recorded gamma), random.randint (the recorded crop",
             "origins), np.random.binomial / randint / uniform (the recorded rectangles; each uniform returns the recorded integer + 0.25).",
             "np.random.normal is numpy's own, seeded: the values inside rectangles are the reference's noise and are NOT compared.",
             "stage_l / stage_r: the uint8 frame adjust_gamma returned (the full frame after all colour operations).",
             "Expected outputs: the float32 tensors do_transform returned."]
    seed0 = synth.SEED0 + 1000
    total = 0

    def finish(name, arrs, note):
        nonlocal total
        save(name, **arrs)
        sz = os.path.getsize(os.path.join(OUT, name + ".npz"))
        total += sz
        lines.append("%-20s B=%d %s -> %s  %s" % (name, arrs["left"].shape[0], tuple(arrs["left"].shape[1:3]), tuple(int(v) for v in arrs["size"]), note))

    with tempfile.TemporaryDirectory() as tmp:
        # --- each operation alone: both ends and the middle of its range; gamma alone
        H, W = 20, 28
        L, R = picture(seed0, "opsL", H, W), picture(seed0, "opsR", H, W)[::-1].copy()
        ps = [par((0,), brightness=v) for v in (0.4, 1.2, 2.0)] + [par((1,), contrast=v) for v in (0.5, 1.0, 1.5)] + \
             [par((2,), saturation=v) for v in (0.5, 1.0, 1.5)] + [par((3,), hue=v) for v in (-0.1, 0.0, 0.1)] + \
             [par((), gamma=v) for v in (0.8, 1.0, 1.2)]
        B = len(ps)
        rows = [ps, ps]
        r = run(tmp, [L] * B, [R] * B, (H, W), rows, [()] * B, [[]] * B)
        finish("augment_ops", pack([L] * B, [R] * B, (H, W), rows, [(0, 0)] * B, [[]] * B, r),
               "brightness 0.4 / 1.2 / 2.0, contrast and saturation 0.5 / 1.0 / 1.5, hue -0.1 / 0 / 0.1, gamma 0.8 / 1.0 / 1.2, each alone")

        # --- all 24 orders with fixed factors: left eye order k, right eye order 23 - k
        import itertools
        perms = list(itertools.permutations(range(4)))
        L, R = picture(seed0 + 1, "ordL", H, W), picture(seed0 + 1, "ordR", H, W)
        fx = dict(brightness=1.3, contrast=0.7, saturation=1.4, hue=0.07, gamma=1.0)
        rows = [[par(perms[k], **fx) for k in range(12)], [par(perms[23 - k], **fx) for k in range(12)]]
        r = run(tmp, [L] * 12, [R] * 12, (H, W), rows, [()] * 12, [[]] * 12)
        finish("augment_orders", pack([L] * 12, [R] * 12, (H, W), rows, [(0, 0)] * 12, [[]] * 12, r),
               "all 24 orders (left: k, right: 23 - k), brightness 1.3, contrast 0.7, saturation 1.4, hue 0.07")

        # --- the full chain + gamma + crop, B=2, different parameters per image and eye
        Ls = [picture(seed0 + 2, "chL%d" % b, 37, 57) for b in range(2)]
        Rs = [picture(seed0 + 2, "chR%d" % b, 37, 57) for b in range(2)]
        rows = [[par((2, 0, 3, 1), 0.62, 1.37, 0.81, -0.083, 0.87), par((1, 3, 0, 2), 1.71, 0.58, 1.22, 0.031, 1.16)],
                [par((3, 2, 1, 0), 1.05, 0.93, 1.45, 0.095, 1.04), par((0, 1, 2, 3), 0.45, 1.49, 0.55, -0.049, 0.93)]]
        crops = [(0, 17), (13, 3)]
        r = run(tmp, Ls, Rs, (24, 40), rows, crops, [[], []])
        finish("augment_chain", pack(Ls, Rs, (24, 40), rows, crops, [[], []], r), "full chain + gamma + crop, per image and eye")

        # --- occlusion: 2, 3 and 4 rectangles, overlapping and touching the window's border; the left eye untouched
        Ls = [picture(seed0 + 3, "ocL%d" % b, 44, 66, 3) for b in range(3)]
        Rs = [picture(seed0 + 3, "ocR%d" % b, 44, 66, 3) for b in range(3)]
        rows = [[par((0, 1, 2, 3), 1.1, 0.9, 1.2, 0.02, 0.95)] * 3, [par((3, 1, 0, 2), 0.8, 1.3, 0.7, -0.06, 1.1)] * 3]
        rects = [[(0, 0, 9, 12), (5, 8, 10, 10)],
                 [(30, 48, 10, 12), (2, 50, 12, 7), (20, 20, 6, 30)],
                 [(0, 40, 15, 20), (10, 30, 20, 20), (25, 0, 15, 35), (12, 33, 5, 5)]]
        crops = [(1, 2), (4, 6), (0, 0)]
        r = run(tmp, Ls, Rs, (40, 60), rows, crops, rects)
        finish("augment_occlusion", pack(Ls, Rs, (40, 60), rows, crops, rects, r), "2 / 3 / 4 rectangles, overlapping, touching the border")

        # --- one case large enough for patches of the default size
        Ls, Rs = [picture(seed0 + 4, "lgL", 130, 210, 6)], [picture(seed0 + 4, "lgR", 130, 210, 6)]
        rows = [[par((1, 0, 2, 3), 1.4, 1.2, 0.9, 0.05, 0.9)], [par((2, 3, 1, 0), 0.7, 0.8, 1.3, -0.02, 1.15)]]
        rects = [[(3, 10, 50, 50), (70, 148, 50, 52)]]
        r = run(tmp, Ls, Rs, (120, 200), rows, [(7, 5)], rects)
        finish("augment_large", pack(Ls, Rs, (120, 200), rows, [(7, 5)], rects, r), "two rectangles of the default minimum size, one touching the corner")

        # --- identity: no colour augmentation drawn, no rectangle
        Ls = [picture(seed0 + 5, "idL%d" % b, 29, 43) for b in range(2)]
        Rs = [picture(seed0 + 5, "idR%d" % b, 29, 43) for b in range(2)]
        rows = [[par()] * 2, [par()] * 2]
        crops = [(2, 0), (5, 11)]
        r = run(tmp, Ls, Rs, (24, 32), rows, crops, [[], []], color=False)
        finish("augment_identity", pack(Ls, Rs, (24, 32), rows, crops, [[], []], r), "do_color_aug False")
    assert total < 700 * 1024, total
    lines.append("total %.0f KB" % (total / 1024))
    with open(os.path.join(OUT, "PROVENANCE_augment.txt"), "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


# ----------------------------------------------------------------------------------------------
def _warp_geometry(rng, B, H, W, kdim, small):
    """a camera and a rigid motion per batch element: focal length 0.8 W, principal point at the centre, a rotation of 0.05-0.2 rad
    about a random axis, a translation of length 0.1-0.4 (`small`: a twentieth of both, for a map of two rows), depth in [1, 9]"""
    k = 0.05 if small else 1.0
    K = np.zeros((B, kdim, kdim))
    T = np.zeros((B, 4, 4))
    for b in range(B):
        K[b] = np.eye(kdim)
        K[b, 0, 0] = K[b, 1, 1] = 0.8 * W
        K[b, 0, 2], K[b, 1, 2] = (W - 1) / 2.0, (H - 1) / 2.0
        axis = rng.normal(size=3)
        axis /= np.linalg.norm(axis)
        ang = k * rng.uniform(0.05, 0.2)
        S = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
        T[b] = np.eye(4)
        T[b, :3, :3] = np.eye(3) + np.sin(ang) * S + (1 - np.cos(ang)) * S @ S
        t = rng.normal(size=3)
        T[b, :3, 3] = t / np.linalg.norm(t) * k * rng.uniform(0.1, 0.4)
    depth = rng.uniform(1.0, 9.0, size=(B, 1, H, W))
    return K, T, depth


def warp_cases(M):
    """tests/golden/inverse_warp_*.npz: the reference's 2-D inverse_warp (layers/inverse_warp.py:6-77) on the CPU, in fp32 and fp64, on
    seeded inputs, for every mode and padding (bilinear); dev32_64 = max |fp32 run - fp64 run| per output."""
    from architecture.modeling.layers.inverse_warp import inverse_warp as ref_warp
    import warp_ref
    shapes = [("a", 2, 3, 7, 37, 7, 37, 3), ("b", 1, 5, 2, 66, 2, 66, 4), ("c", 2, 1, 9, 13, 5, 21, 3), ("e", 1, 17, 5, 4, 5, 4, 4)]
    lines = ["inverse_warp_*.npz: tools/gen_golden.py --only-warp, numpy %s, torch %s CPU -- the reference's own inverse_warp" % (np.__version__, torch.__version__),
             "(architecture/modeling/layers/inverse_warp.py:6-77, with the project_to_3d and mesh_grid it calls) run on seeded inputs in",
             "float32 and in float64, bilinear, for mode disparity / flow / depth x padding zeros / border / reflection.",
             "Inputs: img N(0,1); disparity and flow motions uniform in +-0.75 of the map's width resp. height (a third of the positions",
             "leave the image, some by more than one period of the reflection); depth mode: focal length 0.8 W, principal point at the",
             "centre, a rotation of 0.05-0.2 rad, a translation of 0.1-0.4 (a twentieth of both for the two-row map of inverse_warp_b, where",
             "nothing would stay inside otherwise), depth in [1, 9], inv_K = torch.inverse(K[:, :3, :3]) in fp32.",
             "The generator draws the depth geometry again (next seed) until no fp64 src_pixel_coord lies within 1e-4 px of a flow_mask",
             "bound (0, W-1, H-1) and the fp32 and fp64 masks are equal, and asserts both.",
             "Stored: the inputs, the float32 outputs out_<mode>_<padding> and, in depth mode, the five dictionary entries side_<key>;",
             "dev_* = max |fp32 run - fp64 run| of that output (dev32_64).  tests/warp_ref.py in fp64 agrees with the reference's fp64 run",
             "to 1e-12 on every output (asserted here)."]
    total = 0
    for tag, B, C, H, W, Hi, Wi, kdim in shapes:
        rng = np.random.default_rng(synth.SEED0 + 7000 + ord(tag))
        img = rng.normal(size=(B, C, Hi, Wi))
        disp = rng.uniform(-0.75, 0.75, size=(B, 1, H, W)) * W
        flow = rng.uniform(-0.75, 0.75, size=(B, 2, H, W)) * np.array([W, H]).reshape(1, 2, 1, 1)
        for attempt in range(200):
            grng = np.random.default_rng(synth.SEED0 + 7100 + 1000 * ord(tag) + attempt)
            K, Tm, depth = _warp_geometry(grng, B, H, W, kdim, small=H < 4)
            K32, T32, d32 = T(K).float(), T(Tm).float(), T(depth).float()
            iK32 = torch.inverse(K32[:, :3, :3])
            o32 = ref_warp(T(img).float(), d32, 'depth', K32, iK32, T32, output_all=True)[1]
            o64 = ref_warp(T(img), d32.double(), 'depth', K32.double(), iK32.double(), T32.double(), output_all=True)[1]
            c = o64['src_pixel_coord']
            gap = min(c[:, 0].abs().min(), (c[:, 0] - (W - 1)).abs().min(), c[:, 1].abs().min(), (c[:, 1] - (H - 1)).abs().min())
            if gap > 1e-4 and torch.equal(o32['flow_mask'], o64['flow_mask']):
                break
        assert gap > 1e-4 and torch.equal(o32['flow_mask'], o64['flow_mask']), (tag, float(gap))
        valid = float(o64['flow_mask'].float().mean())
        arrs = dict(img=T(img).float(), motion_disparity=T(disp).float(), motion_flow=T(flow).float(), motion_depth=d32, K=K32, inv_K=iK32, T=T32)
        devs = []
        for mode in ('disparity', 'flow', 'depth'):
            mot = arrs['motion_' + mode]
            geo32 = (K32, iK32, T32) if mode == 'depth' else (None, None, None)
            geo64 = tuple(g.double() for g in geo32) if mode == 'depth' else geo32
            for pad in ('zeros', 'border', 'reflection'):
                r32, s32 = ref_warp(arrs['img'], mot, mode, *geo32, 'bilinear', pad, output_all=True)
                r64, s64 = ref_warp(arrs['img'].double(), mot.double(), mode, *geo64, 'bilinear', pad, output_all=True)
                w64, ws64 = warp_ref.inverse_warp(arrs['img'].double(), mot.double(), mode, *geo64, 'bilinear', pad)
                assert (w64 - r64).abs().max() < 1e-12, (tag, mode, pad)
                arrs['out_%s_%s' % (mode, pad)] = r32
                arrs['dev_%s_%s' % (mode, pad)] = float((r32.double() - r64).abs().max())
                devs.append(arrs['dev_%s_%s' % (mode, pad)])
                if mode == 'depth' and pad == 'zeros':
                    assert sorted(s32) == ['flow_mask', 'homo_points_3d', 'optical_flow', 'src_pixel_coord', 'triangular_depth']
                    for k in s32:
                        arrs['side_' + k] = s32[k]
                        if k != 'flow_mask':
                            assert (ws64[k] - s64[k]).abs().max() < 1e-10, (tag, k)
                            arrs['dev_side_' + k] = float((s32[k].double() - s64[k]).abs().max())
                        else:
                            assert torch.equal(ws64[k], s64[k])
        save("inverse_warp_" + tag, **arrs)
        size = os.path.getsize(os.path.join(OUT, "inverse_warp_%s.npz" % tag))
        assert size < 100 * 1024, size
        total += size
        lines.append("inverse_warp_%s  B=%d C=%d motion %dx%d image %dx%d K %dx%d  dev32_64 of the warped image %.3g .. %.3g; depth: %.0f %% of the "
                     "pixels valid, geometry draw %d, nearest bound %.2e px; %.0f KB"
                     % (tag, B, C, H, W, Hi, Wi, kdim, kdim, min(devs), max(devs), 100 * valid, attempt, float(gap), size / 1024))
    lines.append("total %.0f KB" % (total / 1024))
    with open(os.path.join(OUT, "PROVENANCE_warp.txt"), "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


def raft_cases(M):
    """tests/golden/raft_corr_*.npz: the reference's own CorrBlock (aggregation/utils/raft_corr.py:4-67) on the CPU, in fp32 and fp64,
    forward and backward, on seeded inputs; dev_* = how far its fp32 run lies from its fp64 run."""
    from architecture.modeling.aggregation.utils.raft_corr import CorrBlock as RefCorrBlock
    import raft_ref
    shapes = [("a", 2, 6, 3, 37, 4, 4), ("b", 1, 5, 2, 66, 4, 4), ("c", 1, 40, 1, 8, 4, 1), ("e", 1, 32, 4, 64, 3, 2)]
    lines = ["raft_corr_*.npz: tools/gen_golden.py --only-raft, numpy %s, torch %s CPU -- the reference's own CorrBlock" % (np.__version__, torch.__version__),
             "(architecture/modeling/aggregation/utils/raft_corr.py:4-67) built and called on seeded inputs in float32 and in float64,",
             "with the backward of a seeded cotangent in both.",
             "Inputs: fmap1, fmap2 N(0,1), kept as their seed (tests/synth.py; raft_ref.load_fixture draws them again); disp uniform in [-0.2 W, 0.7 W]; the cotangent is k / 8 with k an integer in [-8, 8].",
             "The generator draws the disparity of single pixels again until, in the fp64 evaluation, no position xp of any level or",
             "tap lies within 1e-3 of an integer and floor(xp) agrees between the fp32 and the fp64 evaluation (the gradient with",
             "respect to disp has a kink at integer xp), and asserts both; it asserts that 50-95 % of the outputs are non-zero.",
             "Stored: seed and shape of the feature maps, disp, the float32 output `out`, the float32 pyramid levels `pyr_<i>` [B*H*W, W >> i], the cotangent",
             "`cot`, the gradients of the float32 run `grad_fmap1`, `grad_fmap2`, `grad_disp`; dev_out and dev_pyr_<i> = max |fp32 run -",
             "fp64 run| (the output compared in double: tests/raft_ref.py in fp64 stands for the fp64 run's output, which the",
             "reference casts to float32 at the end; the two agree to that cast, asserted here; the fp64 pyramid levels are the",
             "reference's own), rel_grad_* = relative L2 of the fp32 run's gradient against the fp64 run's."]
    total = 0
    for tag, B, C, H, W, L, r in shapes:
        rng = np.random.default_rng(synth.SEED0 + 8000 + ord(tag))
        seed = synth.SEED0 + 8000 + ord(tag)
        f1, f2 = (T(a) for a in raft_ref.fixture_features(seed, (B, C, H, W)))
        disp = T(rng.uniform(-0.2, 0.7, size=(B, 1, H, W)) * W).float()
        cot = T(rng.integers(-8, 9, size=(B, L * (2 * r + 1), H, W)) / 8.0).float()

        def bad_pixels(d):
            bad = torch.zeros(d.shape, dtype=torch.bool)
            gap = 1.0
            for i in range(L):
                x64 = raft_ref.positions(d.double(), i, r, W >> i)
                x32 = raft_ref.positions(d, i, r, W >> i)
                near = (x64 - torch.round(x64)).abs()
                gap = min(gap, float(near.min()))
                b = (near < 1e-3) | (torch.floor(x64) != torch.floor(x32.double()))
                bad |= b.any(dim=-1).unsqueeze(1)
            return bad, gap
        redrawn = 0
        for attempt in range(200):
            bad, gap = bad_pixels(disp)
            n = int(bad.sum())
            if n == 0:
                break
            redrawn += n
            disp[bad] = T(rng.uniform(-0.2, 0.7, size=n) * W).float()
        bad, gap = bad_pixels(disp)
        assert int(bad.sum()) == 0 and gap >= 1e-3, (tag, int(bad.sum()), gap)

        def run(dt):
            a, b_, d = (t.detach().clone().to(dt).requires_grad_(True) for t in (f1, f2, disp))
            blk = RefCorrBlock(a, b_, num_levels=L, radius=r)
            o = blk(d)
            o.backward(cot.to(o.dtype))
            return o.detach(), [lv.detach() for lv in blk.corr_pyramid], (a.grad, b_.grad, d.grad)
        o32, p32, g32 = run(torch.float32)
        o64f, p64, g64 = run(torch.float64)
        own64 = raft_ref.corr_block(f1.double(), f2.double(), disp.double(), L, r)
        assert o32.dtype == torch.float32 and o64f.dtype == torch.float32 and tuple(o32.shape) == (B, L * (2 * r + 1), H, W)
        scale = float(own64.abs().max())
        assert float((own64 - o64f.double()).abs().max()) <= 2.0 ** -24 * scale, (tag, float((own64 - o64f.double()).abs().max()))
        nz = float((o32 != 0).float().mean())
        assert 0.50 <= nz <= 0.95, (tag, nz)
        own_levels = raft_ref.corr_pyramid(f1.double(), f2.double(), L)
        arrs = dict(seed=seed, shape=np.array([B, C, H, W]), disp=disp, out=o32, cot=cot, grad_fmap1=g32[0], grad_fmap2=g32[1], grad_disp=g32[2],
                    num_levels=L, radius=r, dev_out=float((o32.double() - own64).abs().max()))
        for i in range(L):
            assert tuple(p32[i].shape) == (B * H * W, 1, 1, W >> i)
            assert float((own_levels[i].reshape(p64[i].shape) - p64[i]).abs().max()) < 1e-12, (tag, i)
            arrs["pyr_%d" % i] = p32[i].reshape(B * H * W, W >> i)
            arrs["dev_pyr_%d" % i] = float((p32[i].double() - p64[i]).abs().max())
        rels = []
        for name, a, b_ in zip(("fmap1", "fmap2", "disp"), g32, g64):
            arrs["rel_grad_" + name] = float((a.double() - b_).norm() / b_.norm())
            rels.append(arrs["rel_grad_" + name])
        save("raft_corr_" + tag, **arrs)
        size = os.path.getsize(os.path.join(OUT, "raft_corr_%s.npz" % tag))
        total += size
        lines.append("raft_corr_%s  B=%d C=%d H=%d W=%d L=%d r=%d  %.0f %% of the outputs non-zero, %d disparities drawn again, nearest "
                     "integer %.2e; dev_out %.3g, dev_pyr %.3g .. %.3g, rel_grad fmap1 %.3g fmap2 %.3g disp %.3g; %.0f KB"
                     % (tag, B, C, H, W, L, r, 100 * nz, redrawn, gap, arrs["dev_out"], min(arrs["dev_pyr_%d" % i] for i in range(L)),
                        max(arrs["dev_pyr_%d" % i] for i in range(L)), rels[0], rels[1], rels[2], size / 1024))
    assert total < 400 * 1024, total
    lines.append("total %.0f KB" % (total / 1024))
    with open(os.path.join(OUT, "PROVENANCE_raft.txt"), "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


def flow_cases(M):
    """tests/golden/flow_corr_*.npz: the reference's own FlowCorrBlock (aggregation/utils/raft_corr.py:71-160) on the CPU, in fp32 and
    fp64, forward and backward, on seeded inputs; dev_* = how far its fp32 run lies from its fp64 run."""
    from architecture.modeling.aggregation.utils.raft_corr import FlowCorrBlock as RefFlowCorrBlock
    import flow_corr_ref
    shapes = [("a", 2, 6, 8, 11, 3, 2), ("c", 1, 40, 4, 4, 2, 1), ("e", 1, 32, 8, 16, 3, 3)]
    lines = ["flow_corr_*.npz: tools/gen_golden.py --only-flow, numpy %s, torch %s CPU -- the reference's own FlowCorrBlock" % (np.__version__, torch.__version__),
             "(architecture/modeling/aggregation/utils/raft_corr.py:71-160) built and called on seeded inputs in float32 and in float64,",
             "with the backward of a seeded cotangent in both.",
             "Inputs: fmap1, fmap2 N(0,1), kept as their seed (tests/synth.py; flow_corr_ref.load_fixture draws them again); coords = the pixel grid (x, y) plus a flow uniform in +-0.25 (W, H); the cotangent is k / 8 with k an integer in [-8, 8].",
             "The generator draws the flow of single pixels again until, in the fp64 evaluation, no sample position of any level or",
             "tap lies within 1e-3 of an integer in x or in y and the floors agree between the fp32 and the fp64 evaluation (the",
             "gradient with respect to coords has a kink at integer positions), and asserts both; it asserts that 40-95 % of the outputs are non-zero.",
             "Stored: seed and shape of the feature maps, coords, the float32 output `out`, the float32 pyramid levels `pyr_<i>` [B*H*W, (H >> i)*(W >> i)], the cotangent",
             "`cot`, the gradients of the float32 run `grad_fmap1`, `grad_fmap2`, `grad_coords`; dev_out and dev_pyr_<i> = max |fp32 run -",
             "fp64 run| (the output compared in double: tests/flow_corr_ref.py in fp64 stands for the fp64 run's output, which the",
             "reference casts to float32 at the end; the two agree to that cast, asserted here; the fp64 pyramid levels are the",
             "reference's own), rel_grad_* = relative L2 of the fp32 run's gradient against the fp64 run's."]
    total = 0
    for tag, B, C, H, W, L, r in shapes:
        seed = synth.SEED0 + 9000 + ord(tag)
        rng = np.random.default_rng(seed)
        f1, f2 = (T(a) for a in flow_corr_ref.fixture_features(seed, (B, C, H, W)))
        grid = RefFlowCorrBlock.init_flow((B, C, H, W), "cpu")[1].clone()
        span = torch.tensor([W, H], dtype=torch.float64).view(1, 2, 1, 1)

        def draw(n):
            return T(rng.uniform(-0.25, 0.25, size=(n, 2))) * span.view(1, 2)
        coords = (grid.double() + draw(B * H * W).view(B, H, W, 2).permute(0, 3, 1, 2)).float()
        cot = T(rng.integers(-8, 9, size=(B, L * (2 * r + 1) ** 2, H, W)) / 8.0).float()

        def bad_pixels(c):
            bad = torch.zeros((B, H, W), dtype=torch.bool)
            gap = 1.0
            for i in range(L):
                p64 = flow_corr_ref.positions(c.double(), i, r, H >> i, W >> i)
                p32 = flow_corr_ref.positions(c, i, r, H >> i, W >> i)
                for a64, a32 in zip(p64, p32):
                    near = (a64 - torch.round(a64)).abs()
                    gap = min(gap, float(near.min()))
                    bad |= ((near < 1e-3) | (torch.floor(a64) != torch.floor(a32.double()))).any(dim=-1)
            return bad, gap
        redrawn = 0
        for attempt in range(200):
            bad, gap = bad_pixels(coords)
            n = int(bad.sum())
            if n == 0:
                break
            redrawn += n
            fresh = (grid.double().permute(0, 2, 3, 1)[bad] + draw(n)).float()
            cp = coords.permute(0, 2, 3, 1).contiguous()
            cp[bad] = fresh
            coords = cp.permute(0, 3, 1, 2).contiguous()
        bad, gap = bad_pixels(coords)
        assert int(bad.sum()) == 0 and gap >= 1e-3, (tag, int(bad.sum()), gap)

        def run(dt):
            a, b_, c = (t.detach().clone().to(dt).requires_grad_(True) for t in (f1, f2, coords))
            blk = RefFlowCorrBlock(a, b_, num_levels=L, radius=r)
            o = blk(c)
            o.backward(cot.to(o.dtype))
            return o.detach(), [lv.detach() for lv in blk.corr_pyramid], (a.grad, b_.grad, c.grad)
        o32, p32, g32 = run(torch.float32)
        o64f, p64, g64 = run(torch.float64)
        own64 = flow_corr_ref.flow_corr_block(f1.double(), f2.double(), coords.double(), L, r)
        assert o32.dtype == torch.float32 and o64f.dtype == torch.float32 and tuple(o32.shape) == (B, L * (2 * r + 1) ** 2, H, W)
        scale = float(own64.abs().max())
        assert float((own64 - o64f.double()).abs().max()) <= 2.0 ** -24 * scale, (tag, float((own64 - o64f.double()).abs().max()))
        nz = float((o32 != 0).float().mean())
        assert 0.40 <= nz <= 0.95, (tag, nz)
        own_levels = flow_corr_ref.corr_pyramid(f1.double(), f2.double(), L)
        arrs = dict(seed=seed, shape=np.array([B, C, H, W]), coords=coords, out=o32, cot=cot, grad_fmap1=g32[0], grad_fmap2=g32[1], grad_coords=g32[2],
                    num_levels=L, radius=r, dev_out=float((o32.double() - own64).abs().max()))
        for i in range(L):
            assert tuple(p32[i].shape) == (B * H * W, 1, H >> i, W >> i)
            assert float((own_levels[i].reshape(p64[i].shape) - p64[i]).abs().max()) < 1e-12, (tag, i)
            arrs["pyr_%d" % i] = p32[i].reshape(B * H * W, (H >> i) * (W >> i))
            arrs["dev_pyr_%d" % i] = float((p32[i].double() - p64[i]).abs().max())
        rels = []
        for name, a, b_ in zip(("fmap1", "fmap2", "coords"), g32, g64):
            arrs["rel_grad_" + name] = float((a.double() - b_).norm() / b_.norm())
            rels.append(arrs["rel_grad_" + name])
        save("flow_corr_" + tag, **arrs)
        size = os.path.getsize(os.path.join(OUT, "flow_corr_%s.npz" % tag))
        assert size <= 200 * 1024, (tag, size)
        total += size
        lines.append("flow_corr_%s  B=%d C=%d H=%d W=%d L=%d r=%d  %.0f %% of the outputs non-zero, %d flows drawn again, nearest "
                     "integer %.2e; dev_out %.3g, dev_pyr %.3g .. %.3g, rel_grad fmap1 %.3g fmap2 %.3g coords %.3g; %.0f KB"
                     % (tag, B, C, H, W, L, r, 100 * nz, redrawn, gap, arrs["dev_out"], min(arrs["dev_pyr_%d" % i] for i in range(L)),
                        max(arrs["dev_pyr_%d" % i] for i in range(L)), rels[0], rels[1], rels[2], size / 1024))
    lines.append("total %.0f KB" % (total / 1024))
    with open(os.path.join(OUT, "PROVENANCE_flow.txt"), "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


def spp3d_cases(M):
    """tests/golden/spp3d_*.npz: the reference's own SPP3D (aggregation/utils/SPP3D.py:8-49) on the CPU, in fp32 and fp64, forward and the
    backward of a seeded cotangent; dev_* = how far its fp32 run lies from its fp64 run, stage by stage."""
    from architecture.modeling.aggregation.utils.SPP3D import SPP3D as RefSPP3D
    import spp3d_ref
    strides = (2, 4, 8, 16)
    L = len(strides)
    shapes = [("a", (2, 8, 5, 6, 7), True), ("b", (1, 8, 18, 17, 35), True), ("c", (2, 32, 3, 9, 20), True), ("d", (1, 8, 1, 2, 2), False)]
    lines = ["spp3d_*.npz: tools/gen_golden.py --only-spp3d, numpy %s, torch %s CPU -- the reference's own SPP3D" % (np.__version__, torch.__version__),
             "(architecture/modeling/aggregation/utils/SPP3D.py:8-49), strides (2, 4, 8, 16), norm 'BN3d', activation 'ReLU', built and called on",
             "seeded inputs in float32 and in float64, with the backward of a seeded cotangent in both (train mode; the eval fixture has no backward).",
             "Inputs, all kept as their seed (tests/spp3d_ref.py fixture_input / fixture_state / fixture_cotangent draw them again):",
             "x = N(0,1) noise + per (batch, channel) an offset N(0,1) + along every axis of more than one plane a ramp a * 2 * (i / (n - 1) - 0.5),",
             "a uniform in [-2, 2] per (batch, channel, axis) (so the means over large boxes differ at order one: a BatchNorm over the two values a",
             "channel has at the coarsest level divides by their distance); parameters and buffers by synth.state_values, except that the",
             "convolution weights are doubled and every BatchNorm bias is sign * m * (that BatchNorm's weight), sign +-1 with equal chance and m",
             "uniform in [1.5, 2.5] per channel (a channel's ReLU is mostly open or mostly shut, so few of a stage's ~10^5 pre-activations lie near",
             "zero: with the plain N(0, 0.1) bias no seed in 2000 met the margin rule below); the cotangent k / 8 with k an integer in [-8, 8].",
             "Train fixtures: the seed is drawn again until, at every ReLU (the L levels and fuse.0), the fp32 and the fp64 run have the same mask",
             "and the smallest |pre-activation| of the fp64 run is >= 32 x that stage's max |fp32 - fp64|; every BatchNorm sees >= 2 values per",
             "channel.  All three are asserted.",
             "Stored: seed, shape, strides, training, keys (the reference's state-dict keys in order), out, pooled_<i> (the avg_pool3d results),",
             "cat_idx / cat_val (the concatenation's level channels cat[:, C:]: all of them up to 8192 elements, else 8192 seeded flat",
             "positions), grad_x, grad_<parameter key>, stat_<buffer key> (running statistics and num_batches_tracked after the step),",
             "dev_out / dev_cat / dev_pooled_<i> / dev_stat_<key> = max |fp32 run - fp64 run|, rel_grad_<key> = relative L2 of the fp32 run's",
             "gradient against the fp64 run's, min_pre_<j> / dev_pre_<j> = the margin figures per ReLU."]
    total = 0
    for tag, shape, training in shapes:
        B, C, D, H, W = shape
        base = synth.SEED0 + 11000 + 1000 * ord(tag)

        def run(seed, dt):
            ref = RefSPP3D(in_planes=C, strides=strides, norm='BN3d', activation='ReLU')
            state = spp3d_ref.fixture_state(seed, C, L, dt)
            missing = ref.load_state_dict(state, strict=True)
            assert not missing.missing_keys and not missing.unexpected_keys
            ref = ref.to(dt).train(training)
            grab = dict(pre=[], pooled=[], cat=[])
            hooks = []
            for p in ref.pools:
                hooks.append(p.register_forward_pre_hook(lambda m, a: grab["pooled"].append(a[0].detach().clone())))
                hooks.append(p.norm.register_forward_hook(lambda m, a, o: grab["pre"].append(o.detach().clone())))
            hooks.append(ref.fuse[0].register_forward_pre_hook(lambda m, a: grab["cat"].append(a[0].detach().clone())))
            hooks.append(ref.fuse[0].norm.register_forward_hook(lambda m, a, o: grab["pre"].append(o.detach().clone())))
            x = spp3d_ref.fixture_input(seed, shape, dt).requires_grad_(training)
            out = ref(x)
            grads = {}
            if training:
                out.backward(spp3d_ref.fixture_cotangent(seed, out.shape, dt))
                grads = {k: p.grad.detach() for k, p in ref.named_parameters()}
                grads["x"] = x.grad.detach()
            for h in hooks:
                h.remove()
            stats = {k: v.detach().clone() for k, v in ref.state_dict().items() if "running_" in k or "num_batches" in k}
            return out.detach(), grab, grads, stats, list(ref.state_dict().keys())

        for attempt in range(2000):
            seed = base + attempt
            o32, g32, d32, s32, keys = run(seed, torch.float32)
            o64, g64, d64, s64, _ = run(seed, torch.float64)
            margins = []
            ok = True
            for j, (p32, p64) in enumerate(zip(g32["pre"], g64["pre"])):
                dev = float((p32.double() - p64).abs().max())
                low = float(p64.abs().min())
                same = bool(((p32 > 0) == (p64 > 0)).all())
                margins.append((low, dev))
                ok = ok and same and low >= 32 * dev
                if training:
                    assert p64.numel() // p64.shape[1] >= 2, (tag, j)
            if ok or not training:
                break
        assert ok or not training, tag
        if training:
            for low, dev in margins:
                assert low >= 32 * dev
        # the restatement stands where the reference stands
        own = spp3d_ref.spp3d(spp3d_ref.fixture_input(seed, shape, torch.float64), spp3d_ref.fixture_state(seed, C, L, torch.float64), strides, training)
        assert float((own["out"] - o64).abs().max()) <= 1e-10 * max(1.0, float(o64.abs().max())), (tag, float((own["out"] - o64).abs().max()))
        cat32, cat64 = g32["cat"][0][:, C:], g64["cat"][0][:, C:]
        n = cat32.numel()
        idx = np.arange(n) if n <= 8192 else np.sort(np.random.RandomState(seed % (2 ** 32)).choice(n, 8192, replace=False))
        arrs = dict(seed=seed, shape=np.array(shape), strides=np.array(strides), training=training, keys=np.array(keys), out=o32,
                    cat_idx=idx.astype(np.int32), cat_val=spp3d_ref.sample(cat32, idx), dev_out=float((o32.double() - o64).abs().max()),
                    dev_cat=float((cat32.double() - cat64).abs().max()), attempts=attempt + 1)
        for i in range(L):
            arrs["pooled_%d" % i] = g32["pooled"][i]
            arrs["dev_pooled_%d" % i] = float((g32["pooled"][i].double() - g64["pooled"][i]).abs().max())
        for j, (low, dev) in enumerate(margins):
            arrs["min_pre_%d" % j], arrs["dev_pre_%d" % j] = low, dev
        rels = []
        for k in d32:
            arrs["grad_" + k] = d32[k]
            arrs["rel_grad_" + k] = float((d32[k].double() - d64[k]).norm() / d64[k].norm())
            rels.append(arrs["rel_grad_" + k])
        for k in s32:
            arrs["stat_" + k] = s32[k]
            arrs["dev_stat_" + k] = float((s32[k].double() - s64[k].double()).abs().max())
        size = save_fixed("spp3d_" + tag, **arrs)
        assert size <= 1024 * 1024, (tag, size)
        total += size
        lines.append("spp3d_%s  B=%d C=%d D=%d H=%d W=%d %s  seed %d (draw %d); levels %s; dev_out %.3g dev_cat %.3g dev_pooled <= %.3g; "
                     "min |pre| / dev per ReLU %s; rel_grad %s; %.0f KB"
                     % (tag, B, C, D, H, W, "train" if training else "eval", seed, attempt + 1, spp3d_ref.level_sizes((D, H, W), strides),
                        arrs["dev_out"], arrs["dev_cat"], max(arrs["dev_pooled_%d" % i] for i in range(L)),
                        " ".join("%.2e/%.1e" % m for m in margins),
                        ("%.3g .. %.3g" % (min(rels), max(rels))) if rels else "-", size / 1024))
    lines.append("total %.0f KB (out and grad_x of shape b, the one with a remainder on every axis, are 343 KB each)" % (total / 1024))
    with open(os.path.join(OUT, "PROVENANCE_spp3d.txt"), "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


def conv_gru_cases(M):
    """tests/golden/conv_gru_*.npz: the reference's own ConvGRU (layers/conv_gru.py:4-28) on the CPU, in fp32 and fp64: one step with
    its gates, three chained steps, and the backward of a seeded cotangent; dev_* = how far its fp32 run lies from its fp64 run."""
    import importlib.util
    import conv_gru_ref
    spec = importlib.util.spec_from_file_location("ref_conv_gru", os.path.join(ref_import.REFERENCE_ROOT, "architecture", "modeling", "layers",
                                                                               "conv_gru.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    RefConvGRU = mod.ConvGRU
    shapes = [("a", (2, 12, 5, 9, 37), True), ("b", (1, 32, 48, 17, 70), True), ("c", (2, 64, 64, 6, 20), True), ("d", (1, 8, 8, 1, 1), False)]
    lines = ["conv_gru_*.npz: tools/gen_golden.py --only-convgru, numpy %s, torch %s CPU -- the reference's own ConvGRU" % (np.__version__, torch.__version__),
             "(architecture/modeling/layers/conv_gru.py:4-28), built and called on seeded inputs in float32 and in float64: one step (the gates",
             "taken from forward hooks on convz / convr / convq), three chained steps in which the output is the next last_hidden and x stays",
             "the same, and the backward of a seeded cotangent of the third output in both (shape d: forward only).",
             "Inputs, all kept as their seed (tests/conv_gru_ref.py fixture_state / fixture_input / fixture_cotangent draw them again):",
             "convolution weights N(0,1) * 2 / sqrt(9 (Ch + Cx)), biases N(0, 0.5), last_hidden = tanh(N(0,1)), x = N(0,1), the cotangent k / 8",
             "with k an integer in [-8, 8].  On shapes with at least 1000 gate values the seed is drawn again until z and r of the fp64 run each go",
             "below 0.05 and above 0.95 (asserted).",
             "Stored: seed, shape (B, Ch, Cx, H, W), keys (the reference's state-dict keys in order), z, r, q, out (one step, fp32), out3, grad_h,",
             "grad_x, grad_<parameter key>; an array of more than %d elements is stored at %d seeded flat positions (conv_gru_ref.sample)." % (conv_gru_ref.SAMPLE, conv_gru_ref.SAMPLE),
             "dev_<stage> = max |fp32 run - fp64 run| and rel_grad_<key> = relative L2 of the fp32 run's gradient against the fp64 run's, both over",
             "the WHOLE arrays; max_<stage> = max |stage| of the fp64 run."]
    total = 0
    for tag, shape, backward in shapes:
        B, Ch, Cx, H, W = shape
        base = synth.SEED0 + 12000 + 1000 * ord(tag)

        def run(seed, dt):
            ref = RefConvGRU(Cx, Ch)
            missing = ref.load_state_dict(conv_gru_ref.fixture_state(seed, Ch, Cx, dt), strict=True)
            assert not missing.missing_keys and not missing.unexpected_keys
            ref = ref.to(dt)
            grab = {}
            def keep(name):
                def hook(m, a, o):
                    grab[name] = o.detach().clone()           # (returns None: the output is not replaced)
                return hook
            hooks = [getattr(ref, n).register_forward_hook(keep(n)) for n in ("convz", "convr", "convq")]
            h, x = conv_gru_ref.fixture_input(seed, shape, dt)
            h.requires_grad_(backward)
            x.requires_grad_(backward)
            out = ref(h, x)
            res = dict(z=torch.sigmoid(grab["convz"]), r=torch.sigmoid(grab["convr"]), q=torch.tanh(grab["convq"]), out=out.detach())
            for hk in hooks:
                hk.remove()
            out3 = ref(ref(out, x), x)
            res["out3"] = out3.detach()
            if backward:
                out3.backward(conv_gru_ref.fixture_cotangent(seed, out3.shape, dt))
                res["grad_h"], res["grad_x"] = h.grad.detach(), x.grad.detach()
                for k, p in ref.named_parameters():
                    res["grad_" + k] = p.grad.detach()
            return res, list(ref.state_dict().keys())

        for attempt in range(200):
            seed = base + attempt
            r32, keys = run(seed, torch.float32)
            r64, _ = run(seed, torch.float64)
            wide = all(float(r64[g].min()) < 0.05 and float(r64[g].max()) > 0.95 for g in ("z", "r"))
            if wide or r64["z"].numel() < 1000:
                break
        assert wide or r64["z"].numel() < 1000, tag
        assert keys == list(conv_gru_ref.KEYS)
        # the restatement stands where the reference stands
        own = conv_gru_ref.run(seed, shape, torch.float64, backward)
        for k in r64:
            assert float((own[k] - r64[k]).abs().max()) <= 1e-10 * max(1.0, float(r64[k].abs().max())), (tag, k, float((own[k] - r64[k]).abs().max()))
        arrs = dict(seed=seed, shape=np.array(shape), keys=np.array(keys), attempts=attempt + 1)
        rels = []
        for k in r32:
            arrs[k] = conv_gru_ref.sample(r32[k], seed)
            if k.startswith("grad_"):
                arrs["rel_" + k] = float((r32[k].double() - r64[k]).norm() / r64[k].norm())
                rels.append(arrs["rel_" + k])
            else:
                arrs["dev_" + k] = float((r32[k].double() - r64[k]).abs().max())
                arrs["max_" + k] = float(r64[k].abs().max())
        size = save_fixed("conv_gru_" + tag, **arrs)
        assert size <= 754 * 1024, (tag, size)
        total += size
        lines.append("conv_gru_%s  B=%d Ch=%d Cx=%d H=%d W=%d  seed %d (draw %d); z %.3f .. %.3f, r %.3f .. %.3f; dev z %.3g r %.3g q %.3g out %.3g "
                     "out3 %.3g; rel_grad %s; %.0f KB"
                     % (tag, B, Ch, Cx, H, W, seed, attempt + 1, float(r64["z"].min()), float(r64["z"].max()), float(r64["r"].min()),
                        float(r64["r"].max()), arrs["dev_z"], arrs["dev_r"], arrs["dev_q"], arrs["dev_out"], arrs["dev_out3"],
                        ("%.3g .. %.3g" % (min(rels), max(rels))) if rels else "-", size / 1024))
    lines.append("total %.0f KB" % (total / 1024))
    with open(os.path.join(OUT, "PROVENANCE_conv_gru.txt"), "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


def reference_decoder():
    """The reference's OWN decoder (architecture/modeling/backbone/TemporalStereo.py), compiled from its file's syntax tree -- the
    module imports timm at the top, which this image does not have.  `build(self, norm, activation)` is the statements of `__init__`
    from `channels = [...]` on (:74-90), run against the reference's own Conv2d; `decode(self, x4, x8, x16, x32)` is the statements of
    `_forward` from `x32 = self.conv32(x32)` up to its return (:125-138)."""
    import ast
    import torch.nn as nn
    import torch.nn.functional as F
    from architecture.modeling.layers import Conv2d, ConvTranspose2d
    path = os.path.join(ref_import.REFERENCE_ROOT, "architecture", "modeling", "backbone", "TemporalStereo.py")
    tree = ast.parse(open(path).read(), filename=path)
    cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "TEMPORALSTEREO")
    init = next(n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name == "__init__")
    fwd = next(n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name == "_forward")

    def targets(stmt):
        return {ast.unparse(t) for t in stmt.targets} if isinstance(stmt, ast.Assign) else set()
    at = next(i for i, s in enumerate(init.body) if "channels" in targets(s))
    build = ast.parse("def build(self, norm, activation):\n    pass").body[0]
    build.body = init.body[at:]
    assert {"self.conv32", "self.deconv32_16", "self.deconv16_8", "self.deconv8_4"} <= set().union(*map(targets, build.body))
    at = next(i for i, s in enumerate(fwd.body) if "x32" in targets(s) and "self.conv32" in ast.unparse(s))
    assert isinstance(fwd.body[-1], ast.Return)
    decode = ast.parse("def decode(self, x4, x8, x16, x32):\n    pass\n    return [x4, x8, x16]").body[0]
    decode.body[0:1] = fwd.body[at:-1]
    assert len(decode.body) == 11, len(decode.body)            # conv32, then three times (h, w / interpolate / cat + pair), return
    ns = {"torch": torch, "nn": nn, "F": F, "Conv2d": Conv2d, "ConvTranspose2d": ConvTranspose2d}
    exec(compile(ast.fix_missing_locations(ast.Module(body=[build, decode], type_ignores=[])), path, "exec"), ns)
    return ns["build"], ns["decode"]


def decoder_cases(M):
    """tests/golden/decoder_*.npz: the reference's own decoder lines on submodules built by its own Conv2d, on the CPU, in fp32 and
    fp64, train mode and eval mode; dev_* = how far its fp32 run lies from its fp64 run."""
    import torch.nn as nn
    import decoder_ref as R
    build, decode = reference_decoder()
    lines = ["decoder_*.npz: tools/gen_golden.py --only-decoder, numpy %s, torch %s CPU -- the reference's own decoder" % (np.__version__, torch.__version__),
             "(architecture/modeling/backbone/TemporalStereo.py: the statements of __init__ :74-90 and of _forward :125-138, compiled from the",
             "file's syntax tree; the submodules are built by the reference's own Conv2d with norm 'BN' and activation 'SiLU') on seeded inputs in",
             "float32 and in float64, in train mode and in eval mode, with the backward of seeded cotangents of the three outputs.",
             "Inputs, all kept as their seed (tests/decoder_ref.py fixture_state / fixture_input / fixture_cotangents draw them again): convolution",
             "weights N(0,1) * 2 / sqrt(9 Cin), BatchNorm weight U(0.5, 1.5) and bias N(0, 0.1), running mean N(0, 0.1), running variance",
             "U(0.5, 1.5), the four maps N(0,1), the cotangents k / 8 with k an integer in [-8, 8].",
             "Stored: seed, keys and key_shapes (the reference's state-dict keys of the four submodules in order, their shapes padded with -1),",
             "and per mode m in (train, eval) the deviations of EVERY output and gradient: dev_<m>_<x4|x8|x16> = max |fp32 run - fp64 run|,",
             "max_<m>_<...> = max |output| of the fp64 run, rel_grad_<m>_<x4|x8|x16|x32|parameter key> = relative L2 of the fp32 run's gradient",
             "against the fp64 run's, all over the WHOLE arrays.  Arrays (fp32 run; one of more than %d elements at %d seeded flat positions," % (R.SAMPLE, R.SAMPLE),
             "decoder_ref.sample): train mode <m>_<output>, grad_<m>_<input>, grad_<m>_<parameter key>; eval mode eval_x4 alone -- the last",
             "output, behind every layer.  The eval-mode arrays left out (two outputs, 17 gradients, ~440 KB per geometry) would take the two",
             "files to 1.8 MB; the tests compare eval mode against the fp64 restatement, with the stored deviations as bars."]
    total = 0
    for tag in ("a", "b"):
        seed = synth.SEED0 + 13000 + 1000 * ord(tag)
        ins, outs = R.geometry_shapes(tag)

        def run(dt, training):
            me = nn.Module()
            build(me, "BN", "SiLU")
            keys = list(me.state_dict().keys())
            shapes = [tuple(v.shape) for v in me.state_dict().values()]
            res = me.load_state_dict(R.fixture_state(seed), strict=True)
            assert not res.missing_keys and not res.unexpected_keys
            me = me.to(dt).train(training)
            maps = R.fixture_input(seed, tag, dt)
            for t in maps.values():
                t.requires_grad_(True)
            got = dict(zip(R.OUTPUTS, decode(me, maps["x4"], maps["x8"], maps["x16"], maps["x32"])))
            cots = R.fixture_cotangents(seed, tag, dt)
            torch.autograd.backward([got[k] for k in R.OUTPUTS], [cots[k] for k in R.OUTPUTS])
            out = {k: v.detach() for k, v in got.items()}
            for k in R.INPUTS:
                out["grad_" + k] = maps[k].grad.detach()
            for k, p in me.named_parameters():
                out["grad_" + k] = p.grad.detach()
            return out, keys, shapes

        arrs = dict(seed=seed)
        note = []
        for mode in R.MODES:
            training = mode == "train"
            r32, keys, shapes = run(torch.float32, training)
            r64, _, _ = run(torch.float64, training)
            assert keys == list(R.KEYS) and shapes == [s for _, s in R.key_shapes()]
            assert {k[5:] for k in r32 if k.startswith("grad_")} == set(R.INPUTS) | set(R.PARAM_KEYS)
            own = R.run(seed, tag, torch.float64, training)            # the restatement stands where the reference stands
            for k in r64:
                assert float((own[k] - r64[k]).abs().max()) <= 1e-10 * max(1.0, float(r64[k].abs().max())), (tag, mode, k)
            devs, rels = [], []
            for k in r32:
                if k.startswith("grad_"):
                    name = k[5:]
                    arrs["rel_grad_%s_%s" % (mode, name)] = float((r32[k].double() - r64[k]).norm() / r64[k].norm())
                    rels.append(arrs["rel_grad_%s_%s" % (mode, name)])
                    if training:
                        arrs["grad_%s_%s" % (mode, name)] = R.sample(r32[k], seed)
                else:
                    arrs["dev_%s_%s" % (mode, k)] = float((r32[k].double() - r64[k]).abs().max())
                    arrs["max_%s_%s" % (mode, k)] = float(r64[k].abs().max())
                    devs.append(arrs["dev_%s_%s" % (mode, k)])
                    if training or k == "x4":
                        arrs["%s_%s" % (mode, k)] = R.sample(r32[k], seed)
            note.append("%s: dev %.3g .. %.3g, rel_grad %.3g .. %.3g" % (mode, min(devs), max(devs), min(rels), max(rels)))
        arrs["keys"] = np.array(keys)
        arrs["key_shapes"] = np.array([list(s) + [-1] * (4 - len(s)) for s in shapes], dtype=np.int64)
        size = save_fixed("decoder_" + tag, **arrs)
        total += size
        B = R.GEOMETRIES[tag][0]
        lines.append("decoder_%s  B=%d x32 %dx%d x16 %dx%d x8 %dx%d x4 %dx%d  seed %d; %s; %.0f KB"
                     % ((tag, B) + tuple(v for p in R.GEOMETRIES[tag][1:] for v in p) + (seed, "; ".join(note), size / 1024)))
    lines.append("total %.0f KB" % (total / 1024))
    assert total < 1000 * 1000, total
    with open(os.path.join(OUT, "PROVENANCE_decoder.txt"), "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


def reference_mbconv(block_class):
    """The reference's OWN `_inverted_residual_forward` and `_block_forward` (architecture/modeling/backbone/TemporalStereo.py:165-218),
    compiled from its file's syntax tree -- the module imports timm at the top, which this image does not have.  The name
    `InvertedResidual` (the isinstance test of `_block_forward`) is bound to `block_class`, `drop_path` to a function that must not be
    called (the stand-in's drop_path_rate is 0)."""
    import ast
    path = os.path.join(ref_import.REFERENCE_ROOT, "architecture", "modeling", "backbone", "TemporalStereo.py")
    tree = ast.parse(open(path).read(), filename=path)
    names = ("_block_forward", "_inverted_residual_forward")
    funcs = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in names]
    assert sorted(f.name for f in funcs) == sorted(names)

    def drop_path(*a, **k):
        raise AssertionError("drop_path must not be reached: the stand-in's drop_path_rate is 0")
    ns = {"torch": torch, "InvertedResidual": block_class, "drop_path": drop_path}
    exec(compile(ast.fix_missing_locations(ast.Module(body=funcs, type_ignores=[])), path, "exec"), ns)
    return ns["_inverted_residual_forward"], ns["_block_forward"]


def mbconv_cases(M):
    """tests/golden/mbconv_*.npz: the reference's own memory-block function and stage walk on tests/mbconv_ref.py's stand-in block, on
    the CPU, in fp32 and fp64, train mode and eval mode; dev_* = how far its fp32 run lies from its fp64 run."""
    import mbconv_ref as R
    block_fwd, stage_fwd = reference_mbconv(R.StandInBlock)
    lines = ["mbconv_*.npz: tools/gen_golden.py --only-mbconv, numpy %s, torch %s CPU -- the reference's own _inverted_residual_forward and" % (np.__version__, torch.__version__),
             "_block_forward (architecture/modeling/backbone/TemporalStereo.py:165-218, compiled from the file's syntax tree with the name",
             "InvertedResidual bound to tests/mbconv_ref.py's StandInBlock -- timm, where the reference's block comes from, is not part of its",
             "checkout -- and drop_path to a function that raises) on seeded inputs in float32 and in float64, in train mode and in eval mode,",
             "with the backward of seeded cotangents of every frame's output.  A case is a stage nn.Sequential(nn.Sequential(block, ...)) walked",
             "by _block_forward once per frame, memory_percent 1/4; a single-block, single-frame case is ALSO run through",
             "_inverted_residual_forward directly and the two runs are asserted identical.",
             "Inputs, all kept as their seed (tests/mbconv_ref.py fixture_state / fixture_inputs / fixture_memory / fixture_cotangents draw them",
             "again): convolution weights N(0,1) * 2 / sqrt(fan-in), convolution biases N(0, 0.1), BatchNorm weight U(0.5, 1.5) and bias N(0, 0.1),",
             "running mean N(0, 0.1), running variance U(0.5, 1.5), inputs and memory N(0,1), cotangents k / 8 with k an integer in [-8, 8].",
             "Stored: seed, keys and key_shapes (the stage's state-dict keys in order, shapes padded with -1), and per mode m in (train, eval) the",
             "deviations of EVERY output, stage and gradient over the WHOLE arrays: dev_<m>_f<frame>_out, dev_<m>_f<frame>_b<block>_<act1|act2|gate>",
             "= max |fp32 run - fp64 run|, max_<m>_<...> = max |.| of the fp64 run, rel_grad_<m>_<in_f<frame>|memory|parameter key> = relative L2",
             "of the fp32 run's gradient against the fp64 run's.  Arrays (fp32 run; one of more than %d elements at %d seeded flat positions," % (R.SAMPLE, R.SAMPLE),
             "mbconv_ref.sample): those mbconv_ref.stored names -- train mode the outputs and the gradients of inputs, memory and the three",
             "convolution weights; eval mode the outputs, act2 and the gate.  The rest would take the four files past 1 MB; the tests compare",
             "everything against the fp64 restatement, which the generator asserts equal to the reference's fp64 run to 1e-10."]
    total = 0
    for tag in R.TAGS:
        c = R.CASES[tag]
        seed = synth.SEED0 + 15000 + 1000 * ord(tag)

        def run(dt, training):
            net = R.stand_in_stage(tag)
            keys = list(net.state_dict().keys())
            shapes = [tuple(v.shape) for v in net.state_dict().values()]
            res = net.load_state_dict(R.fixture_state(seed, tag), strict=True)
            assert not res.missing_keys and not res.unexpected_keys
            net = net.to(dt).train(training)
            ins = R.fixture_inputs(seed, tag, dt)
            memory = R.fixture_memory(seed, tag, dt)
            for t in ins + ([memory] if memory is not None else []):
                t.requires_grad_(True)
            got, hooks = {}, []
            at = {"f": 0}
            for i, blk in enumerate(net[0]):
                for name, mod in (("act1", blk.act1), ("act2", blk.act2), ("gate", blk.se.gate)):
                    hooks.append(mod.register_forward_hook(
                        lambda m, a, o, i=i, name=name: got.__setitem__("f%d_b%d_%s" % (at["f"], i, name), o.detach().clone().flatten(1) if name == "gate" else o.detach().clone())))
            memories = [memory] if memory is not None else None
            outs = []
            for f, x in enumerate(ins):
                at["f"] = f
                out, memories, idx = stage_fwd(net, x, R.MEMORY_PERCENT, memories, 0)
                assert idx == c["blocks"] and len(memories) == c["blocks"]
                for m in memories:
                    assert m.shape[1] == int(c["C"] * R.MEMORY_PERCENT)
                outs.append(out)
                got["f%d_out" % f] = out.detach()
            if c["blocks"] == 1 and c["frames"] == 1:            # the function itself, without the walk
                import copy
                twin = copy.deepcopy(net[0][0])                  # (its running statistics have moved once already in train mode:
                with torch.no_grad():                            #  batch statistics are what a train-mode output is made of)
                    direct, m1 = block_fwd(twin, ins[0], memory, R.MEMORY_PERCENT)
                assert torch.equal(direct, outs[0].detach()) and torch.equal(m1, ins[0][:, :m1.shape[1]])
            for h in hooks:
                h.remove()
            torch.autograd.backward(outs, R.fixture_cotangents(seed, tag, dt))
            for f, x in enumerate(ins):
                got["grad_in_f%d" % f] = x.grad.detach()
            if memory is not None:
                got["grad_memory"] = memory.grad.detach()
            for k, p in net.named_parameters():
                got["grad_" + k] = p.grad.detach()
            return got, keys, shapes

        arrs = dict(seed=seed)
        note = []
        for mode in R.MODES:
            training = mode == "train"
            r32, keys, shapes = run(torch.float32, training)
            r64, _, _ = run(torch.float64, training)
            assert keys == [k for k, _ in R.key_shapes(tag)] and shapes == [s for _, s in R.key_shapes(tag)]
            own = R.run(seed, tag, torch.float64, training)            # the restatement stands where the reference stands
            assert set(own) == set(r64), set(own) ^ set(r64)
            for k in r64:
                assert float((own[k] - r64[k]).abs().max()) <= 1e-10 * max(1.0, float(r64[k].abs().max())), (tag, mode, k)
            devs, rels = [], []
            for k in r32:
                if k.startswith("grad_"):
                    name = "grad_%s_%s" % (mode, k[5:])
                    arrs["rel_" + name] = float((r32[k].double() - r64[k]).norm() / r64[k].norm())
                    rels.append(arrs["rel_" + name])
                else:
                    name = "%s_%s" % (mode, k)
                    arrs["dev_" + name] = float((r32[k].double() - r64[k]).abs().max())
                    arrs["max_" + name] = float(r64[k].abs().max())
                    devs.append(arrs["dev_" + name])
                if R.stored(name):
                    arrs[name] = R.sample(r32[k], seed)
            note.append("%s: dev %.3g .. %.3g, rel_grad %.3g .. %.3g" % (mode, min(devs), max(devs), min(rels), max(rels)))
        arrs["keys"] = np.array(keys)
        arrs["key_shapes"] = np.array([list(s) + [-1] * (4 - len(s)) for s in shapes], dtype=np.int64)
        size = save_fixed("mbconv_" + tag, **arrs)
        total += size
        lines.append("mbconv_%s  B=%d C=%d Cmid=%d Cr=%d plane %dx%d, %d block(s), %d frame(s), first-frame memory %s  seed %d; %s; %.0f KB"
                     % (tag, c["B"], c["C"], c["Cmid"], c["Cr"], c["plane"][0], c["plane"][1], c["blocks"], c["frames"], c["memory"], seed,
                        "; ".join(note), size / 1024))
    lines.append("total %.0f KB" % (total / 1024))
    assert total < 1000 * 1000, total
    with open(os.path.join(OUT, "PROVENANCE_mbconv.txt"), "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


def reference_encoder(mb_class):
    """The reference's OWN `_block_forward`, `_inverted_residual_forward`, `TEMPORALSTEREO._forward` and `TEMPORALSTEREO.forward`
    (architecture/modeling/backbone/TemporalStereo.py:101-218), compiled from its file's syntax tree -- the module imports timm at the
    top, which this image does not have.  `InvertedResidual` is bound to `mb_class`, `drop_path` to a function that raises.
    -> (_block_forward, _forward(self, x, memories), forward(self, l_img, r_img, prev_info))"""
    import ast
    import typing
    import torch.nn.functional as F
    path = os.path.join(ref_import.REFERENCE_ROOT, "architecture", "modeling", "backbone", "TemporalStereo.py")
    tree = ast.parse(open(path).read(), filename=path)
    names = ("_block_forward", "_inverted_residual_forward")
    funcs = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name in names]
    cls = next(n for n in tree.body if isinstance(n, ast.ClassDef) and n.name == "TEMPORALSTEREO")
    funcs += [n for n in cls.body if isinstance(n, ast.FunctionDef) and n.name in ("_forward", "forward")]
    assert sorted(f.name for f in funcs) == sorted(names + ("_forward", "forward"))

    def drop_path(*a, **k):
        raise AssertionError("drop_path must not be reached: the stand-ins' drop_path_rate is 0")
    ns = {"torch": torch, "F": F, "InvertedResidual": mb_class, "drop_path": drop_path, "Union": typing.Union, "List": typing.List,
          "Tuple": typing.Tuple}
    exec(compile(ast.fix_missing_locations(ast.Module(body=funcs, type_ignores=[])), path, "exec"), ns)
    return ns["_block_forward"], ns["_forward"], ns["forward"]


def encoder_cases(M):
    """tests/golden/encoder_*.npz: tests/encoder_ref.py's stand-in blocks called as the reference calls them -- as modules, through its
    own `_block_forward`, and (case d) through its own backbone `forward` -- on the CPU, in fp32 and fp64, train mode and eval mode;
    dev_* = how far the fp32 run lies from the fp64 run."""
    import types
    import encoder_ref as R
    from architecture.modeling.layers import Conv2d
    stage_fwd, ref__forward, ref_forward = reference_encoder(R.StandInMB)
    lines = ["encoder_*.npz: tools/gen_golden.py --only-encoder, numpy %s, torch %s CPU -- tests/encoder_ref.py's stand-ins for timm 0.4.12's" % (np.__version__, torch.__version__),
             "ConvBnAct, EdgeResidual and InvertedResidual (timm, where the reference's blocks come from, is not part of its checkout) run by the",
             "reference's own code: _block_forward, _inverted_residual_forward, TEMPORALSTEREO._forward and TEMPORALSTEREO.forward",
             "(architecture/modeling/backbone/TemporalStereo.py:101-218, compiled from the file's syntax tree with the name InvertedResidual bound to",
             "encoder_ref.StandInMB and drop_path to a function that raises), the decoder's submodules built by the reference's own Conv2d;",
             "on seeded inputs in float32 and in float64, in train mode and in eval mode, with the backward of seeded cotangents.",
             "a, b: one fused block called as a module.  c: a stage of two fused blocks through _block_forward with memory_percent 1/4 (asserted:",
             "out_memories empty, memory_idx unchanged).  d: a miniature backbone (encoder_ref.MINI: stem 3 -> 8, a ConvBnAct with skip, two",
             "fused stages of a stride-2 and a residual block, two MBConv stages of a non-residual stride-2 and a residual block, the",
             "decoder) through forward(l_img, r_img, prev_info) on two frames of 2 x 3 x 64 x 96, the second reading the first's memories.",
             "Inputs, all kept as their seed (encoder_ref fixture_state / fixture_inputs / fixture_cotangents draw them again): convolution weights",
             "N(0,1) * 2 / sqrt(fan-in) (case d, some twenty layers deep: 1 / sqrt(fan-in)), convolution biases N(0, 0.1), BatchNorm weight U(0.5, 1.5) and bias N(0, 0.1), running mean N(0, 0.1),",
             "running variance U(0.5, 1.5), inputs N(0,1), cotangents k / 8 with k an integer in [-8, 8].",
             "Stored: seed, keys and key_shapes (the state-dict keys in order, shapes padded with -1), and per mode m in (train, eval) the",
             "deviations of EVERY output, stage and gradient over the WHOLE arrays: dev_<m>_<key> = max |fp32 run - fp64 run|, max_<m>_<key> =",
             "max |.| of the fp64 run, rel_grad_<m>_<input|parameter key> = relative L2 of the fp32 run's gradient against the fp64 run's.",
             "Arrays (fp32 run; one of more than %d elements at %d seeded flat positions, encoder_ref.sample): those encoder_ref.stored names." % (R.SAMPLE, R.SAMPLE),
             "The tests compare everything against the fp64 restatement, which the generator asserts equal to the reference's fp64 run to 1e-10."]
    total = 0
    for tag in R.TAGS:
        c = R.CASES[tag]
        seed = synth.SEED0 + 17000 + 1000 * ord(tag)

        def run(dt, training):
            net = R.stand_in(tag, Conv2d)
            keys = list(net.state_dict().keys())
            shapes = [tuple(v.shape) for v in net.state_dict().values()]
            res = net.load_state_dict(R.fixture_state(seed, tag), strict=True)
            assert not res.missing_keys and not res.unexpected_keys
            net = net.to(dt).train(training)
            ins = R.fixture_inputs(seed, tag, dt)
            for t in ins:
                t.requires_grad_(True)
            got, hooks, at = {}, [], {"f": 0}

            def keep(name, pick=lambda o: o):
                return lambda m, a, o=None: got.__setitem__("f%d_%s" % (at["f"], name), pick(a[0] if o is None else o).detach().clone())
            outs = []
            if c["kind"] == "backbone":
                net._forward = types.MethodType(ref__forward, net)
                o4 = R.MINI["out_channels"][4]
                hooks += [net.act1.register_forward_hook(keep("stem")), net.block0.register_forward_hook(keep("block0")),
                          net.block1[0][-1].register_forward_hook(keep("block1")), net.block2[0][-1].register_forward_hook(keep("block2")),
                          net.deconv32_16.register_forward_pre_hook(keep("block3", lambda t: t[:, o4:])),
                          net.conv32.register_forward_pre_hook(keep("block4"))]
                info = {}
                for f in range(c["frames"]):
                    at["f"] = f
                    before = list(info.get("memories", []))
                    l_fms, r_fms, info = ref_forward(net, ins[2 * f], ins[2 * f + 1], info)
                    assert len(info["memories"]) == 2 and (f == 0) == (before == [])
                    assert [m.shape[1] for m in info["memories"]] == [6, 8]
                    for k, l, r in zip(R.OUTS, l_fms, r_fms):
                        whole = torch.cat([l, r], 0)
                        outs.append(whole)
                        got["f%d_%s" % (f, k)] = whole.detach()
            else:
                for i, blk in enumerate(net[0]):
                    hooks += [blk.act1.register_forward_hook(keep("b%d_mid" % i)), blk.register_forward_hook(keep("b%d_out" % i))]
                if c["kind"] == "stage":
                    out, memories, idx = stage_fwd(net, ins[0], R.MEMORY_PERCENT, None, 0)
                    assert memories == [] and idx == 0           # no member is an InvertedResidual: nothing takes or leaves a memory
                else:
                    out = net[0][0](ins[0])
                outs.append(out)
                got["f0_out"] = out.detach()
            for h in hooks:
                h.remove()
            torch.autograd.backward(outs, R.fixture_cotangents(seed, tag, dt))
            for name, x in zip(R.input_names(tag), ins):
                got["grad_" + name] = x.grad.detach()
            for k, p in net.named_parameters():
                got["grad_" + k] = p.grad.detach()
            return got, keys, shapes

        arrs = dict(seed=seed)
        note = []
        for mode in R.MODES:
            training = mode == "train"
            r32, keys, shapes = run(torch.float32, training)
            r64, _, _ = run(torch.float64, training)
            assert keys == [k for k, _ in R.key_shapes(tag)] and shapes == [s for _, s in R.key_shapes(tag)]
            own = R.run(seed, tag, torch.float64, training)            # the restatement stands where the reference stands
            assert set(own) == set(r64), set(own) ^ set(r64)
            for k in r64:
                assert float((own[k] - r64[k]).abs().max()) <= 1e-10 * max(1.0, float(r64[k].abs().max())), (tag, mode, k)
            devs, rels = [], []
            for k in r32:
                if k.startswith("grad_"):
                    name = "grad_%s_%s" % (mode, k[5:])
                    arrs["rel_" + name] = float((r32[k].double() - r64[k]).norm() / r64[k].norm())
                    rels.append(arrs["rel_" + name])
                else:
                    name = "%s_%s" % (mode, k)
                    arrs["dev_" + name] = float((r32[k].double() - r64[k]).abs().max())
                    arrs["max_" + name] = float(r64[k].abs().max())
                    devs.append(arrs["dev_" + name])
                if R.stored(name):
                    arrs[name] = R.sample(r32[k], seed)
            note.append("%s: dev %.3g .. %.3g, rel_grad %.3g .. %.3g" % (mode, min(devs), max(devs), min(rels), max(rels)))
        arrs["keys"] = np.array(keys)
        arrs["key_shapes"] = np.array([list(s) + [-1] * (4 - len(s)) for s in shapes], dtype=np.int64)
        size = save_fixed("encoder_" + tag, **arrs)
        total += size
        lines.append("encoder_%s  %s, B=%d, plane %dx%d, %d frame(s)  seed %d; %s; %.0f KB"
                     % (tag, c["kind"] + (" " + repr(c["members"]) if "members" in c else ""), c["B"], c["plane"][0], c["plane"][1], c["frames"],
                        seed, "; ".join(note), size / 1024))
    lines.append("total %.0f KB" % (total / 1024))
    assert total < 1000 * 1000, total
    with open(os.path.join(OUT, "PROVENANCE_encoder.txt"), "w") as fh:
        fh.write("\n".join(lines) + "\n")
    print("\n".join(lines))


def save_fixed(name, **arrs):
    """`save` with the archive's time stamps pinned, so that a fixture regenerates byte for byte."""
    import zipfile
    path = os.path.join(OUT, name + ".npz")
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_DEFLATED) as z:
        for k, v in arrs.items():
            info = zipfile.ZipInfo(k + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            with z.open(info, "w", force_zip64=True) as fh:
                np.lib.format.write_array(fh, np.asanyarray(v.detach().cpu().numpy() if torch.is_tensor(v) else v), allow_pickle=False)
    print("wrote %-38s %8.1f KB" % (name + ".npz", os.path.getsize(path) / 1024))
    return os.path.getsize(path)


def _reference_flow_frame():
    """The reference's flow_calc_error, do_flow_evaluation, flow_colormap.py and load_png.  The packages' __init__s import more than
    this image has, so the files are loaded by path; do_flow_evaluation is taken from flow_eval.py's syntax tree and compiled as it
    is (its relative import replaced by the loaded flow_calc_error); load_flow.py's `png` (pypng, absent here) is bound to a reader
    that hands load_png the rows of an array in pypng's asDirect() form -- decoding the file is not what is restated."""
    import ast
    import importlib.util
    import types
    import warnings
    os.environ.setdefault("MPLBACKEND", "Agg")

    def by_path(name, *parts):
        spec = importlib.util.spec_from_file_location(name, os.path.join(ref_import.REFERENCE_ROOT, *parts))
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        return mod
    pe = by_path("_ref_flow_pixel_error", "architecture", "data", "evaluation", "flow_pixel_error.py")
    path = os.path.join(ref_import.REFERENCE_ROOT, "architecture", "data", "evaluation", "flow_eval.py")
    tree = ast.parse(open(path).read(), filename=path)
    fns = [n for n in tree.body if isinstance(n, ast.FunctionDef) and n.name == "do_flow_evaluation"]
    ns = {"torch": torch, "warnings": warnings, "flow_calc_error": pe.flow_calc_error}
    exec(compile(ast.Module(body=fns, type_ignores=[]), path, "exec"), ns)
    cm = by_path("_ref_flow_colormap", "architecture", "utils", "visualization", "flow_colormap.py")
    held = {}

    class Reader:
        def __init__(self, filename):
            self.a = held[filename]

        def asDirect(self):
            h, w, _ = self.a.shape
            return w, h, (row.reshape(-1).tolist() for row in self.a), {'size': (w, h)}
    before = sys.modules.get("png")
    sys.modules["png"] = types.SimpleNamespace(Reader=Reader)
    try:
        lf = by_path("_ref_load_flow", "architecture", "data", "utils", "load_flow.py")
    finally:
        if before is None:
            del sys.modules["png"]
        else:
            sys.modules["png"] = before

    def load_png(raw_hw3):
        held["mem"] = raw_hw3
        return lf.load_png("mem")
    return pe.flow_calc_error, ns["do_flow_evaluation"], cm, load_png


FLOW_FRAME_TIE_CAP = 0.005


def flow_frame_cases(M):
    """tests/golden/flow_frame_*.npz: the reference's own flow_calc_error / do_flow_evaluation, flow_max_rad / flow_to_color /
    flow_err_to_color / make_color_wheel and load_png on seeded flow maps on the CPU.

    Inputs are stored as int16 in 1/64 px (KITTI's grid) plus the planted non-finite / huge / negative-zero values at their flat
    indices.  Discrete outputs (percentages, class maps) are the reference's own; tests/flow_frame_ref.py must reproduce them
    exactly, asserted here.  Continuous outputs (colours) are the reference's float32 images; dev_own / dev_given = the largest
    distance of tests/flow_frame_ref.py from them over the cases with a maximum taken from the data / a given or shared maximum.
    tie_* = pixels whose normalised radius lies within 4 x (the largest float32-vs-float64 deviation of that radius) of 1, the one
    discontinuity rounding can move under a given or shared maximum; at most 0.5 % of a case's pixels, asserted here.  With the
    map's own maximum the reference, which normalises in float64 by the float32 maximum, can find the pixel that set the maximum
    a rounding outside the disc and darken it; bright_* marks those pixels (at most two per image, and maximal: asserted), where
    the device is compared with tests/flow_frame_ref.py instead.
    The rescaled case scores the torch composition F.interpolate(est, size, bilinear, align_corners=True) * (Wg / w, Hg / h) on the
    CPU; tau = 16 units in the last place of the largest rescaled component (three lerps of at most three roundings each, the scale,
    the difference, the radius: under ten half-units per component) and near_thr / tie_class = the pixels within tau of a
    threshold / a class bound."""
    import warnings
    import torch.nn.functional as F
    import flow_frame_ref as R
    warnings.filterwarnings("ignore")
    calc, do_eval, cm, load_png = _reference_flow_frame()
    ALL = ("color_est", "color_gt", "color_est_given", "color_shared", "class", "class_val")
    cases = {"dense": dict(hw=(48, 80), B=1, outs=("color_est", "color_gt", "class", "class_val"), planted=True),
             "sparse": dict(hw=(40, 64), B=2, zero_block=True, outs=("class",)),
             "none_valid": dict(hw=(16, 24), B=1, all_zero=True, outs=("color_gt", "class")),
             "nonfinite": dict(hw=(40, 60), B=2, nonfinite=True, outs=("color_est", "color_gt", "class")),
             "ragged": dict(hw=(50, 78), B=2, outs=("color_est", "class")),
             "tiny1": dict(hw=(1, 1), B=1, outs=ALL, given=0.6),
             "tiny35": dict(hw=(3, 5), B=2, outs=ALL, given=0.6),
             "batch3": dict(hw=(30, 50), B=3, unknown_image=1, outs=("color_est", "color_est_given"), given=0.2),
             "given_max": dict(hw=(49, 83), B=1, outs=("color_est_given",), given=25.0, absolute=True),
             "shared": dict(hw=(44, 72), B=1, outs=("color_shared",)),
             "rescaled": dict(hw=(56, 88), low=(14, 22), B=1, outs=("class",))}
    assert tuple(cases) == R.CASES
    VARIANTS = ((0.0, 400, False), (-1.0, 400, True), (2.0, 30.0, False), (-1.0, 400, False))          # (lb, ub, sparse) of metrics[0..3]
    runs = {}
    for ci, (name, c) in enumerate(cases.items()):
        seed = synth.SEED0 + 9500 + ci
        B = c["B"]
        H, W = c["hw"]
        h, w = c.get("low", c["hw"])
        yy, xx = np.meshgrid(np.arange(H, dtype=np.float64), np.arange(W, dtype=np.float64), indexing="ij")
        amp = synth.uniform(seed, "amp", (B, 1, 1), 12.0, 40.0).astype(np.float64)
        gu = amp * (0.2 + 0.7 * np.sin(2 * np.pi * xx / max(W, 2) + amp) + 0.3 * np.cos(2 * np.pi * yy / max(H, 2)))
        gv = 0.6 * amp * (0.1 + 0.8 * np.cos(2 * np.pi * xx / max(W, 2) - 0.5 * amp) - 0.4 * np.sin(2 * np.pi * yy / max(H, 2) + amp))
        gt = np.stack([gu, gv], axis=1) + synth.uniform(seed, "gtn", (B, 2, H, W), -0.5, 0.5)
        # errors spread over every class: many small ones, a few beyond 48 px
        uu = synth.uniform(seed, "eu", (B, 1, H, W))
        mag = np.where(uu < 0.3, 0.15, np.where(uu < 0.55, 0.6, np.where(uu < 0.75, 2.5, np.where(uu < 0.9, 9.0, np.where(uu < 0.97, 30.0, 70.0)))))
        full = gt + synth.normal(seed, "en", (B, 2, H, W), 1.0).astype(np.float64) * mag
        if c.get("all_zero"):
            gt = np.zeros_like(gt)
        if c.get("zero_block"):
            gt[:, :, H // 4:H // 2, W // 8:W // 2] = 0.0
        gq = np.round(gt * 64).astype(np.int16)
        if (h, w) != (H, W):
            iy, ix = (np.arange(h) * H) // h, (np.arange(w) * W) // w
            eq = np.round(full[:, :, iy][..., ix] * np.array([w / W, h / H]).reshape(1, 2, 1, 1) * 64).astype(np.int16)
        else:
            eq = np.round(full * 64).astype(np.int16)
        es, gs = [], []                                     # planted (flat index, value)
        at = lambda b, ch, y, x, hh=H, ww=W: ((b * 2 + ch) * hh + y) * ww + x
        if c.get("planted"):
            # E exactly on the class end points 0.1875, 3.0 and 48.0; err exactly 1, 2, 3 and 5; the pair (3, +0.0), (3, -0.0)
            for k, (du, dv) in enumerate(((12, 0), (192, 0), (0, 3072), (64, 0), (0, 128), (192, 256))):
                eq[0, 0, 5, 10 + k] = gq[0, 0, 5, 10 + k] - du
                eq[0, 1, 5, 10 + k] = gq[0, 1, 5, 10 + k] - dv
            eq[0, :, 7, 20] = (192, 0)
            eq[0, :, 7, 21] = (192, 0)
            es.append((at(0, 1, 7, 21), np.float32(-0.0)))
        if c.get("nonfinite"):
            es += [(at(0, 0, 10, 20), np.float32(np.nan)), (at(0, 1, 11, 21), np.float32(np.inf)), (at(1, 0, 12, 22), np.float32(-np.inf)),
                   (at(1, 1, 13, 23), np.float32(2e7)), (at(1, 0, 14, 24), np.float32(-3e7))]
            gs += [(at(0, 0, 20, 30), np.float32(np.nan)), (at(0, 1, 21, 31), np.float32(np.nan)), (at(1, 1, 22, 32), np.float32(np.inf)),
                   (at(1, 0, 23, 33), np.float32(2e7))]
        if "unknown_image" in c:
            b = c["unknown_image"]
            es += [(at(b, 0, y, x), np.float32(3e7)) for y in range(H) for x in range(W)]
        unpack = lambda lst: (np.array([i for i, _ in lst], dtype=np.int64), np.array([v for _, v in lst], dtype=np.float32))
        ei, ev_ = unpack(es)
        gi, gv_ = unpack(gs)
        est, gtf = R.dequant(eq, ei, ev_), R.dequant(gq, gi, gv_)
        gt_val = None
        if "class_val" in c["outs"]:
            r = synth.uniform(seed, "val", (B, H, W))
            gt_val = np.where(r < 0.3, 0, np.where(r < 0.4, 1, 2)).astype(np.uint8)           # in halves: 0, 0.5, 1
        runs[name] = dict(c=c, eq=eq, gq=gq, ei=ei, ev=ev_, gi=gi, gv=gv_, est=est, gt=gtf, gt_val=gt_val)

    # ---- the reference's outputs
    dev = {"own": 0.0, "given": 0.0}
    dev_rad = 0.0
    for name, r in runs.items():
        c, est, gt = r["c"], r["est"], r["gt"]
        B = c["B"]
        H, W = c["hw"]
        o = r["out"] = {}
        if est.shape[-2:] != (H, W):
            scale = torch.tensor([W / est.shape[-1], H / est.shape[-2]], dtype=torch.float32).view(1, 2, 1, 1)
            full = (F.interpolate(T(est), size=(H, W), mode='bilinear', align_corners=True) * scale).numpy()
            o["est_full"] = full
            o["tau"] = np.float64(16 * np.spacing(np.float32(np.abs(full).max())))
        else:
            full = est
        # metrics
        met, nv = [], []
        for lb, ub, sparse in VARIANTS:
            d = calc(T(full.copy()), T(gt.copy()), lb=lb, ub=ub, sparse=sparse)
            met.append([float(d[k]) for k in R.KEYS])
            mine, n = R.calc_error(full, gt, lb, ub, sparse)
            nv.append(n)
            got = np.array(met[-1], dtype=np.float32)
            assert np.array_equal(got[:4], mine[:4]), (name, lb, ub, sparse, got, mine)
            assert np.array_equal(np.isnan(got), np.isnan(mine)), (name, got, mine)
            if np.isfinite(got[4]):
                assert abs(float(got[4]) - float(mine[4])) <= 2e-6 * abs(float(got[4])), (name, got, mine)
        o["metrics"] = np.array(met, dtype=np.float32)
        o["n_valid"] = np.array(nv, dtype=np.int64)
        d = do_eval(T(full.copy()), T(gt.copy()), lb=2.0, ub=30.0, sparse=False)       # its lb / ub are not passed on
        o["do_flow_evaluation"] = np.array([float(d[k]) for k in R.KEYS], dtype=np.float32)
        assert np.array_equal(o["do_flow_evaluation"], o["metrics"][0], equal_nan=True), name
        if "tau" in o:
            near = []
            for lb, ub, sparse in VARIANTS:
                e = R.flow_error(full, gt)[R.valid_mask(gt, lb, ub, sparse)].astype(np.float64)
                near.append([int((np.abs(e - t) <= o["tau"]).sum()) for t in (1, 2, 3, 5)])
            o["near_thr"] = np.array(near, dtype=np.int64)
        # colours
        fh, gh = R.hwc(full), R.hwc(gt)
        own_e = np.array([cm.flow_max_rad(fh[b].copy()) for b in range(B)], dtype=np.float32)
        own_g = np.array([cm.flow_max_rad(gh[b].copy()) for b in range(B)], dtype=np.float32)
        o["max_rad_est"], o["max_rad_gt"] = own_e, own_g
        assert np.array_equal(own_e, np.array([R.max_rad(fh[b]) for b in range(B)])), name
        assert np.array_equal(own_g, np.array([R.max_rad(gh[b]) for b in range(B)])), name

        def color(key, maps, maxima, group):
            """the reference's image of each map with its maximum (None: its own); the restatement's distance from it"""
            nonlocal dev_rad
            img = np.stack([cm.flow_to_color(maps[b].copy(), max_rad=None if maxima is None else float(maxima[b])) for b in range(B)])
            assert img.dtype == np.float32 and img.shape == (B, H, W, 3)
            mine = np.stack([R.flow_to_color(maps[b], None if maxima is None else maxima[b], data_max=maxima is None or group == "shared")
                             for b in range(B)])
            m = own_e if maps is fh else own_g
            m = m if maxima is None else np.asarray(maxima, dtype=np.float32)
            rad32 = np.stack([R.norm_radius(maps[b], m[b]) for b in range(B)])
            kn = np.stack([R.known(maps[b]) for b in range(B)]).astype(np.float64)
            den = (m.astype(np.float32) + np.float32(2.0 ** -52)).astype(np.float64).reshape(B, 1, 1)
            rad64 = np.sqrt((kn[..., 0] / den) ** 2 + (kn[..., 1] / den) ** 2)
            ok = np.isfinite(rad64)
            if ok.any():
                dev_rad = max(dev_rad, float(np.abs(rad32.astype(np.float64) - rad64)[ok].max()))
            if maxima is None:
                # The reference normalises in float64 by the float32 maximum, so the pixel(s) that set the maximum can come out
                # at a radius a rounding above 1 and are then darkened (x 0.75).  The device never does that: those pixels are
                # marked, left out of the distance, and must be the maximal ones.
                bright = rad64 > 1
                r0 = np.stack([R.radius(R.known(maps[b])[..., 0], R.known(maps[b])[..., 1]) for b in range(B)])
                assert (r0[bright] == np.broadcast_to(m.reshape(B, 1, 1), r0.shape)[bright]).all() and bright.sum() <= 2 * B, (name, key)
                o["bright_" + key[6:]] = bright
                r["skip_" + key] = bright
            o[key] = img
            r["rad64_" + key] = rad64
            r["mine_" + key] = mine
            r["group_" + key] = "own" if maxima is None else "given"
            return img

        if "color_est" in c["outs"]:
            color("color_est", fh, None, "own")
        if "color_gt" in c["outs"]:
            color("color_gt", gh, None, "own")
        if "color_est_given" in c["outs"]:
            given = np.full(B, c["given"], dtype=np.float32) if c.get("absolute") else (own_e * np.float32(c["given"])).astype(np.float32)
            o["given_max"] = given
            color("color_est_given", fh, given, "given")
            if B * H * W >= 400:
                outside = float((np.stack([R.norm_radius(fh[b], given[b]) for b in range(B)]) > 1).mean())
                assert 0.03 <= outside <= 0.8, (name, outside)
                o["outside_share"] = np.float64(outside)
        if "color_shared" in c["outs"]:
            shared = np.maximum(own_e, own_g)
            o["shared_max"] = shared
            color("color_shared_est", fh, shared, "shared")
            color("color_shared_gt", gh, shared, "shared")
        # classes
        idx_of = lambda img: np.where(img.reshape(-1, 3).sum(axis=1) == 0, -1,
                                      np.abs(img.reshape(-1, 1, 3) - (R.CLASS_RGB / np.float32(255))[None]).sum(axis=2).argmin(axis=1)).astype(np.int8)
        if "class" in c["outs"]:
            img = np.stack([cm.flow_err_to_color(fh[b].copy(), gh[b].copy()) for b in range(B)])
            assert img.dtype == np.float32
            cls = idx_of(img).reshape(B, H, W)
            assert np.array_equal(R.class_colors(cls), img), name
            assert np.array_equal(cls, R.err_class(full, gt)), name
            o["class_idx"] = cls
            if "tau" in o:
                E = R.flow_error(full, gt).astype(np.float64)
                tie = np.zeros(E.shape, dtype=bool)
                for lo in R.CLASS_LO[1:]:
                    tie |= np.abs(E - float(lo)) <= o["tau"]
                assert tie.mean() <= FLOW_FRAME_TIE_CAP, (name, tie.mean())
                o["tie_class"] = tie
        if "class_val" in c["outs"]:
            val = r["gt_val"].astype(np.float32) / np.float32(2)
            img = np.stack([cm.flow_err_to_color(fh[b].copy(), gh[b].copy(), val[b].copy()) for b in range(B)])
            cls = idx_of(img).reshape(B, H, W)
            assert np.array_equal(R.class_colors(cls), img), name
            assert np.array_equal(cls, R.err_class(full, gt, val)), name
            o["class_val_idx"] = cls
        for key in [k for k in r if k.startswith("mine_")]:
            k = key[5:]
            d = np.abs(r[key].astype(np.float64) - o[k].astype(np.float64))
            if r["group_" + k] == "given":                  # the branch may differ on a near-tie pixel: measured away from them below
                r["diff_" + k] = d
            else:
                away = d[~r["skip_" + k]]
                if away.size:
                    dev["own"] = max(dev["own"], float(away.max()))
    tau_rad = 4 * dev_rad
    for name, r in runs.items():
        o = r["out"]
        for key in [k for k in r if k.startswith("diff_")]:
            k = key[5:]
            tie = np.abs(r["rad64_" + k] - 1.0) <= tau_rad
            assert tie.mean() <= FLOW_FRAME_TIE_CAP or tie.size < 400, (name, k, tie.mean())
            o["tie_" + k[6:]] = tie
            away = r[key][~tie]
            if away.size:
                dev["given"] = max(dev["given"], float(away.max()))
    wheel = cm.make_color_wheel()
    assert wheel.shape == (55, 3) and np.array_equal(wheel, R.make_color_wheel())
    lines = ["flow_frame_*.npz: tools/gen_golden.py --only-flow-frame, numpy %s, torch %s CPU -- the reference's own flow_calc_error /" % (np.__version__, torch.__version__),
             "do_flow_evaluation (architecture/data/evaluation), make_color_wheel / flow_max_rad / flow_to_color / flow_err_to_color",
             "(architecture/utils/visualization/flow_colormap.py) and the arithmetic of load_png (architecture/data/utils/load_flow.py) on seeded maps.",
             "Inputs: int16 in 1/64 px plus planted NaN / inf / > 1e7 / -0.0 values.  metrics[0..3] = (lb, ub, sparse) of %s;" % (VARIANTS,),
             "do_flow_evaluation was called with lb=2, ub=30 and equals metrics[0]: it does not pass its bounds on.",
             "Percentages, maximum radii, class maps and the decode are the reference's and tests/flow_frame_ref.py reproduces them exactly (asserted).",
             "Colours: dev_own = %.3g (maximum from the data), dev_given = %.3g (given or shared maximum, away from the near-tie pixels) = the" % (dev["own"], dev["given"]),
             "largest |tests/flow_frame_ref.py - reference| over those cases; a device result may lie 4 x that from the reference.",
             "Near ties: the float32 normalised radius deviates from its float64 value by at most %.3g; tie_* = |rad - 1| <= 4 x that = %.3g," % (dev_rad, tau_rad),
             "at most %.1f %% of a case's pixels (asserted).  bright_* = the pixels that set a map's own maximum and that the reference, normalising in" % (100 * FLOW_FRAME_TIE_CAP),
             "float64 by the float32 maximum, finds a rounding outside the disc and darkens; the device keeps them inside (left out of dev_own)."]
    total = 0
    for name, r in runs.items():
        c, o = r["c"], r["out"]
        arrs = dict(est_q64=r["eq"], gt_q64=r["gq"], est_special_idx=r["ei"], est_special_val=r["ev"], gt_special_idx=r["gi"],
                    gt_special_val=r["gv"], dev_own=np.float64(dev["own"]), dev_given=np.float64(dev["given"]), tau_rad=np.float64(tau_rad))
        if r["gt_val"] is not None:
            arrs["gt_val_half"] = r["gt_val"]
        if name == "dense":
            arrs["wheel"] = wheel
        arrs.update(o)
        size = save_fixed("flow_frame_" + name, **arrs)
        assert size <= 260 * 1024, (name, size)
        total += size
        ties = {k: int(v.sum()) for k, v in o.items() if k.startswith("tie_") or k.startswith("bright_")}
        lines.append("flow_frame_%-10s B=%d %dx%d%s  N = %s  outputs %s%s%s; %.0f KB"
                     % (name, c["B"], c["hw"][0], c["hw"][1], (" est %dx%d" % c["low"]) if "low" in c else "", o["n_valid"].tolist(),
                        ", ".join(c["outs"]), ("  near ties %s" % ties) if ties else "",
                        ("  tau %.3g near thresholds %s" % (o["tau"], o["near_thr"].tolist())) if "tau" in o else "", size / 1024))
    # KITTI 16-bit flow
    seed = synth.SEED0 + 9590
    B, H, W = 2, 20, 31
    raw = np.empty((B, H, W, 3), dtype=np.uint16)
    raw[..., :2] = np.clip(32768 + np.round(synth.normal(seed, "uv", (B, H, W, 2), 40.0) * 64), 0, 65535).astype(np.uint16)
    raw[..., 2] = (synth.uniform(seed, "ok", (B, H, W)) >= 0.3).astype(np.uint16)
    raw[0, 0, 0] = (0, 65535, 1)
    raw[0, 0, 1] = (65535, 0, 7)
    raw[1, 3, 4] = (12345, 54321, 0)
    ref = np.stack([load_png(raw[b]) for b in range(B)])
    assert ref.dtype == np.float32 and ref.shape == (B, H, W, 3)
    flow, valid = R.decode_kitti(raw)
    assert np.array_equal(flow, np.moveaxis(ref[..., :2], -1, 1)) and np.array_equal(valid[:, 0], ref[..., 2] != 0)
    size = save_fixed("flow_frame_kitti", raw=raw, flow=np.ascontiguousarray(np.moveaxis(ref[..., :2], -1, 1)), valid=(ref[..., 2] != 0)[:, None])
    total += size
    lines.append("flow_frame_kitti      B=%d %dx%d uint16 [B,H,W,3], %.0f %% invalid: load_png's flow and third channel; %.0f KB"
                 % (B, H, W, 100 * float((raw[..., 2] == 0).mean()), size / 1024))
    lines.append("total %.0f KB" % (total / 1024))
    with open(os.path.join(OUT, "PROVENANCE_flow_frame.txt"), "w") as fh_:
        fh_.write("\n".join(lines) + "\n")
    print("\n".join(lines))


def main():
    os.makedirs(OUT, exist_ok=True)
    torch.manual_seed(0)
    torch.set_num_threads(8)
    M = ref_import.import_reference()
    if "--only-siblings" in sys.argv:
        sibling_cases(M)
        return
    if "--only-temporal" in sys.argv:
        temporal_update_cases(M)
        return
    if "--only-losses" in sys.argv:
        loss_cases(M)
        return
    if "--only-eval" in sys.argv:
        eval_cases(M)
        return
    if "--only-render" in sys.argv:
        render_cases(M)
        return
    if "--only-prepare" in sys.argv:
        prepare_cases(M)
        return
    if "--only-warp" in sys.argv:
        warp_cases(M)
        return
    if "--only-raft" in sys.argv:
        raft_cases(M)
        return
    if "--only-flow" in sys.argv:
        flow_cases(M)
        return
    if "--only-spp3d" in sys.argv:
        spp3d_cases(M)
        return
    if "--only-convgru" in sys.argv:
        conv_gru_cases(M)
        return
    if "--only-decoder" in sys.argv:
        decoder_cases(M)
        return
    if "--only-mbconv" in sys.argv:
        mbconv_cases(M)
        return
    if "--only-encoder" in sys.argv:
        encoder_cases(M)
        return
    if "--only-flow-frame" in sys.argv:
        flow_frame_cases(M)
        return
    if "--only-augment" in sys.argv:
        augment_cases(M)
        return
    if "--only-backbone-memory" in sys.argv:
        backbone_memory_cases(M)
        return
    if "--only-planted" in sys.argv:
        planted_cases(M, [a for a in sys.argv[1:] if a.startswith("planted_")] or None)
        if not any(a.startswith("planted_") for a in sys.argv[1:]):
            planted_gradient_case(M)
        return
    if "--only-planted-grads-c1" in sys.argv:
        planted_gradient_case(M, full_size=True)
        return
    if "--only-planted-grads" in sys.argv:
        planted_gradient_case(M)
        return
    functional_cases(M)
    sibling_cases(M)
    temporal_update_cases(M)
    loss_cases(M)
    backbone_memory_cases(M)
    eval_cases(M)
    planted_cases(M)
    planted_gradient_case(M)
    aggregator_case("agg_tiny_single", TINY, synth.SEED0 + 100, 2, 96, 160, temporal=False, store_inputs=True)
    aggregator_case("agg_tiny_temporal", TINY, synth.SEED0 + 101, 2, 96, 160, temporal=True, store_inputs=True)
    aggregator_case("agg_tiny_train", TINY, synth.SEED0 + 102, 2, 96, 160, temporal=False, store_inputs=True,
                    training=True)
    c1 = dict(SCENEFLOW); c1['coarse'] = dict(SCENEFLOW['coarse'], num_sample=3)      # D=48 -> 48/16
    aggregator_case("agg_config1_256x512", c1, synth.SEED0 + 1, 1, 256, 512, temporal=False, store_inputs=False)
    with open(os.path.join(OUT, "PROVENANCE.txt"), "w") as fh:
        fh.write("Generated by tools/gen_golden.py from the reference at /root/reference (v1), torch %s CPU.\n"
                 "Inputs come from tests/synth.py seeds; weights from synth.state_values().\n" % torch.__version__)


if __name__ == "__main__":
    main()
