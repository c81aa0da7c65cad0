"""Training-frame augmentation (temporalstereo_amd/augment.py): the numpy restatement of tests/augment_ref.py against the PIL-made
fixtures (tests/golden/augment_*.npz, tools/gen_golden.py --only-augment), the host-side draws, the gamma table, the parameter
table's layout and the C ABI's entries -- no GPU needed."""
import os
import re

import numpy as np
import pytest

import augment_ref as R
import temporalstereo_amd as ts
from temporalstereo_amd import augment as ag

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CASES = ("augment_ops", "augment_orders", "augment_chain", "augment_occlusion", "augment_large", "augment_identity")
ENTRIES = ("ts_frames_augment_fwd", "ts_disp_u16_window_fwd")
MEAN, STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


def load(name):
    return dict(np.load(os.path.join(GOLDEN, name + ".npz")))


def fixture_rows(g, e, b):
    """(order, factors, gamma table or None) of eye e, image b of a fixture"""
    order = [int(o) for o in g["order"][e, b]]
    colour = name_has_colour(g)
    return order, [float(v) for v in g["factors"][e, b]], (ag.gamma_table(float(g["gamma"][e, b])) if colour else None)


def name_has_colour(g):
    return bool((g["order"] != R.NONE).any() or (g["gamma"] != 1.0).any() or not np.array_equal(g["stage_l"], g["left"]))


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_fixture(name):
    """every uint8 stage and every float outside the rectangles, bit for bit"""
    g = load(name)
    size = tuple(int(v) for v in g["size"])
    B = g["left"].shape[0]
    for b in range(B):
        crop = tuple(int(v) for v in g["crop"][b])
        for e, side in enumerate("lr"):
            src = g["left" if e == 0 else "right"][b]
            order, factors, table = fixture_rows(g, e, b)
            stage, color, aug = R.frame(src, order, factors, None, table, crop, size, MEAN, STD)
            assert np.array_equal(stage, g["stage_" + side][b]), "%s image %d eye %s: uint8 stage" % (name, b, side)
            assert np.array_equal(color.view(np.int32), g["color_" + side][b].view(np.int32)), "%s image %d eye %s: color" % (name, b, side)
            rects = [tuple(int(v) for v in q) for q in g["rects"][b][:int(g["nrect"][b])]] if e == 1 else []
            keep = ~R.rect_mask(rects, size)
            exp = g["aug_" + side][b]
            assert np.array_equal(aug.view(np.int32)[:, keep], exp.view(np.int32)[:, keep]), "%s image %d eye %s: color_aug" % (name, b, side)
            if rects:                                     # the reference did overwrite what the mask leaves out
                assert (aug[:, ~keep] != exp[:, ~keep]).mean() > 0.999


def test_fixtures_hold_the_cases_asked_for():
    g = load("augment_ops")
    px = g["left"][0].reshape(-1, 3).astype(int)
    assert (px.max(1) == px.min(1)).any()                                            # greys
    assert any((px == p).all(1).any() for p in ((255, 0, 0), (0, 255, 0), (0, 0, 255)))
    assert ((px[:, 0] == px[:, 1]) & (px[:, 1] != px[:, 2])).any() and ((px[:, 1] == px[:, 2]) & (px[:, 0] != px[:, 1])).any()
    assert (g["factors"][0, :, 3] < 0).any() and (g["factors"][0, :, 3] > 0).any()
    assert sorted(set(g["gamma"][0])) == [0.8, 1.0, 1.2]
    o = load("augment_orders")["order"]
    assert len({tuple(r) for r in o.reshape(-1, 4)}) == 24
    assert sorted(load("augment_occlusion")["nrect"]) == [2, 3, 4]
    assert sum(os.path.getsize(os.path.join(GOLDEN, n + ".npz")) for n in CASES) < 1024 * 1024


def test_gamma_table():
    assert np.array_equal(ag.gamma_table(1.0), np.arange(256, dtype=np.uint8))
    t = ag.gamma_table(0.8)
    assert t.dtype == np.uint8 and t.shape == (256,) and t[0] == 0 and t[255] == 255 and (np.diff(t.astype(int)) >= 0).all()
    assert t[128] == min(255, int((255 + 1 - 1e-3) * (128 / 255.0) ** 0.8))
    assert ag.gamma_table(1.0, gain=2.0)[200] == 255
    with pytest.raises(ValueError):
        ag.gamma_table(-1.0)


def test_draws_respect_ranges_and_are_reproducible():
    a = ag.draw_augmentation(64, (540, 960), (512, 960), seed=7, p_color=1.0, p_occlusion=1.0)
    assert a.eyes == 2 and a.B == 64 and a.table is None
    lo, hi = np.array([0.4, 0.5, 0.5, -0.1]), np.array([2.0, 1.5, 1.5, 0.1])
    assert (a.factors >= lo).all() and (a.factors <= hi).all()
    assert (a.gamma >= 0.8).all() and (a.gamma <= 1.2).all() and a.gamma_on.all()
    assert all(sorted(int(o) for o in a.order[e, b]) == [0, 1, 2, 3] for e in range(2) for b in range(64))
    assert len({tuple(r) for r in a.order.reshape(-1, 4)}) > 12                      # the orders do vary
    assert (a.crop[:, 0] >= 0).all() and (a.crop[:, 0] <= 28).all() and (a.crop[:, 1] == 0).all() and len(set(a.crop[:, 0])) > 5
    for b in range(64):
        assert a.rects[0][b] == [] and 2 <= len(a.rects[1][b]) <= 4
        for sh, sw, oh, ow in a.rects[1][b]:
            assert 50 <= ow < 250 and 50 <= oh < 180 and 0 <= sh and sh + oh <= 512 and 0 <= sw and sw + ow <= 960
    assert {len(r) for r in a.rects[1]} == {2, 3, 4}
    assert not np.array_equal(a.factors[0], a.factors[1])                            # same_lr=False: independent eyes
    a.check((540, 960), (512, 960))
    b = ag.draw_augmentation(64, (540, 960), (512, 960), seed=7, p_color=1.0, p_occlusion=1.0)
    assert np.array_equal(a.table_host(), b.table_host())
    c = ag.draw_augmentation(64, (540, 960), (512, 960), seed=8, p_color=1.0, p_occlusion=1.0)
    assert not np.array_equal(a.table_host(), c.table_host())
    s = ag.draw_augmentation(5, (540, 960), (512, 960), seed=7, p_color=1.0, p_occlusion=1.0)      # prefix-stable in B
    assert np.array_equal(s.table_host(), a.table_host()[:, :5])
    one = ag.draw_augmentation(5, (540, 960), (512, 960), seed=7, p_color=1.0, p_occlusion=1.0, eyes=1)
    assert np.array_equal(one.table_host()[0], a.table_host()[0, :5])
    same = ag.draw_augmentation(8, (540, 960), (512, 960), seed=7, p_color=1.0, same_lr=True)
    assert np.array_equal(same.factors[0], same.factors[1]) and np.array_equal(same.order[0], same.order[1])
    d = ag.draw_augmentation(400, (100, 120), (64, 64), seed=3)                      # the default probabilities
    assert 0.35 < d.gamma_on[0].mean() < 0.65 and 0.35 < np.mean([len(r) > 0 for r in d.rects[1]]) < 0.65
    assert all(q[2] <= 64 and q[3] <= 64 for r in d.rects[1] for q in r)
    gen = ag.draw_augmentation(3, (64, 64), (32, 32), generator=np.random.default_rng(5))
    gen2 = ag.draw_augmentation(3, (64, 64), (32, 32), generator=np.random.default_rng(5))
    assert np.array_equal(gen.table_host(), gen2.table_host())
    with pytest.raises(ValueError):
        ag.draw_augmentation(2, (64, 64), (65, 32), seed=0)
    with pytest.raises(ValueError):
        ag.draw_augmentation(2, (64, 64), (32, 32))
    with pytest.raises(ValueError):
        ag.draw_augmentation(2, (64, 64), (32, 32), seed=0, patches=(2, 5))


def test_table_layout():
    rows = [[dict(order=('hue', 'brightness'), brightness=1.25, hue=-0.1, gamma=0.9, seed=0x1122334455667788)],
            [dict(order=(ag.CONTRAST,), contrast=0.5, rects=[(1, 2, 3, 4), (5, 6, 7, 8)], gamma_table=np.arange(255, -1, -1))]]
    a = ag.Augmentation.from_values(rows, crop=[(3, 9)])
    t = a.table_host()
    assert t.shape == (2, 1, ag.ROW_INTS) and t.dtype == np.int32
    r = t[0, 0]
    assert r[0] == 1 and r[1] == (ag.HUE | ag.BRIGHTNESS << 8 | ag.NONE << 16 | ag.NONE << 24)
    assert r[2:5].view(np.float32).tolist() == [1.25, 1.0, 1.0] and r[5] == (int(-0.1 * 255) & 255) == 231
    assert (r[6], r[7], r[8]) == (3, 9, 0) and r[25:27].view(np.uint32).tolist() == [0x55667788, 0x11223344] and not r[27:32].any()
    assert np.array_equal(r[32:].view(np.uint8), ag.gamma_table(0.9))
    r = t[1, 0]
    assert r[8] == 2 and r[9:17].tolist() == [1, 2, 3, 4, 5, 6, 7, 8] and np.array_equal(r[32:].view(np.uint8), np.arange(255, -1, -1))
    ident = ag.Augmentation.identity(3, crop=[(0, 0), (1, 1), (2, 2)]).table_host()
    assert (ident[:, :, 0] == 0).all() and (ident[:, :, 1] == 0x04040404).all() and (ident[:, :, 8] == 0).all()
    with pytest.raises(ValueError):
        ag.Augmentation.from_values([[dict(order=('hue', 'hue'))]])
    with pytest.raises(ValueError):
        ag.Augmentation.from_values([[dict(rects=[(0, 0, 1, 1)] * 5)]])
    with pytest.raises(ValueError):
        ag.Augmentation.from_values([[dict(colour=1)]])
    with pytest.raises(ValueError):                                                  # host values that leave the window / the frame
        ag.Augmentation.from_values([[dict(rects=[(0, 0, 10, 33)])]]).check((40, 40), (32, 32))
    with pytest.raises(ValueError):
        ag.Augmentation.identity(1, crop=[(9, 0)]).check((40, 40), (32, 32))


def test_abi_entries():
    from temporalstereo_amd import _lib, build
    build.build(verbose=False)
    header = open(os.path.join(ROOT, "include", "ts_hip.h")).read()
    for name in ENTRIES + ("ts_frames_augment_workspace_bytes",):
        assert name in _lib.SIGNATURES and re.search(r"\b%s\s*\(" % name, header), name
    assert int(re.search(r"#define TS_AUGMENT_ROW_INTS (\d+)", header).group(1)) == ag.ROW_INTS
    assert int(re.search(r"#define TS_AUGMENT_MAX_RECTS (\d+)", header).group(1)) == ag.MAX_RECTS
    L = _lib.lib()
    import ctypes as C
    plan = L.ts_plan_create()
    w = (C.c_ulonglong * 32)()
    for name in ENTRIES:                                               # a launch plan can replay them
        assert name not in _lib._QUERIES
        assert L.ts_plan_add_call(plan, name.encode(), w, len(_lib.SIGNATURES[name][1])) == 0, name
    L.ts_plan_destroy(plan)
    assert L.ts_frames_augment_workspace_bytes(4, 540, 960) > 0 and L.ts_frames_augment_workspace_bytes(0, 540, 960) == 0
    one, m, s = C.c_void_p(256), MEAN, STD                             # a non-NULL, aligned, never dereferenced pointer
    f = L.ts_frames_augment_fwd
    assert f(None, None, 1, 8, 8, 0, *m, *s, 8, 8, one, one, None, 192, one, None, 192, one, 4096, None) == -1
    assert f(one, None, 1, 8, 8, 0, *m, *s, 8, 8, None, one, None, 192, one, None, 192, one, 4096, None) == -1      # no table
    assert f(one, None, 1, 8, 8, 0, *m, *s, 8, 8, one, None, None, 0, None, one, 192, one, 4096, None) == -1        # right output, no right image
    assert f(one, None, 0, 8, 8, 0, *m, *s, 8, 8, one, None, None, 0, one, None, 192, one, 4096, None) == -2
    assert f(one, None, 1, 8, 8, 0, *m, *s, 9, 8, one, None, None, 0, one, None, 216, one, 4096, None) == -2        # window > image
    assert f(one, None, 1, 8, 8, 0, *m, *s, 8, 8, one, None, None, 0, one, None, 191, one, 4096, None) == -2        # stride < image
    assert f(one, None, 1, 8, 8, 0, *m, *s, 8, 8, one, None, None, 0, one, None, 192, one, 0, None) == -2           # workspace too small
    assert f(one, None, 1, 8, 8, 2, *m, *s, 8, 8, one, None, None, 0, one, None, 192, one, 4096, None) == -2        # unknown flag
    d = L.ts_disp_u16_window_fwd
    assert d(None, 1, 8, 8, 4, 4, one, 256.0, one, None, None) == -1
    assert d(one, 1, 8, 8, 4, 4, None, 256.0, one, None, None) == -1
    assert d(one, 1, 8, 8, 9, 4, one, 256.0, one, None, None) == -2
    assert d(one, 1, 8, 8, 4, 4, one, 0.0, one, None, None) == -2


def test_public_names():
    for n in ("Augmentation", "draw_augmentation", "gamma_table", "augment_frames", "prepare_train_batch"):
        assert hasattr(ts, n), n
