"""Input preparation (temporalstereo_amd/preprocess.py): the C ABI's entries, the fixtures' integrity (tests/golden/prepare_*.npz,
tools/gen_golden.py --only-prepare) and the refusals that need no device -- no GPU needed."""
import os
import re

import numpy as np
import pytest
import torch

import temporalstereo_amd as ts
from temporalstereo_amd import preprocess as pp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
EXACT = ("prepare_same", "prepare_ramp", "prepare_train_crop")
RESIZED = ("prepare_dataset_up", "prepare_video_up", "prepare_down", "prepare_degenerate")
ENTRIES = ("ts_frames_prepare_fwd", "ts_intrinsics_pyramid_fwd", "ts_disp_u16_decode_fwd")


def load(name):
    return dict(np.load(os.path.join(GOLDEN, name + ".npz")))


def test_abi_entries():
    from temporalstereo_amd import _lib, build
    build.build(verbose=False)
    header = open(os.path.join(ROOT, "include", "ts_hip.h")).read()
    for name in ENTRIES:
        assert name in _lib.SIGNATURES and re.search(r"\b%s\s*\(" % name, header), name
        assert name not in _lib._QUERIES
    assert int(re.search(r"#define TS_PREPARE_CHW (\d+)", header).group(1)) == pp.CHW
    L = _lib.lib()
    assert L.ts_version() >= 13
    plan = L.ts_plan_create()
    import ctypes as C
    w = (C.c_ulonglong * 32)()
    for name in ENTRIES:                                               # a launch plan can replay them
        assert L.ts_plan_add_call(plan, name.encode(), w, len(_lib.SIGNATURES[name][1])) == 0, name
    L.ts_plan_destroy(plan)


def test_abi_refusals_before_any_launch():
    """null pointers, zero sizes and bad flags return the error status and set ts_last_error_string (nothing is launched)."""
    from temporalstereo_amd import _lib, build
    build.build(verbose=False)
    L = _lib.lib()
    m, s = pp.IMAGENET_MEAN, pp.IMAGENET_STD
    one = 16          # any non-null, aligned value: validation comes first and fails before a launch in every call below
    assert L.ts_frames_prepare_fwd(None, None, 1, 8, 8, 0, *m, *s, 8, 8, None, one, None, 192, one, None, 192, None) == -1
    assert b"NULL" in L.ts_last_error_string()
    assert L.ts_frames_prepare_fwd(one, None, 1, 8, 8, 0, *m, *s, 8, 8, None, None, None, 0, None, None, 0, None) == -1     # no output
    assert L.ts_frames_prepare_fwd(one, None, 1, 8, 8, 0, *m, *s, 8, 8, None, None, None, 0, None, one, 192, None) == -1    # right output, no right image
    assert L.ts_frames_prepare_fwd(one, None, 0, 8, 8, 0, *m, *s, 8, 8, None, None, None, 0, one, None, 192, None) == -2
    assert L.ts_frames_prepare_fwd(one, None, 1, 0, 8, 0, *m, *s, 8, 8, None, None, None, 0, one, None, 192, None) == -2
    assert L.ts_frames_prepare_fwd(one, None, 1, 8, 8, 0, *m, *s, 8, 0, None, None, None, 0, one, None, 192, None) == -2
    assert L.ts_frames_prepare_fwd(one, None, 1, 8, 8, 2, *m, *s, 8, 8, None, None, None, 0, one, None, 192, None) == -2    # unknown flag
    assert b"flags" in L.ts_last_error_string()
    assert L.ts_frames_prepare_fwd(one, None, 1, 8, 8, 0, *m, *s, 9, 8, one, None, None, 0, one, None, 216, None) == -2     # window > image
    assert b"9x8" in L.ts_last_error_string()
    assert L.ts_frames_prepare_fwd(one, None, 1, 8, 8, 0, *m, *s, 8, 8, None, None, None, 0, one, None, 191, None) == -2    # stride < image
    assert L.ts_frames_prepare_fwd(one, None, 1, 8, 8, 0, *m, 0.0, 1.0, 1.0, 8, 8, None, None, None, 0, one, None, 192, None) == -2
    assert L.ts_intrinsics_pyramid_fwd(None, 0, 1, 8, 8, 1, one, one, None) == -1
    assert L.ts_intrinsics_pyramid_fwd(one, 0, 1, 8, 8, 1, None, one, None) == -1
    assert L.ts_intrinsics_pyramid_fwd(one, 0, 0, 8, 8, 1, one, one, None) == -2
    assert L.ts_intrinsics_pyramid_fwd(one, 0, 1, 8, 8, 0, one, one, None) == -2
    assert L.ts_intrinsics_pyramid_fwd(one, 2, 1, 8, 8, 1, one, one, None) == -2
    assert L.ts_intrinsics_pyramid_fwd(one, 0, 1, 8, 8, 5, one, one, None) == -2            # 8 >> 4 == 0: a singular K
    assert b"singular" in L.ts_last_error_string()
    assert L.ts_disp_u16_decode_fwd(None, 1, 8, 8, 256.0, one, None, None) == -1
    assert L.ts_disp_u16_decode_fwd(one, 1, 8, 8, 256.0, None, None, None) == -1
    assert L.ts_disp_u16_decode_fwd(one, 1, 0, 8, 256.0, one, None, None) == -2
    assert L.ts_disp_u16_decode_fwd(one, 1, 8, 8, 0.0, one, None, None) == -2


def test_exports_and_defaults():
    for name in ("prepare_frames", "prepare_batch", "intrinsics_pyramid", "disp_from_uint16"):
        assert getattr(ts, name) is getattr(pp, name)
    # the reference's defaults (architecture/data/datasets/base.py:41)
    assert pp.IMAGENET_MEAN == (0.485, 0.456, 0.406) and pp.IMAGENET_STD == (0.229, 0.224, 0.225)
    assert pp.default_num_scales((544, 960)) == 9 and pp.default_num_scales((24, 36)) == 4


@pytest.mark.parametrize("name", EXACT + RESIZED)
def test_fixture_integrity(name):
    path = os.path.join(GOLDEN, name + ".npz")
    assert os.path.getsize(path) <= 110 * 1024
    g = load(name)
    subs = int(g["subs"])
    assert subs >= 1
    resized = name in RESIZED
    assert ("dev32_64" in g) == resized
    if resized:
        assert 0 < float(g["dev32_64"]) < 1e-4
    for k in range(subs):
        L, R = g["left%d" % k], g["right%d" % k]
        assert L.dtype == np.uint8 and L.shape == R.shape and L.ndim == 4 and L.shape[-1] == 3
        B, Hs, Ws, _ = L.shape
        for s in "lr":
            a, c = g["aug_%s%d" % (s, k)], g["color_%s%d" % (s, k)]
            assert a.dtype == np.float32 and c.dtype == np.float32 and a.shape[:2] == (B, 3) and c.shape[:2] == (B, 3)
            H, W = a.shape[-2:]
            assert ((H, W) != (Hs, Ws)) == (resized or "crop%d" % k in g)
            assert c.shape[-2:] == ((H, W) if "crop%d" % k in g else (Hs, Ws))
            assert 0.0 <= c.min() and c.max() <= 1.0 and -2.2 < a.min() and a.max() < 2.7
            assert (("d64_%s%d" % (s, k)) in g) == resized
            if resized:
                d = g["d64_%s%d" % (s, k)]
                assert d.shape == a.shape and np.abs(d).max() <= float(g["dev32_64"])
        if "K%d" % k in g:
            K, inv = g["K%d" % k], g["inv_K%d" % k]
            assert K.dtype == np.float32 and K.shape == inv.shape and K.shape[0] in (1, B) and K.shape[2:] == (4, 4)
            assert g["K_norm%d" % k].shape == (4, 4) and g["k_size%d" % k].shape == (2,)
            eye = np.einsum("bsij,bsjk->bsik", K.astype(np.float64), inv.astype(np.float64))
            assert np.abs(eye - np.eye(4)).max() < 1e-6


def test_cases_hold_what_their_names_say():
    g = load("prepare_ramp")
    assert sorted(g["left%d" % k].shape[2] % 4 for k in range(3)) == [1, 2, 3]
    for k in range(3):
        for c in range(3):
            assert len(np.unique(g["left%d" % k][..., c])) == 256
    g = load("prepare_train_crop")
    B, Hs, Ws, _ = g["left0"].shape
    H, W = g["aug_l0"].shape[-2:]
    assert g["crop0"].tolist() == [[0, 0], [Hs - H, Ws - W]] and tuple(g["k_size0"]) == (Hs, Ws)
    g = load("prepare_dataset_up")
    assert g["left0"].shape[0] == 2 and tuple(g["k_size0"]) == g["aug_l0"].shape[-2:] and g["K0"].shape[1] == 4
    g = load("prepare_down")
    assert g["aug_l0"].shape[-1] < g["left0"].shape[2] and g["aug_l0"].shape[-2] < g["left0"].shape[1]
    g = load("prepare_degenerate")
    assert g["left0"].shape[1] == 1 and g["left1"].shape[2] == 1 and g["aug_l2"].shape[-2] == 1
    g = load("prepare_disp16")
    raw = g["raw0"]
    assert raw.dtype == np.uint16 and {0, 1, 65535} <= set(raw[0, 0, :3].tolist()) and 0.1 < (raw == 0).mean() < 0.5
    assert np.array_equal(g["valid0"][:, 0], raw > 0) and np.array_equal(g["disp0"][:, 0], raw.astype(np.float32) / 256)
    txt = open(os.path.join(GOLDEN, "PROVENANCE_prepare.txt")).read()
    for name in EXACT + RESIZED + ("prepare_disp16",):
        assert name in txt
    assert "stand-in" in txt and "dev32_64" in txt


def test_cpu_tensors_are_refused():
    img = torch.zeros(8, 8, 3, dtype=torch.uint8)
    for call in (lambda: pp.prepare_frames(img), lambda: pp.prepare_frames(img, img, size=(16, 16)),
                 lambda: pp.intrinsics_pyramid(torch.eye(4), (8, 8)), lambda: pp.disp_from_uint16(torch.zeros(4, 4, dtype=torch.int16)),
                 lambda: pp.prepare_batch(img, img, torch.eye(4), 0.54, (8, 8))):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


def test_argument_errors_without_a_device():
    """the shape / dtype refusals come before the device check, with the offending shape in the message"""
    u8 = lambda *s: torch.zeros(*s, dtype=torch.uint8)
    with pytest.raises(TypeError, match=r"uint8.*\(8, 8, 3\)"):
        pp.prepare_frames(torch.zeros(8, 8, 3))
    with pytest.raises(ValueError, match=r"three channels.*\(8, 8, 4\)"):
        pp.prepare_frames(u8(8, 8, 4))
    with pytest.raises(ValueError, match=r"three channels.*\(8, 8, 3\)"):
        pp.prepare_frames(u8(8, 8, 3), layout='CHW')
    with pytest.raises(ValueError, match=r"empty batch.*\(0, 8, 8, 3\)"):
        pp.prepare_frames(u8(0, 8, 8, 3))
    with pytest.raises(ValueError, match=r"left has shape \(8, 8, 3\), right \(8, 9, 3\)"):
        pp.prepare_frames(u8(8, 8, 3), u8(8, 9, 3))
    with pytest.raises(ValueError, match="layout"):
        pp.prepare_frames(u8(8, 8, 3), layout='NHWC')
