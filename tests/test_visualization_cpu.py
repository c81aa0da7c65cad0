"""Colour maps and the 16-bit map (temporalstereo_amd/visualization.py): the fixtures' integrity (tests/golden/render_*.npz,
tools/gen_golden.py --only-render), the product's own jet table against the recorded matplotlib one, the refusals and the C ABI's
entries -- no GPU needed."""
import os
import re

import numpy as np
import pytest
import torch

from temporalstereo_amd import visualization as vz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CASES = ("render_dense", "render_sparse", "render_rescaled", "render_empty_range", "render_small_errors", "render_given_max",
         "render_batch3", "render_nonfinite")
TIES = ("class_tie", "jet_tie", "u16_tie")


@pytest.mark.parametrize("name", CASES)
def test_fixture_integrity(name):
    path = os.path.join(GOLDEN, name + ".npz")
    assert os.path.getsize(path) <= 100 * 1024
    g = dict(np.load(path))
    B, _, H, W = g["gt"].shape
    assert g["est"].shape[:2] == (B, 1) and g["est"].dtype == np.float32 and g["gt"].dtype == np.float32
    rescaled = str(g["group"]) == "rescaled"
    assert rescaled == (g["est"].shape[-2:] != (H, W))
    for k in ("class_idx", "jet_idx", "u16") + TIES:
        assert g[k].shape == (B, H, W), k
    assert g["bar_idx"].shape == (W,) and g["stats"].shape == (B, 4 + 18) and g["count_slack"].shape == (B, 6)
    if int(g["has_max"]):
        assert g["disp_color"].shape == (B, H, W, 3) and g["disp_color_u8_tie"].shape == (B, H, W, 3)
    else:
        assert g["cat_color"].shape == (B, 2 * H, W, 3) and g["cat_color_u8_tie"].shape == (B, 2 * H, W, 3)
    # the near-tie sets cannot grow to hide a failure: 1 % of a case's pixels, 8 % where the estimate is rescaled
    cap = 0.08 if rescaled else 0.01
    assert float(g["cap"]) == cap
    for k in g:
        if k.endswith("_tie"):
            assert g[k].dtype == np.bool_ and g[k].mean() <= cap, (k, g[k].mean())
    assert g["tau"].shape == (4,) and np.all(g["tau"] >= 0) and np.all(g["tau"] < 0.05)
    assert (float(g["rescale_dev"]) > 0) == rescaled


def test_fixture_set_and_provenance():
    total = sum(os.path.getsize(os.path.join(GOLDEN, f)) for f in os.listdir(GOLDEN) if f.startswith("render_"))
    assert total <= 1024 * 1024
    t = dict(np.load(os.path.join(GOLDEN, "render_tables.npz")))
    assert t["jet"].shape == (256, 3) and t["class_rgb"].shape == (10, 3) and t["class_bounds"].shape == (10,)
    versions = [str(v) for v in t["versions"]]
    assert len(versions) == 3 and all(re.match(r"\d+\.\d+", v) for v in versions)
    txt = open(os.path.join(GOLDEN, "PROVENANCE_render.txt")).read()
    for v in versions:
        assert v in txt
    assert "tau" in txt and "deviation" in txt
    for name in CASES:
        assert name in txt
    sizes = [tuple(np.load(os.path.join(GOLDEN, n + ".npz"))["gt"].shape[-2:]) for n in CASES]
    assert any(w % 4 for _, w in sizes) and any(w % 4 == 0 for _, w in sizes)      # a ragged width and a multiple of 4 both occur


def test_cases_hold_what_their_names_say():
    cnt = lambda n: np.load(os.path.join(GOLDEN, n + ".npz"))["stats"][:, -6:]
    assert cnt("render_empty_range")[0, 4] == 0 and np.all(np.delete(cnt("render_empty_range")[0], 4) > 0)
    assert np.all(cnt("render_small_errors")[0, 1:] == 0) and cnt("render_small_errors")[0, 0] > 0
    assert np.all(cnt("render_dense") > 0)
    g = np.load(os.path.join(GOLDEN, "render_sparse.npz"))
    assert 0.6 < (g["gt"] == 0).mean() < 0.8
    g = np.load(os.path.join(GOLDEN, "render_given_max.npz"))
    assert (g["est"] > g["max_disp"]).any() and (g["est"] < 0).any()
    g = np.load(os.path.join(GOLDEN, "render_batch3.npz"))
    assert len(set(g["stats"][:, 0].tolist())) == 3
    g = np.load(os.path.join(GOLDEN, "render_nonfinite.npz"))
    assert np.isnan(g["est"]).any() and np.isinf(g["est"]).any() and np.isnan(g["cat_color"]).any()


def test_jet_table_equals_recorded_matplotlib_table():
    ref = np.load(os.path.join(GOLDEN, "render_tables.npz"))["jet"]
    mine = vz.jet_table()
    assert mine.shape == (256, 3) and mine.dtype == np.float32
    # float32 rounding of a float64 table: at most one unit in the last place of a number below 1
    assert np.abs(mine.astype(np.float64) - ref).max() <= 2.0 ** -24


def test_cpu_tensors_are_refused():
    x = torch.zeros(1, 1, 8, 8)
    for call in (lambda: vz.disp_to_color(x), lambda: vz.disp_to_color(x[0, 0], 10.0), lambda: vz.disp_err_to_color(x, x),
                 lambda: vz.disp_err_to_colorbar(x, x), lambda: vz.disp_err_to_colorbar(x, x, with_bar=True),
                 lambda: vz.disp_to_uint16(x), lambda: vz.render_frame(x, x), lambda: vz.render_frame(x, size=(16, 16)),
                 lambda: vz.render_stats(x, x), lambda: vz.colormap(vz.disp_err_to_color, x, x, normalize=False)):
        with pytest.raises(RuntimeError, match="no CPU fallback"):
            call()


def test_argument_errors():
    x = torch.zeros(1, 1, 8, 8)
    with pytest.raises(ValueError, match="jet"):
        vz.disp_err_to_colorbar(x, x, cmap='hot')
    with pytest.raises(ValueError):
        vz.colormap('plasma', x)
    with pytest.raises(ValueError):
        vz.colormap(vz.disp_to_color, x, normalize=True)


def test_abi_entries():
    from temporalstereo_amd import _lib, build
    build.build(verbose=False)
    header = open(os.path.join(ROOT, "include", "ts_hip.h")).read()
    for name in ("ts_disp_render_workspace_bytes", "ts_disp_render_fwd"):
        assert name in _lib.SIGNATURES and re.search(r"\b%s\s*\(" % name, header), name
    assert "ts_disp_render_fwd" not in _lib._QUERIES and "ts_disp_render_workspace_bytes" in _lib._QUERIES
    assert int(re.search(r"#define TS_RENDER_STATS_FLOATS (\d+)", header).group(1)) == vz.STATS_FLOATS
    for flag in ("EST_COLOR", "GT_COLOR", "ERR_CLASS", "ERR_JET", "U16", "UINT8", "CHW", "BAR", "CLIP", "MAX_SHARED", "MAX_GIVEN"):
        assert int(re.search(r"#define TS_RENDER_%s (\d+)" % flag, header).group(1)) == getattr(vz, flag), flag
    L = _lib.lib()
    assert L.ts_version() >= 12
    assert L.ts_disp_render_workspace_bytes(1, 544, 960) > 0 and L.ts_disp_render_workspace_bytes(4, 544, 960) % 256 == 0
    assert L.ts_disp_render_workspace_bytes(2, 1, 1) > 0
    for args in ((0, 544, 960), (1, 0, 960), (1, 544, 0), (-1, 4, 4), (65536, 4, 4), (4096, 4096, 4096)):
        assert L.ts_disp_render_workspace_bytes(*args) == 0, args
    # validation happens before any launch
    z = [None] * 4
    assert L.ts_disp_render_fwd(*z, 1, 8, 8, 8, 8, vz.EST_COLOR, 256.0, *z, None, None, None) == -1
    assert b"NULL" in L.ts_last_error_string()
    assert L.ts_disp_render_fwd(*z, 1, 8, 8, 8, 8, 0, 256.0, *z, None, None, None) == -2                  # no output selected
    assert L.ts_disp_render_fwd(*z, 1, 8, 8, 8, 8, 1 << 11, 256.0, *z, None, None, None) == -2            # unknown flag
    assert L.ts_disp_render_fwd(*z, 1, 8, 8, 8, 8, vz.BAR | vz.U16, 256.0, *z, None, None, None) == -2    # legend without the jet map
    assert L.ts_disp_render_fwd(*z, 0, 8, 8, 8, 8, vz.U16, 256.0, *z, None, None, None) == -2
