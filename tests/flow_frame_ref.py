"""numpy restatement, in float32, of the optical-flow metrics, colour maps and KITTI decode that csrc/flow_frame.hip runs on the
device -- the reference's flow_calc_error (architecture/data/evaluation/flow_pixel_error.py:9-96), flow_max_rad / flow_to_color /
flow_err_to_color (architecture/utils/visualization/flow_colormap.py:8-220) and the arithmetic of load_png
(architecture/data/utils/load_flow.py:54-78) -- plus this project's rescale of an estimate to the ground truth's size.

Every operation is one rounded float32 operation, in the reference's order; where the device deliberately differs from the
reference, this file follows the device and says so:
  - the colours are normalised and interpolated in float32 (the reference divides by the float64 scalar max_rad + eps, so from
    there on it is float64); only the angle is atan2 in float64, rounded once to float32;
  - with a maximum taken from the data, "inside the disc" is r <= max_rad on the unnormalised radius (`data_max=True`); the
    reference can find the pixel that set the maximum a rounding outside and darken it.
tests/test_flow_frame_cpu.py pins it to the reference-made fixtures tests/golden/flow_frame_*.npz; tools/gen_golden.py
--only-flow-frame measures its distance from the reference, which sets the tolerances of tests/test_flow_frame_gpu.py."""
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
F32 = np.float32
KEYS = ('1px', '2px', '3px', '5px', 'epe')
UNKNOWN = F32(1e7)
CLASS_LO = np.array([0, 0.1875, 0.375, 0.75, 1.5, 3, 6, 12, 24, 48], dtype=np.float32)
CLASS_RGB = np.array([[49, 54, 149], [69, 117, 180], [116, 173, 209], [171, 217, 233], [224, 243, 248], [254, 224, 144],
                      [253, 174, 97], [244, 109, 67], [215, 48, 39], [165, 0, 38]], dtype=np.float32)
CASES = ("dense", "sparse", "none_valid", "nonfinite", "ragged", "tiny1", "tiny35", "batch3", "given_max", "shared", "rescaled")


# ------------------------------------------------------------------------------------------------------------------- fixtures
def dequant(q, idx, val):
    """int16 in 1/64 px -> float32, then the planted values (NaN, +-inf, > 1e7, -0.0) at their flat indices."""
    a = q.astype(np.float32) / F32(64)
    a.reshape(-1)[idx] = val
    return a


def load_fixture(name):
    """tests/golden/flow_frame_<name>.npz with `est` [B,2,h,w] and `gt` [B,2,H,W] rebuilt as float32."""
    g = dict(np.load(os.path.join(GOLDEN, "flow_frame_%s.npz" % name)))
    g["est"] = dequant(g["est_q64"], g["est_special_idx"], g["est_special_val"])
    g["gt"] = dequant(g["gt_q64"], g["gt_special_idx"], g["gt_special_val"])
    return g


def hwc(a):
    """[B,2,H,W] -> [B,H,W,2], contiguous"""
    return np.ascontiguousarray(np.moveaxis(a, -3, -1))


# -------------------------------------------------------------------------------------------------------------------- metrics
def radius(a, b):
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    with np.errstate(all='ignore'):
        return np.sqrt(a * a + b * b)


def valid_mask(gt, lb=0.0, ub=400, sparse=False):
    """gt [B,2,H,W] -> bool [B,H,W]"""
    gu, gv = gt[:, 0], gt[:, 1]
    m = np.ones(gu.shape, dtype=bool)
    if sparse:
        m &= ~((np.abs(gu) < F32(1e-12)) & (np.abs(gv) < F32(1e-12)))
    m &= ~(np.isnan(gu) | np.isnan(gv))
    rad = radius(gu, gv)
    with np.errstate(all='ignore'):
        return m & (rad > F32(lb)) & (rad < F32(ub))


def flow_error(est, gt):
    with np.errstate(all='ignore'):
        return radius(gt[:, 0] - est[:, 0], gt[:, 1] - est[:, 1])


def calc_error(est, gt, lb=0.0, ub=400, sparse=False):
    """-> float32 [5] = {1px, 2px, 3px, 5px, epe} and N.  The percentages are the reference's bits; epe is the float64 mean
    rounded once (the reference: a float32 mean)."""
    m = valid_mask(gt, lb, ub, sparse)
    n = int(m.sum())
    if n < 1:
        return np.zeros(5, dtype=np.float32), 0
    e = flow_error(est, gt)[m]
    with np.errstate(all='ignore'):
        pct = [F32(int((e > F32(t)).sum())) / F32(n) * F32(100) for t in (1, 2, 3, 5)]
        return np.array(pct + [F32(e.astype(np.float64).sum() / n)], dtype=np.float32), n


def rescale(est, size):
    """est [B,2,h,w] at size (Hg, Wg): align-corners bilinear, then u * Wg / w and v * Hg / h, in float32.  The device contracts
    some of the products and sums into fused multiply-adds, so this is equal to it only to a few units in the last place."""
    B, _, h, w = est.shape
    Hg, Wg = size
    if (h, w) == (Hg, Wg):
        return est.copy()

    def src(n_in, n_out):
        s = F32(n_in - 1) / F32(n_out - 1) if n_out > 1 else F32(0)
        p = s * np.arange(n_out, dtype=np.float32)
        i0 = p.astype(np.int64)
        return i0, i0 + (i0 < n_in - 1), p - i0.astype(np.float32)
    y0, y1, ly = src(h, Hg)
    x0, x1, lx = src(w, Wg)
    ly = ly.reshape(1, 1, Hg, 1)
    top = (F32(1) - lx) * est[:, :, y0][..., x0] + lx * est[:, :, y0][..., x1]
    bot = (F32(1) - lx) * est[:, :, y1][..., x0] + lx * est[:, :, y1][..., x1]
    out = (F32(1) - ly) * top + ly * bot
    scale = np.array([F32(Wg) / F32(w), F32(Hg) / F32(h)], dtype=np.float32).reshape(1, 2, 1, 1)
    return (out * scale).astype(np.float32)


# -------------------------------------------------------------------------------------------------------------------- colours
def make_color_wheel():
    """float64 [55, 3], values 0..255: red-yellow 15, yellow-green 6, green-cyan 4, cyan-blue 11, blue-magenta 13, magenta-red 6"""
    arcs = ((15, 0, 1, 1), (6, 1, 0, -1), (4, 1, 2, 1), (11, 2, 1, -1), (13, 2, 0, 1), (6, 0, 2, -1))
    rows = []
    for n, held, ramp, sign in arcs:
        a = np.zeros((n, 3))
        a[:, held] = 255
        step = np.floor(255 * np.arange(n) / n)
        a[:, ramp] = step if sign > 0 else 255 - step
        rows.append(a)
    return np.concatenate(rows)


def unknown(flow):
    """flow [..., H, W, 2] -> bool [..., H, W]"""
    u, v = flow[..., 0], flow[..., 1]
    with np.errstate(all='ignore'):
        return (np.abs(u) > UNKNOWN) | (np.abs(v) > UNKNOWN) | np.isnan(u) | np.isnan(v)


def known(flow):
    """flow with its unknown pixels as (+0, +0) (a copy)"""
    f = np.array(flow, dtype=np.float32, copy=True)
    f[unknown(flow)] = 0
    return f


def max_rad(flow):
    """flow [H,W,2] -> float32: the maximum radius with unknown pixels as 0"""
    f = known(flow)
    return F32(np.max(radius(f[..., 0], f[..., 1])))


def flow_to_color(flow, max_rad_=None, data_max=None):
    """flow [H,W,2] -> float32 [H,W,3].  max_rad_ None: the map's own maximum.  data_max: whether the maximum came from the data
    (default: when max_rad_ is None) -- then inside = r <= max_rad_ on the unnormalised radius, else rad <= 1 on the normalised one."""
    unk = unknown(flow)
    f = known(flow)
    u, v = f[..., 0], f[..., 1]
    r0 = radius(u, v)
    if data_max is None:
        data_max = max_rad_ is None
    m = F32(np.max(r0)) if max_rad_ is None else F32(max_rad_)
    den = m + F32(2.0 ** -52)
    with np.errstate(all='ignore'):
        un, vn = u / den, v / den
        rad = radius(un, vn)
        ang = np.arctan2((-vn).astype(np.float64), (-un).astype(np.float64)).astype(np.float32)
        a = ang / F32(np.pi)
        fk = (a + F32(1)) * F32(0.5) * F32(54) + F32(1)
        k0 = np.where(fk >= 1, np.where(fk < 55, np.nan_to_num(fk, nan=1.0).astype(np.int64), 55), 1)
        k1 = np.where(k0 == 55, 1, k0 + 1)
        fr = fk - k0.astype(np.float32)
        g = F32(1) - fr
        inside = (r0 <= m) if data_max else (rad <= F32(1))
        wheel = make_color_wheel().astype(np.float32) / F32(255)
        img = np.zeros(u.shape + (3,), dtype=np.float32)
        for c in range(3):
            col = g * wheel[k0 - 1, c] + fr * wheel[k1 - 1, c]
            img[..., c] = np.where(inside, F32(1) - rad * (F32(1) - col), col * F32(0.75))
    img[unk] = 0
    return img


def norm_radius(flow, m):
    """the normalised radius flow_to_color compares with 1, for a maximum m: float32 [H,W]"""
    f = known(flow)
    den = F32(m) + F32(2.0 ** -52)
    with np.errstate(all='ignore'):
        return radius(f[..., 0] / den, f[..., 1] / den)


def err_class(est, gt, val=None):
    """est, gt [..., 2, H, W] (val [..., H, W] or None) -> int8 class 0..9 per pixel, -1: black"""
    with np.errstate(all='ignore'):
        E = radius(gt[..., 0, :, :] - est[..., 0, :, :], gt[..., 1, :, :] - est[..., 1, :, :])
        ok = np.ones(E.shape, dtype=bool)
        if val is not None:
            E = E * val.astype(np.float32)
            ok = val != 0
        ok &= E >= 0
        cls = np.zeros(E.shape, dtype=np.int64)
        for k in range(1, 10):
            cls += E >= CLASS_LO[k]
    return np.where(ok, cls, -1).astype(np.int8)


def class_colors(cls):
    """class map -> float32 [..., 3] colours, black for -1"""
    table = np.concatenate([CLASS_RGB / F32(255), np.zeros((1, 3), dtype=np.float32)])
    return table[cls.astype(np.int64)]


def class_counts(cls):
    """class map [B,H,W] -> int [B,10]"""
    return np.stack([(cls == k).reshape(cls.shape[0], -1).sum(axis=1) for k in range(10)], axis=1)


def q8(v):
    """the uint8 code of a float32 colour: floor(255 v + 0.5) after a clamp to [0,1], NaN -> 0"""
    v = np.asarray(v, dtype=np.float32)
    with np.errstate(all='ignore'):
        c = np.clip(np.nan_to_num(v, nan=0.0), F32(0), F32(1))
        return np.floor(F32(255) * c + F32(0.5)).astype(np.uint8)


# --------------------------------------------------------------------------------------------------------------------- decode
def decode_kitti(raw):
    """raw uint16 [B,H,W,3] -> flow float32 [B,2,H,W], valid bool [B,1,H,W]"""
    ok = raw[..., 2] != 0
    f = (raw[..., :2].astype(np.float32) - F32(32768)) / F32(64)
    f[~ok] = 0
    return np.ascontiguousarray(np.moveaxis(f, -1, 1)), ok[:, None]
