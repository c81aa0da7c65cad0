"""numpy restatement of the colour augmentation's arithmetic (PIL's ImageEnhance blends, its RGB <-> HSV conversions, the grey
conversion, Image.point) and of the frame chain built on it: full uint8 frame -> operations in order -> gamma table -> / 255 ->
normalise -> crop.  Written from the definitions in temporalstereo_amd/csrc/augment.hip's header; doubles exactly where PIL's C code
computes in double.  tests/test_augment_cpu.py pins it to PIL-made fixtures; the GPU tests compare the kernels with it at full size."""
import numpy as np

BRIGHTNESS, CONTRAST, SATURATION, HUE, NONE = 0, 1, 2, 3, 4


def grey(img):
    """uint8 [..., 3] -> int64 [...]"""
    x = img.astype(np.int64)
    return (19595 * x[..., 0] + 38470 * x[..., 1] + 7471 * x[..., 2] + 0x8000) >> 16


def blend(deg, x, f):
    """deg, x: integer arrays (broadcast); f: the factor, rounded to fp32 as PIL's C entry takes it"""
    f = np.float32(f)
    d = (np.asarray(x, dtype=np.int64) - np.asarray(deg, dtype=np.int64)).astype(np.float32)
    t = np.asarray(deg, dtype=np.int64).astype(np.float32) + f * d          # fp32 product, fp32 sum: two roundings
    out = np.where(t <= 0, 0, np.where(t >= 255, 255, np.trunc(t))).astype(np.uint8)
    return out


def brightness(img, f):
    return blend(0, img, f)


def contrast_mean(img):
    g = grey(img)
    return int(float(g.sum()) / float(g.size) + 0.5)


def contrast(img, f, m=None):
    return blend(contrast_mean(img) if m is None else m, img, f)


def saturation(img, f):
    return blend(grey(img)[..., None], img, f)


def rgb_to_hsv(img):
    x = img.astype(np.int64)
    r, g, b = x[..., 0], x[..., 1], x[..., 2]
    maxc, minc = x.max(-1), x.min(-1)
    flat = maxc == minc
    with np.errstate(divide='ignore', invalid='ignore'):
        cr = (maxc - minc).astype(np.float32)
        s = cr / maxc.astype(np.float32)
        rc = (maxc - r).astype(np.float32) / cr
        gc = (maxc - g).astype(np.float32) / cr
        bc = (maxc - b).astype(np.float32) / cr
        h0 = bc - gc
        h1 = (2.0 + rc.astype(np.float64) - bc.astype(np.float64)).astype(np.float32)
        h2 = (4.0 + gc.astype(np.float64) - rc.astype(np.float64)).astype(np.float32)
        h = np.where(r == maxc, h0, np.where(g == maxc, h1, h2))
        h = np.fmod(h.astype(np.float64) / 6.0 + 1.0, 1.0).astype(np.float32)
        H = np.clip(np.nan_to_num(h.astype(np.float64) * 255.0).astype(np.int64), 0, 255)
        S = np.clip(np.nan_to_num(s.astype(np.float64) * 255.0).astype(np.int64), 0, 255)
    H = np.where(flat, 0, H)
    S = np.where(flat, 0, S)
    return np.stack([H, S, maxc], -1).astype(np.uint8)


def _round_half_away(v):
    return np.where(v >= 0, np.floor(v + 0.5), np.ceil(v - 0.5))


def hsv_to_rgb(hsv):
    x = hsv.astype(np.int64)
    H, S, V = x[..., 0], x[..., 1], x[..., 2]
    fs = (S.astype(np.float64) / 255.0).astype(np.float32)
    h6 = H.astype(np.float64) * 6.0 / 255.0
    i = np.floor(h6).astype(np.int64)
    f = (h6 - i.astype(np.float32).astype(np.float64)).astype(np.float32)
    dv, dfs, df = V.astype(np.float64), fs.astype(np.float64), f.astype(np.float64)
    fsf = (fs * f).astype(np.float64)                                        # a float product in C
    p = np.clip(_round_half_away(dv * (1.0 - dfs)), 0, 255).astype(np.int64)
    q = np.clip(_round_half_away(dv * (1.0 - fsf)), 0, 255).astype(np.int64)
    t = np.clip(_round_half_away(dv * (1.0 - dfs * (1.0 - df))), 0, 255).astype(np.int64)
    k = i % 6
    r = np.choose(k, [V, q, p, p, t, V])
    g = np.choose(k, [t, V, V, q, p, p])
    b = np.choose(k, [p, p, t, V, V, q])
    grey_px = S == 0
    out = np.stack([np.where(grey_px, V, r), np.where(grey_px, V, g), np.where(grey_px, V, b)], -1)
    return out.astype(np.uint8)


def hue_shift_byte(f):
    """uint8(int(f * 255)) with the wrap of a negative value"""
    return int(f * 255) & 255


def hue(img, f=None, shift=None):
    hsv = rgb_to_hsv(img)
    sh = hue_shift_byte(f) if shift is None else int(shift)
    hsv[..., 0] = ((hsv[..., 0].astype(np.int64) + sh) & 255).astype(np.uint8)
    return hsv_to_rgb(hsv)


def color_chain(img, order, factors, hue_shift=None, table=None):
    """img: uint8 [H,W,3], the FULL frame.  order: operation codes in the order applied (NONE entries are skipped);
    factors: (brightness, contrast, saturation, hue); hue_shift overrides the byte derived from factors[3]; table: 256 bytes or None."""
    out = np.ascontiguousarray(img)
    for op in order:
        if op == BRIGHTNESS:
            out = brightness(out, factors[0])
        elif op == CONTRAST:
            out = contrast(out, factors[1])
        elif op == SATURATION:
            out = saturation(out, factors[2])
        elif op == HUE:
            out = hue(out, factors[3], hue_shift)
    if table is not None:
        out = np.asarray(table, dtype=np.uint8)[out]
    return out


def to_color(img):
    """uint8 [H,W,3] -> fp32 [3,H,W] = byte / 255"""
    return (img.astype(np.float32) / np.float32(255)).transpose(2, 0, 1)


def normalise(img, mean, std):
    v = img.astype(np.float32) / np.float32(255)
    m, s = np.asarray(mean, dtype=np.float32), np.asarray(std, dtype=np.float32)
    return ((v - m) / s).transpose(2, 0, 1)


def frame(img, order, factors, hue_shift, table, crop, size, mean, std):
    """One image -> (stage uint8 [Hs,Ws,3], color fp32 [3,H,W], color_aug fp32 [3,H,W]) without the rectangles."""
    stage = color_chain(img, order, factors, hue_shift, table)
    (ch, cw), (H, W) = crop, size
    return (stage, np.ascontiguousarray(to_color(img)[:, ch:ch + H, cw:cw + W]),
            np.ascontiguousarray(normalise(stage, mean, std)[:, ch:ch + H, cw:cw + W]))


def rect_mask(rects, size):
    """bool [H,W]: the union of (sh, sw, occh, occw) rectangles clipped to the window"""
    H, W = size
    m = np.zeros((H, W), dtype=bool)
    for sh, sw, oh, ow in rects:
        m[max(sh, 0):max(sh + oh, 0), max(sw, 0):max(sw + ow, 0)] = True
    return m
