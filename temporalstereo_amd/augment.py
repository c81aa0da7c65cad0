"""Training frames augmented on the device, on the kernels of csrc/augment.hip: uint8 frames and one parameter table in, the
training form of the batch dictionary out.

What the reference does on the host for every training image (architecture/data/datasets/base.py:65-187), restated:
  build_transform   :73-90     ColorJitter(brightness (0.4, 2.0), contrast (0.5, 1.5), saturation (0.5, 1.5), hue (-0.1, 0.1)) -- the four
                               operations in a random order, each with a random factor -- then AdjustGamma(0.8, 1.2, gain 1.0)
  do_transform      :99-130    color = ToTensor(image); color_aug = normalize(ToTensor(color_aug(image))): the colour operations
                               run on the FULL uint8 PIL image
                    :137-155   one random crop origin (ch, cw) for every tensor of the sample, the ground truth included
                    :157-173   with probability 0.5, 2-4 rectangles of N(0, 0.1) noise (normalised) over the RIGHT eye's color_aug

The split kept here: the random DRAWS stay on the host (`draw_augmentation`, or explicit values through `Augmentation.from_values`),
the PIXELS stay on the device.  An `Augmentation` holds the host values and ONE int32 device tensor, `table` [eyes,B,96] (the row
layout: include/ts_hip.h); the kernels read nothing else, so a captured step is replayed on new draws by `aug.refill(other)`.

Semantics kept from the reference:
  - every uint8 stage has PIL 12's bytes (ImageEnhance.Brightness / Contrast / Color, the HSV round trip with torchvision's uint8 hue
    shift, Image.point), and the floats are ((byte / 255) - mean[c]) / std[c] with correctly rounded divisions: outside the
    rectangles color_aug has the reference's bits;
  - contrast blends towards the mean grey level of the whole frame as it stands when contrast is applied (a reduction launch);
  - the rectangles are applied in order (a later one overwrites an earlier one), on the cropped color_aug of the right eye.
Differences, deliberate:
  - the noise inside a rectangle is N(0, 0.1) from a counter-based generator on the device (Philox-4x32-10 keyed by the row's seed,
    counted by position in the rectangle, channel and rectangle): the reference's numpy stream is not reproduced, and its
    `noise + mean - mean` (:172-173, the identity up to float64 rounding) is not computed;
  - the gamma operation is a 256-byte table per image and eye; `gamma_table` is the truncating table of torchvision's current PIL
    path (older torchvision versions hand PIL a float table, which PIL rounds); an explicit table can be given instead;
  - host values are checked (a crop outside the frame, a rectangle outside the window are refused); what is already in the device
    table cannot be inspected without a synchronisation and is clamped / clipped by the kernel.
uint8 GPU tensors only: a CPU tensor raises, there is no CPU fallback.
"""
import numpy as np
import torch

from . import _lib
from .functional import _stream
from ._frameio import _batch_dict, _color_outputs, _frames, _gt_rows, _on_gpu, _three, _u16_map
from .preprocess import CHW, IMAGENET_MEAN, IMAGENET_STD, default_num_scales

ROW_INTS = 96                               # TS_AUGMENT_ROW_INTS (include/ts_hip.h)
MAX_RECTS = 4                               # TS_AUGMENT_MAX_RECTS
BRIGHTNESS, CONTRAST, SATURATION, HUE, NONE = 0, 1, 2, 3, 4
_NAMES = {'brightness': BRIGHTNESS, 'contrast': CONTRAST, 'saturation': SATURATION, 'hue': HUE, 'none': NONE, None: NONE}


def gamma_table(gamma, gain=1.0):
    """The 256 bytes of adjust_gamma on a PIL image: min(255, int((255 + 1 - 1e-3) * gain * (e / 255.0) ** gamma)), the truncating
    table of torchvision's current PIL path, in Python floats.  gamma_table(1.0) is the identity."""
    gamma, gain = float(gamma), float(gain)
    if gamma < 0:
        raise ValueError("gamma_table: gamma must be non-negative (got %r)" % gamma)
    return np.array([min(255, int((255 + 1 - 1e-3) * gain * (e / 255.0) ** gamma)) for e in range(256)], dtype=np.uint8)


def _f32_bits(v):
    return int(np.array([v], dtype=np.float32).view(np.int32)[0])


class Augmentation:
    """The parameters of one batch: host values (numpy, for logging and tests) and `table`, the int32 device tensor
    [eyes,B,ROW_INTS] the kernels read.  Per image b and eye e (0 left, 1 right):
      order[e,b]      four operation codes in the order applied (BRIGHTNESS, CONTRAST, SATURATION, HUE; NONE = skipped)
      factors[e,b]    (brightness, contrast, saturation, hue) as drawn; hue_shift[e,b] = uint8(int(hue * 255)), what the kernel adds
      gamma_on[e,b]   whether gamma_tables[e,b] (256 bytes) is applied; gamma[e,b] / gain[e,b] the values it was made from (nan: given)
      crop[b]         (ch, cw), one origin for both eyes and the ground truth
      rects[e][b]     up to four (sh, sw, occh, occw) in window coordinates, in the order applied
      seeds[e,b]      the 64-bit key of the rectangle noise"""

    def __init__(self, order, factors, gamma_on, gamma_tables, crop, rects, seeds, gamma=None, gain=None, hue_shift=None, device=None):
        self.order = np.asarray(order, dtype=np.int64)
        if self.order.ndim != 3 or self.order.shape[2] != 4:
            raise ValueError("Augmentation: order must be [eyes,B,4] (got %s)" % (self.order.shape,))
        self.eyes, self.B = int(self.order.shape[0]), int(self.order.shape[1])
        E, B = self.eyes, self.B
        if E not in (1, 2) or B <= 0:
            raise ValueError("Augmentation: %d eyes, %d images" % (E, B))
        self.factors = np.asarray(factors, dtype=np.float64).reshape(E, B, 4)
        self.gamma_on = np.asarray(gamma_on, dtype=bool).reshape(E, B)
        self.gamma_tables = np.asarray(gamma_tables, dtype=np.uint8).reshape(E, B, 256)
        self.gamma = np.full((E, B), np.nan) if gamma is None else np.asarray(gamma, dtype=np.float64).reshape(E, B)
        self.gain = np.full((E, B), np.nan) if gain is None else np.asarray(gain, dtype=np.float64).reshape(E, B)
        self.crop = np.asarray(crop, dtype=np.int64).reshape(B, 2)
        self.rects = [[[tuple(int(v) for v in r) for r in rects[e][b]] for b in range(B)] for e in range(E)]
        self.seeds = np.asarray(seeds, dtype=np.uint64).reshape(E, B)
        self.hue_shift = (np.array([[int(self.factors[e, b, 3] * 255) & 255 for b in range(B)] for e in range(E)], dtype=np.int64)
                          if hue_shift is None else np.asarray(hue_shift, dtype=np.int64).reshape(E, B))
        for e in range(E):
            for b in range(B):
                ops = [int(o) for o in self.order[e, b]]
                real = [o for o in ops if o != NONE]
                if any(o not in (BRIGHTNESS, CONTRAST, SATURATION, HUE, NONE) for o in ops) or len(set(real)) != len(real):
                    raise ValueError("Augmentation: order %s of image %d, eye %d: each operation at most once" % (ops, b, e))
                if len(self.rects[e][b]) > MAX_RECTS or any(len(r) != 4 or r[2] <= 0 or r[3] <= 0 for r in self.rects[e][b]):
                    raise ValueError("Augmentation: rectangles %s of image %d, eye %d: at most %d of (sh, sw, occh > 0, occw > 0)"
                                     % (self.rects[e][b], b, e, MAX_RECTS))
                if not 0 <= self.hue_shift[e, b] <= 255:
                    raise ValueError("Augmentation: hue shift %d" % self.hue_shift[e, b])
        if not np.all(np.isfinite(self.factors)):
            raise ValueError("Augmentation: a factor is not finite")
        self.table = None
        if device is not None:
            self.table = torch.from_numpy(self.table_host()).to(device)        # the ONE host-to-device copy

    # ---------------------------------------------------------------------------------------------------------- constructors
    @classmethod
    def from_values(cls, rows, crop=None, device=None):
        """rows[e][b]: a dict per eye and image with any of
             order ('brightness' / 'contrast' / 'saturation' / 'hue' names or codes, in the order applied; default: none),
             brightness, contrast, saturation (factors, default 1.0), hue (default 0.0; the round trip through HSV bytes runs
             whenever 'hue' is in the order, as in torchvision), gamma (+ gain) or gamma_table (256 bytes), rects, seed.
        crop: one (ch, cw) per image (default (0, 0))."""
        E, B = len(rows), len(rows[0])
        if any(len(r) != B for r in rows):
            raise ValueError("Augmentation.from_values: the eyes hold different numbers of images")
        order = np.full((E, B, 4), NONE, dtype=np.int64)
        factors = np.tile(np.array([1.0, 1.0, 1.0, 0.0]), (E, B, 1))
        on = np.zeros((E, B), dtype=bool)
        tabs = np.tile(np.arange(256, dtype=np.uint8), (E, B, 1))
        gam, gain = np.full((E, B), np.nan), np.full((E, B), np.nan)
        rects = [[[] for _ in range(B)] for _ in range(E)]
        seeds = np.zeros((E, B), dtype=np.uint64)
        for e in range(E):
            for b in range(B):
                d = dict(rows[e][b])
                ops = [(_NAMES[o] if (o is None or isinstance(o, str)) else int(o)) for o in d.pop('order', ())]
                if len(ops) > 4:
                    raise ValueError("Augmentation.from_values: more than four operations")
                order[e, b, :len(ops)] = ops
                for k, name in enumerate(('brightness', 'contrast', 'saturation', 'hue')):
                    factors[e, b, k] = float(d.pop(name, factors[e, b, k]))
                if 'gamma_table' in d:
                    t = np.asarray(d.pop('gamma_table'))
                    if t.shape != (256,) or t.min() < 0 or t.max() > 255:
                        raise ValueError("Augmentation.from_values: a gamma table is 256 bytes")
                    tabs[e, b], on[e, b] = t.astype(np.uint8), True
                    d.pop('gamma', None); d.pop('gain', None)
                elif 'gamma' in d:
                    gam[e, b], gain[e, b] = float(d.pop('gamma')), float(d.pop('gain', 1.0))
                    tabs[e, b], on[e, b] = gamma_table(gam[e, b], gain[e, b]), True
                rects[e][b] = list(d.pop('rects', ()))
                seeds[e, b] = np.uint64(int(d.pop('seed', 0)) & 0xFFFFFFFFFFFFFFFF)
                if d:
                    raise ValueError("Augmentation.from_values: unknown keys %s" % sorted(d))
        return cls(order, factors, on, tabs, np.zeros((B, 2), dtype=np.int64) if crop is None else crop, rects, seeds, gam, gain,
                   device=device)

    @classmethod
    def identity(cls, B, crop=None, eyes=2, device=None):
        """No operation, no gamma, no rectangle: augment_frames then gives prepare_frames(size, crop)'s bits."""
        return cls.from_values([[{} for _ in range(B)] for _ in range(eyes)], crop=crop, device=device)

    # ------------------------------------------------------------------------------------------------------------- the table
    def table_host(self):
        """int32 numpy [eyes,B,ROW_INTS]: what `table` holds"""
        E, B = self.eyes, self.B
        t = np.zeros((E, B, ROW_INTS), dtype=np.int32)
        for e in range(E):
            for b in range(B):
                r = t[e, b]
                r[0] = 1 if self.gamma_on[e, b] else 0
                r[1] = sum(int(o) << (8 * k) for k, o in enumerate(self.order[e, b]))
                for k in range(3):
                    r[2 + k] = _f32_bits(self.factors[e, b, k])
                r[5] = int(self.hue_shift[e, b])
                r[6], r[7] = int(self.crop[b, 0]), int(self.crop[b, 1])
                r[8] = len(self.rects[e][b])
                for k, rc in enumerate(self.rects[e][b]):
                    r[9 + 4 * k:13 + 4 * k] = rc
                s = int(self.seeds[e, b])
                r[25:27] = np.array([s & 0xFFFFFFFF, s >> 32], dtype=np.uint32).view(np.int32)
                r[32:96] = self.gamma_tables[e, b].view('<u4').view(np.int32)
        return t

    def to(self, device):
        self.table = torch.from_numpy(self.table_host()).to(device)
        return self

    def refill(self, other):
        """Take over `other`'s values (same eyes and B) and write them into THIS object's device table (one host-to-device copy on
        the current stream): a captured graph or a recorded plan that read the table replays on the new values."""
        if (other.eyes, other.B) != (self.eyes, self.B):
            raise ValueError("Augmentation.refill: a table for %d eyes x %d images into one for %d x %d" % (other.eyes, other.B, self.eyes, self.B))
        if self.table is None:
            raise RuntimeError("Augmentation.refill: this object has no device table")
        for k in ('order', 'factors', 'gamma_on', 'gamma_tables', 'gamma', 'gain', 'crop', 'rects', 'seeds', 'hue_shift'):
            setattr(self, k, getattr(other, k))
        self.table.copy_(torch.from_numpy(self.table_host()), non_blocking=False)
        return self

    def check(self, source_size, size):
        """Refuse host values that leave the frame / the window (the kernel would clamp / clip them)."""
        (Hs, Ws), (H, W) = source_size, size
        for b in range(self.B):
            ch, cw = (int(v) for v in self.crop[b])
            if not (0 <= ch <= Hs - H and 0 <= cw <= Ws - W):
                raise ValueError("Augmentation: the crop origin %s puts a %s window outside an image of shape %s" % ((ch, cw), (H, W), (Hs, Ws)))
            for e in range(self.eyes):
                for sh, sw, oh, ow in self.rects[e][b]:
                    if not (0 <= sh and sh + oh <= H and 0 <= sw and sw + ow <= W):
                        raise ValueError("Augmentation: the rectangle %s of image %d leaves the %s window" % ((sh, sw, oh, ow), b, (H, W)))


def draw_augmentation(B, source_size, size, *, eyes=2, seed=None, generator=None, p_color=0.5, brightness=(0.4, 2.0), contrast=(0.5, 1.5),
                      saturation=(0.5, 1.5), hue=(-0.1, 0.1), gamma=(0.8, 1.2), gain=(1.0, 1.0), p_occlusion=0.5, patches=(2, 4),
                      patch_w=(50, 250), patch_h=(50, 180), same_lr=False, device=None):
    """Draw the parameters of B training samples on the host -> Augmentation.  The defaults are the reference's numbers
    (base.py:73-90, :137-138, :158-166).  Per image: with probability p_color the four operations in a uniformly random order with
    factors uniform in their ranges plus a gamma table from uniform gamma / gain; the crop origin uniform over the positions that
    keep a `size` window inside `source_size`; with probability p_occlusion patches[0]..patches[1] rectangles on the right eye,
    each int(uniform(patch_w)) x int(uniform(patch_h)) (cut to the window) at a uniform position inside it; a 64-bit noise seed.
      same_lr=False   independent colour draws for the two eyes.  This is what the reference computes in BOTH its modes: with
                      do_same_lr_transform=True the same ColorJitter object is called for each eye and redraws on every call, with
                      False the right eye picks one of two such objects (base.py:109-118); either way left and right differ.
      same_lr=True    one set of colour values for both eyes: what the reference's flag promises by its name.
      p_color         the reference draws do_color_aug ONCE per dataset object with probability 0.5 (base.py:73); per image here --
                      pass 1.0 or 0.0 for a whole run to restate that.
    Reproducible from `seed` (or from one integer taken from `generator`, a numpy Generator), and image i draws the same values
    whatever B is.  The reference's torch / numpy random streams are not reproduced."""
    (Hs, Ws), (H, W) = (int(v) for v in source_size), (int(v) for v in size)
    if B <= 0 or eyes not in (1, 2):
        raise ValueError("draw_augmentation: B %d, eyes %d" % (B, eyes))
    if H <= 0 or W <= 0 or H > Hs or W > Ws:
        raise ValueError("draw_augmentation: an image of shape %s cannot be cropped to %s" % ((Hs, Ws), (H, W)))
    if (seed is None) == (generator is None):
        raise ValueError("draw_augmentation: give seed or generator (one of them)")
    if not 1 <= int(patches[0]) <= int(patches[1]) <= MAX_RECTS:
        raise ValueError("draw_augmentation: patches %s (at most %d rectangles)" % (patches, MAX_RECTS))
    seed = int(generator.integers(0, 2 ** 63 - 1)) if seed is None else int(seed)
    ranges = (brightness, contrast, saturation, hue)
    rows = [[None] * B for _ in range(eyes)]
    crop = np.zeros((B, 2), dtype=np.int64)
    for i in range(B):
        rng = np.random.default_rng([seed & 0xFFFFFFFFFFFFFFFF, i])          # one stream per image: prefix-stable in B
        do_color = rng.random() < p_color
        per_eye = []
        for e in range(2):                                                   # always two eyes' worth: the stream does not depend on `eyes`
            perm = [int(v) for v in rng.permutation(4)]
            f = [float(rng.uniform(lo, hi)) for lo, hi in ranges]
            g, gn = float(rng.uniform(*gamma)), float(rng.uniform(*gain))
            per_eye.append((perm, f, g, gn))
        if same_lr:
            per_eye[1] = per_eye[0]
        crop[i] = (int(rng.integers(0, Hs - H + 1)), int(rng.integers(0, Ws - W + 1)))
        occl = rng.random() < p_occlusion
        num = int(rng.integers(int(patches[0]), int(patches[1]) + 1))
        rects = []
        for _ in range(MAX_RECTS):
            occw, occh = min(int(rng.uniform(*patch_w)), W), min(int(rng.uniform(*patch_h)), H)
            sw, sh = int(rng.uniform(0, W - occw)), int(rng.uniform(0, H - occh))
            rects.append((sh, sw, max(occh, 1), max(occw, 1)))
        seeds = [int(v) for v in rng.integers(0, 2 ** 64, size=2, dtype=np.uint64)]
        for e in range(eyes):
            perm, f, g, gn = per_eye[e]
            d = {'seed': seeds[e]}
            if do_color:
                d.update(order=perm, brightness=f[0], contrast=f[1], saturation=f[2], hue=f[3], gamma=g, gain=gn)
            if e == 1 and occl:
                d['rects'] = rects[:num]
            rows[e][i] = d
    return Augmentation.from_values(rows, crop=crop, device=device)


def _table_for(what, aug, B, eyes, dev, source_size, size):
    if not isinstance(aug, Augmentation):
        raise TypeError("%s: aug must be an Augmentation (got %s)" % (what, type(aug).__name__))
    if aug.B != B or aug.eyes < eyes:
        raise ValueError("%s: an Augmentation for %d eye(s) x %d image(s), the frames are %d x %d" % (what, aug.eyes, aug.B, eyes, B))
    if aug.table is None:
        if _lib.recording() or torch.cuda.is_current_stream_capturing():
            raise RuntimeError("%s: the Augmentation has no device table (build it with device=, outside the capture)" % what)
        aug.to(dev)
    _on_gpu(what, aug.table)
    if aug.table.device != dev or aug.table.dtype != torch.int32 or tuple(aug.table.shape) != (aug.eyes, aug.B, ROW_INTS) or \
            not aug.table.is_contiguous():
        raise ValueError("%s: the device table must be a contiguous int32 [%d,%d,%d] on %s" % (what, aug.eyes, aug.B, ROW_INTS, dev))
    aug.check(source_size, size)
    return aug.table


def augment_frames(left, right, aug, size, *, mean=IMAGENET_MEAN, std=IMAGENET_STD, layout='HWC', color=True, out=None):
    """Colour operations + gamma on the full frames, ToTensor, normalize, the crop window and the occlusion rectangles of both eyes
    in two launches (statistics for contrast, then the window).  left / right (may be None): uint8 GPU tensors as prepare_frames
    takes them; aug: an Augmentation for this B (and for two eyes when `right` is given); size = (H, W), the window.
    Returns {'color_l', 'color_aug_l'} and, with `right`, {'color_r', 'color_aug_r'}, fp32 [B,3,H,W] ([3,H,W] for an unbatched
    input): color = the plain / 255 window of the frame as it came, color_aug = the augmented, normalised window.  `color=False`
    leaves the plain images out; out= as prepare_frames (dense images, a free batch stride shared by both eyes)."""
    what = "augment_frames"
    left, right, B, Hs, Ws, batched = _frames(what, left, right, layout)
    dev = left.device
    mean, std = _three("mean", mean), _three("std", std)
    if size is None:
        raise ValueError("%s: the window's size is needed" % what)
    H, W = (int(v) for v in size)
    if H <= 0 or W <= 0:
        raise ValueError("%s: size %s" % (what, (H, W)))
    if H > Hs or W > Ws:
        raise ValueError("%s: an image of shape %s cannot be cropped to %s" % (what, (Hs, Ws), (H, W)))
    sides = ('l', 'r') if right is not None else ('l',)
    table = _table_for(what, aug, B, len(sides), dev, (Hs, Ws), (H, W))
    res, aug_stride = _color_outputs(what, sides, B, H, W, (H, W), out, color, dev)
    L = _lib.lib()
    nbytes = int(L.ts_frames_augment_workspace_bytes(B, Hs, Ws))
    work = torch.empty((nbytes // 8,), device=dev, dtype=torch.int64)
    _lib.check(L.ts_frames_augment_fwd(
        _lib.ptr(left), _lib.ptr(right), B, Hs, Ws, CHW if layout == 'CHW' else 0, *mean, *std, H, W, _lib.ptr(table),
        _lib.ptr(res.get('color_l')), _lib.ptr(res.get('color_r')), 3 * H * W,
        _lib.ptr(res['color_aug_l']), _lib.ptr(res.get('color_aug_r')), aug_stride, _lib.ptr(work), nbytes, _stream()), "ts_frames_augment_fwd")
    if not batched:
        res = {k: v[0] for k, v in res.items()}
    return res


def disp_window_from_uint16(raw, aug, size, scale=256.0, with_valid=False):
    """disp_from_uint16 of the window [ch:ch+H, cw:cw+W] whose origin is read from aug's device table: a 16-bit map [B,Hs,Ws] /
    [B,1,Hs,Ws] ([Hs,Ws] for B = 1) -> fp32 [B,1,H,W]; with_valid also the mask raw > 0 (bool).  raw: uint16 / int16
    (reinterpreted) / int32 (low 16 bits; a cast on the device, not while a launch plan is recorded), as disp_from_uint16."""
    what = "disp_window_from_uint16"
    r, (B, Hs, Ws, _) = _u16_map(what, raw, scale)
    H, W = (int(v) for v in size)
    if H <= 0 or W <= 0 or H > Hs or W > Ws:
        raise ValueError("%s: a map of shape %s cannot be cropped to %s" % (what, (Hs, Ws), (H, W)))
    table = _table_for(what, aug, B, 1, r.device, (Hs, Ws), (H, W))
    disp = torch.empty((B, 1, H, W), device=r.device, dtype=torch.float32)
    valid = torch.empty((B, 1, H, W), device=r.device, dtype=torch.uint8) if with_valid else None
    _lib.check(_lib.lib().ts_disp_u16_window_fwd(_lib.ptr(r), B, Hs, Ws, H, W, _lib.ptr(table), float(scale), _lib.ptr(disp),
                                                 _lib.ptr(valid), _stream()), "ts_disp_u16_window_fwd")
    return (disp, valid.view(torch.bool)) if with_valid else disp


def prepare_train_batch(left, right, K_norm, baseline, size, aug, *, timestamp=0, disp_gt_raw=None, k_size=None, num_scales=None,
                        mean=IMAGENET_MEAN, std=IMAGENET_STD, layout='HWC', gt_scale=256.0, out=None):
    """The training form of prepare_batch's dictionary with the reference's augmentation (base.py do_transform, is_train=True), in
    four launches (frames 2, intrinsics 1, ground truth 1) and without touching the host:
      ('color', t, 'l' / 'r')       [B,3,H,W]     the plain / 255 window
      ('color_aug', t, 'l' / 'r')   [B,3,H,W]     augment_frames(left, right, aug, size)
      ('K', s), ('inv_K', s)        [B,4,4]       the pyramid at k_size -- default: the SOURCE size, the un-cropped resolution
                                                  training uses (base.py:235-236)
      'baseline'                    [B,1,1,1]
      ('disp_gt', t, 'l')           [B,1,H,W]     the SAME window of disp_from_uint16(disp_gt_raw, gt_scale) (base.py:152-155), cut
                                                  inside the decode from the origin in aug's device table
    Usable inside torch.cuda.graph capture and while a launch plan is recorded; replay on new draws after aug.refill(new)."""
    what = "prepare_train_batch"
    if right is None:
        raise ValueError("%s: a stereo pair is needed" % what)
    if size is None:
        raise ValueError("%s: the window's size is needed" % what)
    size = tuple(int(v) for v in size)
    fr = augment_frames(left, right, aug, size, mean=mean, std=std, layout=layout, color=True, out=out)
    if k_size is None:
        k_size = (left.shape[-3], left.shape[-2]) if layout == 'HWC' else (left.shape[-2], left.shape[-1])
    S = default_num_scales(size) if num_scales is None else int(num_scales)
    batch = _batch_dict(what, fr, K_norm, k_size, S, baseline, timestamp)
    if disp_gt_raw is not None:
        batch[('disp_gt', timestamp, 'l')] = disp_window_from_uint16(_gt_rows(what, disp_gt_raw, batch), aug, size, gt_scale)
    return batch
