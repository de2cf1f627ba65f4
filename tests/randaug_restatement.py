"""Plain statements of the RandAugment ops (include/fastvision_amd.h, the torchvision space) in integer / float64 numpy, with the rule by
which the GPU tests compare against them.  ``apply_op(img, op, v, fill)`` returns ``(out, excused, skipped)`` for one uint8 [H, W, 3] image:

  * ``excused``: elements whose float64 value before truncation lies within 2^-10 of an integer inside the clamp range -- the kernel's
    fp32 evaluation (a few roundings of 2^-15 at magnitudes below 512) may truncate to the neighbour there: a difference of 1 is allowed.
    Values that are exact in fp32 by construction are NOT excused: v == 0 (f == 1, the blend is x), and x == d, where the header's form
    d + f (x - d) gives x.
  * ``skipped``: pixels of ShearX / ShearY / Rotate with a source coordinate within 2^-10 of a half-integer: nearest sampling is
    undecided there, the pixel is left out.
Everything else is bit-exact: the integer ops, AutoContrast (an integer division: x 255 over hi - lo truncates alike in any arithmetic that
rounds the quotient correctly), the translations, and grey(), which IS the fp32 sequence of the header, not an approximation of one."""
import numpy as np

OPS = ('Identity', 'ShearX', 'ShearY', 'TranslateX', 'TranslateY', 'Rotate', 'Brightness', 'Color', 'Contrast', 'Sharpness', 'Posterize',
       'Solarize', 'AutoContrast', 'Equalize')
SIGNED = OPS[1:10]
EPS = 2.0 ** -10
F32 = np.float32


def grey(img):
    """trunc(0.2989f r + 0.587f g + 0.114f b), left to right in fp32"""
    r, g, b = (img[..., c].astype(F32) for c in range(3))
    return ((F32(0.2989) * r + F32(0.587) * g) + F32(0.114) * b).astype(np.int64)


def _blend(x, d, v):
    """trunc(clamp(f x + (1 - f) d, 0, 255)), f = 1 + v, in float64 in the header's form d + f (x - d) -> (bytes, excused)"""
    if v == 0:
        return x.astype(np.uint8), np.zeros(x.shape, bool)
    f = 1.0 + float(v)
    pre = d + f * (x.astype(np.float64) - d)
    near = (np.abs(pre - np.rint(pre)) < EPS) & (pre > -EPS) & (pre < 255 + EPS) & (x != d)
    return np.trunc(np.clip(pre, 0, 255)).astype(np.uint8), near


def smoothed(img):
    """the 3 x 3 sum with weights [[1,1,1],[1,5,1],[1,1,1]] over 13, to nearest (13 is odd: no ties); valid for interior pixels"""
    p = np.pad(img.astype(np.int64), ((1, 1), (1, 1), (0, 0)))
    H, W = img.shape[:2]
    s = sum(p[dy:dy + H, dx:dx + W] for dy in range(3) for dx in range(3)) + 4 * p[1:1 + H, 1:1 + W]
    return (2 * s + 13) // 26


def equalize_table(hist, n):
    """the 256-entry table of one channel from its histogram; None: identity (step 0)"""
    last = hist[np.nonzero(hist)[0][-1]]
    step = (n - last) // 255
    if step == 0:
        return None
    lut = np.minimum(255, (np.cumsum(hist)[:-1] + step // 2) // step)
    return np.concatenate([[0], lut]).astype(np.uint8)


def posterize_mask(bits):
    return 0xFF & ~((1 << (8 - int(bits))) - 1)


def _sources(op, v, H, W):
    """float64 source coordinates (sx, sy) of every output pixel, and the skipped pixels"""
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    cx, cy = (W - 1) / 2, (H - 1) / 2
    dx, dy = x - cx, y - cy
    v = float(v)
    if op == 'TranslateX':
        return x - int(v), y, np.zeros((H, W), bool)
    if op == 'TranslateY':
        return x, y - int(v), np.zeros((H, W), bool)
    if op == 'ShearX':
        sx, sy = x + v * dy, y
    elif op == 'ShearY':
        sx, sy = x, y + v * dx
    else:
        c, s = np.cos(np.deg2rad(v)), np.sin(np.deg2rad(v))
        sx, sy = c * dx - s * dy + cx, s * dx + c * dy + cy
    tie = lambda t: np.abs(t + 0.5 - np.rint(t + 0.5)) < EPS
    return sx, sy, (tie(sx) | tie(sy)) if v != 0 else np.zeros((H, W), bool)


def apply_op(img, op, v, fill=(0, 0, 0)):
    op = OPS[op] if not isinstance(op, str) else op
    H, W, _ = img.shape
    none = np.zeros(img.shape, bool)
    x = img.astype(np.int64)
    if op == 'Identity':
        return img.copy(), none, none
    if op in ('ShearX', 'ShearY', 'TranslateX', 'TranslateY', 'Rotate'):
        sx, sy, skip = _sources(op, v, H, W)
        ix, iy = np.floor(sx + 0.5).astype(np.int64), np.floor(sy + 0.5).astype(np.int64)
        inside = (ix >= 0) & (ix < W) & (iy >= 0) & (iy < H)
        out = np.empty_like(img)
        out[:] = np.asarray(fill, np.uint8)
        out[inside] = img[iy[inside], ix[inside]]
        return out, none, np.repeat(skip[..., None], 3, 2)
    if op == 'Brightness':
        out, near = _blend(x, 0.0, v)
    elif op == 'Color':
        out, near = _blend(x, grey(img)[..., None].astype(np.float64), v)
    elif op == 'Contrast':
        out, near = _blend(x, grey(img).astype(np.float64).mean(), v)
    elif op == 'Sharpness':
        out, near = _blend(x, smoothed(img).astype(np.float64), v)
        border = np.ones((H, W), bool)
        border[1:-1, 1:-1] = False
        out[border], near[border] = img[border], False
    elif op == 'Posterize':
        return (x & posterize_mask(v)).astype(np.uint8), none, none
    elif op == 'Solarize':
        return np.where(x >= float(v), 255 - x, x).astype(np.uint8), none, none
    elif op == 'AutoContrast':
        out = img.copy()
        for c in range(3):
            lo, hi = int(img[..., c].min()), int(img[..., c].max())
            if hi > lo:
                out[..., c] = np.clip((x[..., c] - lo) * 255 // (hi - lo), 0, 255)
        return out, none, none
    elif op == 'Equalize':
        out = img.copy()
        for c in range(3):
            lut = equalize_table(np.bincount(img[..., c].ravel(), minlength=256), H * W)
            if lut is not None:
                out[..., c] = lut[img[..., c]]
        return out, none, none
    return out, near, none


def apply_plan(batch, ops, values, fill=(0, 0, 0)):
    """the rounds chained, image by image: ops / values [B][N].  An undecided element of an earlier round would make everything downstream
    of it undecided (a histogram, a neighbourhood), so only the LAST round may have any: the marks returned are its own."""
    outs, exc, skp = [], [], []
    for img, row_ops, row_vals in zip(batch, ops, values):
        for i, (op, v) in enumerate(zip(row_ops, row_vals)):
            img, e, s = apply_op(img, op, v, fill)
            assert i == len(row_ops) - 1 or not (e.any() or s.any()), f'round {i} ({op}, {v}) leaves undecided elements'
        outs.append(img), exc.append(e), skp.append(s)
    return np.stack(outs), np.stack(exc), np.stack(skp)


def compare(got, want, excused, skipped):
    """-> (ok, share): ok iff every element that is not skipped matches exactly, or within 1 where excused; share of excused or skipped"""
    diff = np.abs(got.astype(np.int64) - want.astype(np.int64))
    bad = ~skipped & (diff > np.where(excused, 1, 0))
    return not bad.any(), float((excused | skipped).mean())


def canvases(B, H, W, seed):
    """image 0: full-range noise; image 1: a constant channel (AutoContrast identity, Equalize step 0), a two-level channel and noise;
    image 2 and on: a smooth ramp with noise in a narrow range, the channels apart (AutoContrast, Sharpness and Color have something to do)"""
    rng = np.random.default_rng(seed)
    out = rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)
    if B > 1:
        out[1, ..., 0] = 77
        out[1, ..., 1] = np.where(rng.random((H, W)) < 0.4, 41, 203)
    for b in range(2, B):
        ramp = np.add.outer(np.arange(H) * 70 // H, np.arange(W) * 50 // W)[..., None]
        out[b] = (37 + ramp + rng.integers(0, 23, (H, W, 3)) + np.array([0, 60, 10])).astype(np.uint8)
    return out
