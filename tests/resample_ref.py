"""The definition of the device resampler (csrc/resample.hip) in numpy and ``math``: Pillow's ``Image.resize(size, resample,
box)`` for 8-bit images, restated in integers, and its 16-bit extension.

Per axis, for a source length n, a source interval [in0, in1) and an output length m, a filter f of support s:
  scale = (in1 - in0) / m, fs = max(scale, 1), support = s * fs, ksize = 2 * ceil(support) + 1                      (double)
  output j: center = in0 + (j + 0.5) * scale, xmin = max(0, (int)(center - support + 0.5)),
            xmax = min(n, (int)(center + support + 0.5)) - xmin
  w_x = f((x + xmin - center + 0.5) / fs) for x < xmax, each divided by their sequential sum when that is non-zero
  k_x = (int)(w_x * 2^22 +- 0.5) (the sign of w_x), zero from xmax to ksize
  out_j = clamp((2^21 + sum_x in[xmin + x] * k_x) >> 22, 0, top)                                   (an arithmetic shift)
The horizontal pass runs first and is rounded to the sample type (top = 255 or 65535), the vertical pass runs on its result; an axis with
m == n, in0 == 0 and in1 == n is copied.  ``math.sin`` / ``math.cos`` (libm), never numpy's: the tables are compared integer for integer.
"""
import math

import numpy as np

BITS = 22
MAX_TAPS = 64
FILTER_IDS = {"box": 0, "bilinear": 1, "hamming": 2, "bicubic": 3, "lanczos": 4}


def _box(x):
    return 1.0 if -0.5 < x <= 0.5 else 0.0


def _bilinear(x):
    x = abs(x)
    return 1.0 - x if x < 1.0 else 0.0


# (Pillow writes the two Hamming constants as C float literals: 0.54f, 0.46f)
_H54, _H46 = float(np.float32(0.54)), float(np.float32(0.46))


def _hamming(x):
    x = abs(x)
    if x == 0.0:
        return 1.0
    if x >= 1.0:
        return 0.0
    x = x * math.pi
    return math.sin(x) / x * (_H54 + _H46 * math.cos(x))


def _bicubic(x, a=-0.5):
    x = abs(x)
    if x < 1.0:
        return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
    if x < 2.0:
        return (((x - 5) * x + 8) * x - 4) * a
    return 0.0


def _sinc(x):
    if x == 0.0:
        return 1.0
    x = x * math.pi
    return math.sin(x) / x


def _lanczos(x):
    return _sinc(x) * _sinc(x / 3) if -3.0 <= x < 3.0 else 0.0


FILTERS = {"box": (_box, 0.5), "bilinear": (_bilinear, 1.0), "hamming": (_hamming, 1.0), "bicubic": (_bicubic, 2.0), "lanczos": (_lanczos, 3.0)}


def ksize_of(in0, in1, m, filt):
    scale = (in1 - in0) / m
    return 2 * int(math.ceil(FILTERS[filt][1] * max(scale, 1.0))) + 1


def coeffs(n, in0, in1, m, filt, normalise=True, nearest=False):
    """(k int32 [m, ksize], bounds int32 [m, 2]) of one axis.  ``normalise=False`` / ``nearest=True``: the two deliberately wrong variants
    of test_resample_host.py (weights left unnormalised; ``round`` — to nearest, ties to even — wherever the definition adds 0.5 and
    truncates: the window's two ends and w * 2^22.  The two differ at ties only, which a box filter at scale 1.5 makes visible)."""
    f, s = FILTERS[filt]
    scale = (in1 - in0) / m
    fs = max(scale, 1.0)
    support = s * fs
    ksize = 2 * int(math.ceil(support)) + 1
    k = np.zeros((m, ksize), np.int32)
    bounds = np.zeros((m, 2), np.int32)
    for j in range(m):
        center = in0 + (j + 0.5) * scale
        if nearest:
            xmin, xmax = max(0, round(center - support)), min(n, round(center + support))
        else:
            xmin, xmax = max(0, int(center - support + 0.5)), min(n, int(center + support + 0.5))
        xmax -= xmin
        w = [f((x + xmin - center + 0.5) / fs) for x in range(xmax)]
        total = 0.0
        for v in w:
            total += v
        if normalise and total != 0.0:
            w = [v / total for v in w]
        for x, v in enumerate(w):
            k[j, x] = round(v * (1 << BITS)) if nearest else int(v * (1 << BITS) + (0.5 if v >= 0 else -0.5))
        bounds[j] = xmin, xmax
    return k, bounds


def apply_axis(a, k, bounds, axis, top, rounded=True):
    """One pass along ``axis`` of the integer array ``a``: int64 sums, then (``rounded``) the shift and the clamp to 0 .. top."""
    a = np.moveaxis(np.asarray(a).astype(np.int64), axis, 0)
    n = a.shape[0]
    m, ksize = k.shape
    idx = np.minimum(bounds[:, :1].astype(np.int64) + np.arange(ksize)[None], n - 1)  # (weights past xmax are zero)
    out = np.zeros((m,) + a.shape[1:], np.int64)
    for x in range(ksize):
        out += a[idx[:, x]] * k[:, x].astype(np.int64).reshape((m,) + (1,) * (a.ndim - 1))
    if rounded:
        out = np.clip((out + (1 << (BITS - 1))) >> BITS, 0, top)
    return np.moveaxis(out, 0, axis)


def axis_is_identity(n, in0, in1, m):
    return m == n and in0 == 0 and in1 == n


def resize(img, size, filt, box=None, variant=None):
    """``img`` uint8 / uint16 [..., H, W, C] -> [..., h, w, C] for ``size = (w, h)`` and the integer source box (x0, y0, x1, y1) (default:
    the whole image).  ``variant``: None (the definition) or one of the four deliberately wrong twins — "vertical_first",
    "no_intermediate" (the horizontal sums are not rounded before the vertical pass), "nearest", "unnormalised"."""
    img = np.asarray(img)
    top = 255 if img.dtype == np.uint8 else 65535
    h_in, w_in = img.shape[-3], img.shape[-2]
    w, h = size
    x0, y0, x1, y1 = box if box is not None else (0, 0, w_in, h_in)
    kw = dict(normalise=variant != "unnormalised", nearest=variant == "nearest")
    passes = []
    if not axis_is_identity(w_in, x0, x1, w):
        passes.append((-2,) + coeffs(w_in, x0, x1, w, filt, **kw))
    if not axis_is_identity(h_in, y0, y1, h):
        passes.append((-3,) + coeffs(h_in, y0, y1, h, filt, **kw))
    if variant == "vertical_first":
        passes.reverse()
    out = img.astype(np.int64)
    if variant == "no_intermediate" and len(passes) == 2:
        out = apply_axis(out, passes[0][1], passes[0][2], passes[0][0], top, rounded=False)
        out = apply_axis(out, passes[1][1], passes[1][2], passes[1][0], top, rounded=False)
        out = np.clip((out + (1 << (2 * BITS - 1))) >> (2 * BITS), 0, top)
    else:
        for axis, k, bounds in passes:
            out = apply_axis(out, k, bounds, axis, top)
    return out.astype(img.dtype)


def resize_into(canvas, img, window, filt, box=None):
    """The entry's windowed form: ``img`` resized to the window (x, y, w, h) of a copy of ``canvas`` [..., H, W, C], the rest untouched."""
    x, y, w, h = window
    out = np.array(canvas, copy=True)
    out[..., y:y + h, x:x + w, :] = resize(img, (w, h), filt, box)
    return out


# ---------------------------------------------------------------------------------------------------------------- render.FrameResize in integers
def fit_geometry(W, H, w, h, fit):
    """(source box (x0, y0, x1, y1), window (x, y, w, h)) of render.FrameResize for a W x H source and a w x h target."""
    if fit == "stretch":
        return (0, 0, W, H), (0, 0, w, h)
    if fit == "crop":
        if W * h > H * w:
            cw, ch = min(max((H * w + h // 2) // h, 1), W), H
        else:
            cw, ch = W, min(max((W * h + w // 2) // w, 1), H)
        x0, y0 = (W - cw) // 2, (H - ch) // 2
        return (x0, y0, x0 + cw, y0 + ch), (0, 0, w, h)
    if fit == "pad":
        if W * h > H * w:  # the source is wider than the target: full width, bars above and below
            dw, dh = w, (H * w + W // 2) // W
        else:
            dw, dh = (W * h + H // 2) // H, h
        dw, dh = max(min(dw, w) & ~1, 2), max(min(dh, h) & ~1, 2)
        return (0, 0, W, H), (((w - dw) // 2) & ~1, ((h - dh) // 2) & ~1, dw, dh)
    raise ValueError(fit)


def deliver(frames, size, filt="lanczos", fit="crop"):
    """render.resize_frames in numpy: [b, H, W, 3] -> [b, h, w, 3], the border of a padded frame 0."""
    frames = np.asarray(frames)
    w, h = size
    box, window = fit_geometry(frames.shape[2], frames.shape[1], w, h, fit)
    canvas = np.zeros(frames.shape[:1] + (h, w, 3), frames.dtype)
    return resize_into(canvas, frames, window, filt, box)
