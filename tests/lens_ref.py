"""The lens effects of csrc/lens.hip (include/maua_hip.h states them) restated in numpy: ``dtype=np.float64`` is the definition,
``dtype=np.float32`` the all-float32 emulation in the header's order (every operation rounded on its own).  For the blur the header fixes
no order: the emulation takes the centre first, then k = 1 .. R with the pair summed before it is weighted, unfused.

Also the plan rule of audioreactive/lens.py, the deliberately wrong variants the host tests tell apart, the operands of
the GPU case lists and the allowances the GPU tests hold the device to (never computed from the device's own output)."""
import math

import numpy as np

ROW = 16
THRESHOLD, KNEE, BLOOM, SHARPEN, VIGNETTE, INNER, OUTER = 0, 1, 2, 5, 6, 7, 8
RMAX, TILE = 64, 64
REDUCTIONS = (1, 2, 4, 8)
SIGMA_PER_D, SHARPEN_SIGMA_MAX = 6.0, 8.0
F32, F64 = np.float32, np.float64


def make_row(threshold=0.7, knee=0.1, bloom_rgb=(0, 0, 0), sharpen=0, vignette=0, inner=0.5, outer=1.0):
    row = np.zeros(ROW, F32)
    row[THRESHOLD], row[KNEE], row[BLOOM:BLOOM + 3], row[SHARPEN], row[VIGNETTE], row[INNER], row[OUTER] = threshold, knee, bloom_rgb, sharpen, vignette, inner, outer
    return row


def is_identity(rows):
    rows = np.atleast_2d(rows)
    return (rows[:, BLOOM:BLOOM + 3] == 0).all(axis=1) & (rows[:, SHARPEN] == 0) & (rows[:, VIGNETTE] == 0)


# ------------------------------------------------------------------------------------------------ the plan rule
def plan_reduction(sigma_max):
    """The smallest d of 1, 2, 4, 8 with sigma_max / d <= 6, else 8."""
    for d in REDUCTIONS:
        if sigma_max / d <= SIGMA_PER_D:
            return d
    return REDUCTIONS[-1]


def plan_radius(sigma_max, d=1):
    return int(math.ceil(3.0 * sigma_max / d))


def gaussian_taps(sigmas, radius):
    """float32 [n, radius + 1]: exp(-k^2 / (2 sigma^2)) in float64, normalised to w[0] + 2 sum w[k] = 1; sigma 0 is the delta."""
    sigmas = np.atleast_1d(np.asarray(sigmas, F64))
    k = np.arange(radius + 1, dtype=F64)
    out = np.zeros((len(sigmas), radius + 1), F64)
    for i, s in enumerate(sigmas):
        if s == 0:
            out[i, 0] = 1.0
            continue
        g = np.exp(-k * k / (2.0 * s * s))
        out[i] = g / (g[0] + 2.0 * g[1:].sum())
    return out.astype(F32)


def plan(bloom_size, h, sharpen_sigma):
    """(d, bloom radius, bloom taps, sharpen radius, sharpen taps) of per-frame bloom sizes (fractions of h) and sharpen sigmas (px)."""
    sig = np.atleast_1d(np.asarray(bloom_size, F64)) * h
    d = plan_reduction(sig.max())
    rb = plan_radius(sig.max(), d)
    if rb > RMAX:
        raise ValueError(f"bloom radius {rb} > {RMAX}")
    ss = np.atleast_1d(np.asarray(sharpen_sigma, F64))
    if ss.max() > SHARPEN_SIGMA_MAX:
        raise ValueError(f"sharpen sigma {ss.max()} > {SHARPEN_SIGMA_MAX}")
    rs = plan_radius(ss.max())
    return d, rb, gaussian_taps(sig / d, rb), rs, gaussian_taps(ss, rs)


# ------------------------------------------------------------------------------------------------ the definition
def clamp01(a):
    return np.where(np.isnan(a), a.dtype.type(0), np.minimum(np.maximum(a, a.dtype.type(0)), a.dtype.type(1)))


def highlight(x, rows, dtype=F64, knee=True):
    """[B,3,H,W] -> hl [B,3,H,W].  ``knee=False``: the wrong variant that ignores the knee (a hard threshold)."""
    T = dtype
    x = np.asarray(x).astype(T)
    rows = np.asarray(rows)
    th = rows[:, THRESHOLD].astype(T)[:, None, None]
    kn = (rows[:, KNEE].astype(T) if knee else np.zeros(len(rows), T))[:, None, None]
    with np.errstate(invalid="ignore"):  # (a signalling NaN)
        v = clamp01(x * T(0.5) + T(0.5))
    m = np.maximum(np.maximum(v[:, 0], v[:, 1]), v[:, 2])
    o = m - th
    s = np.minimum(np.maximum(o + kn, T(0)), T(2) * kn)
    s = (s * s) / (T(4) * kn + T(1e-5))
    q = np.maximum(s, o) / np.maximum(m, T(1e-5))
    return (v * q[:, None]).astype(T)


def box_reduce(hl, d, dtype=F64):
    """Mean over the existing pixels of every d x d block: summed from 0 row by row, left to right, divided by the count."""
    T = dtype
    b, c, h, w = hl.shape
    oh, ow = -(-h // d), -(-w // d)
    pad = np.zeros((b, c, oh * d, ow * d), T)
    pad[:, :, :h, :w] = hl
    acc = np.zeros((b, c, oh, ow), T)
    for r in range(d):
        for q in range(d):
            acc = (acc + pad[:, :, r::d, q::d]).astype(T)  # (absent pixels add 0.0, which changes nothing: every term is >= +0)
    ch = np.minimum(d, h - d * np.arange(oh))[:, None]
    cw = np.minimum(d, w - d * np.arange(ow))[None, :]
    return (acc / (ch * cw).astype(T)).astype(T)


def extract(x, rows, d, dtype=F64, knee=True):
    return box_reduce(highlight(x, rows, dtype, knee), d, dtype)


def _blur_axis(x, taps, axis, T, edge):
    n = x.shape[axis]
    radius = taps.shape[1] - 1
    i = np.arange(n)
    shape = [len(taps)] + [1] * (x.ndim - 1)

    def take(idx):
        got = np.take(x, np.clip(idx, 0, n - 1), axis=axis)
        if edge == "zero":
            mask_shape = [1] * x.ndim
            mask_shape[axis] = n
            got = got * ((idx >= 0) & (idx < n)).reshape(mask_shape).astype(T)
        return got

    acc = (taps[:, 0].reshape(shape) * x).astype(T)
    for k in range(1, radius + 1):
        acc = (acc + taps[:, k].reshape(shape) * (take(i - k) + take(i + k))).astype(T)
    return acc


def blur(x, taps, dtype=F64, edge="replicate"):
    """[B,P,H,W] with per-frame half-kernels [B, R + 1]: along rows, then along columns.  ``edge="zero"``: the wrong variant."""
    T = dtype
    x, taps = np.asarray(x).astype(T), np.asarray(taps).astype(T)
    return _blur_axis(_blur_axis(x, taps, 3, T, edge), taps, 2, T, edge)


def upsample(bloom, h, w, d, dtype=F64, half_pixel=True):
    """The bilinear sample of the reduced map [B,3,bh,bw] at every pixel of h x w.  ``half_pixel=False``: the wrong variant u = px / d."""
    T = dtype
    bloom = np.asarray(bloom).astype(T)
    bh, bw = bloom.shape[2:]

    def axis(n, size):
        p = np.arange(n).astype(T)
        u = (p + T(0.5)) / T(d) - T(0.5) if half_pixel else p / T(d)
        u = np.minimum(np.maximum(u, T(0)), T(size - 1))
        i0 = u.astype(np.int64)
        return i0, np.minimum(i0 + 1, size - 1), (u - i0.astype(T)).astype(T)

    y0, y1, fy = axis(h, bh)
    x0, x1, fx = axis(w, bw)
    fy, fx = fy[:, None], fx[None, :]
    w00, w01, w10, w11 = (T(1) - fx) * (T(1) - fy), fx * (T(1) - fy), (T(1) - fx) * fy, fx * fy
    g = lambda yi, xi: bloom[:, :, yi][:, :, :, xi]
    return (((w00 * g(y0, x0) + w01 * g(y0, x1)) + w10 * g(y1, x0)) + w11 * g(y1, x1)).astype(T)


def vignette_factor(h, w, strength, inner, outer, dtype=F64):
    T = dtype
    dx = ((np.arange(w).astype(T) + T(0.5)) - T(w) * T(0.5)) / (T(w) * T(0.5))
    dy = ((np.arange(h).astype(T) + T(0.5)) - T(h) * T(0.5)) / (T(h) * T(0.5))
    inv = T(0.70710678118654752)
    r = np.sqrt(dx[None, :] * dx[None, :] + dy[:, None] * dy[:, None]) * inv
    t = clamp01(((r - T(inner)) / (T(outer) - T(inner))).astype(T))
    return (T(1) - T(strength) * ((t * t) * (T(3) - T(2) * t))).astype(T)


def apply(x, rows, bloom=None, d=1, soft=None, dtype=F64, half_pixel=True, bloom_factor=2):
    """The apply entry.  ``bloom_factor=1``: the wrong variant that forgets the display-range factor."""
    T = dtype
    x = np.asarray(x)
    rows = np.asarray(rows, F32)
    b, _, h, w = x.shape
    out = np.empty(x.shape, T)
    ident = is_identity(rows)
    up = None if bloom is None else upsample(bloom, h, w, d, T, half_pixel)
    for i in range(b):
        with np.errstate(invalid="ignore"):  # (a signalling NaN in an identity frame)
            xi = x[i].astype(T)
        if ident[i]:
            out[i] = xi  # (float32: the input's bits; the caller compares bits)
            continue
        y = xi
        if soft is not None:
            y = y + T(rows[i, SHARPEN]) * (xi - np.asarray(soft[i]).astype(T))
        if up is not None:
            gain = (T(bloom_factor) * rows[i, BLOOM:BLOOM + 3].astype(T))[:, None, None]
            y = y + gain * up[i]
        if rows[i, VIGNETTE] != 0:
            f = vignette_factor(h, w, rows[i, VIGNETTE], rows[i, INNER], rows[i, OUTER], T)
            y = (y + T(1)) * f - T(1)
        out[i] = y
    if T is F32 and x.dtype == F32:
        out.view(np.uint32)[ident] = x.view(np.uint32)[ident]  # NaN payloads included
    return out


def lens(x, rows, d, bloom_taps, sharpen_taps, dtype=F64, **wrong):
    """The whole chain as render.lens_frames launches it: extract -> blur -> (blur of the image) -> apply.  ``wrong``: edge, half_pixel,
    knee, bloom_factor."""
    edge = wrong.get("edge", "replicate")
    bl = soft = None
    if bloom_taps is not None:
        bl = blur(extract(x, rows, d, dtype, wrong.get("knee", True)), bloom_taps, dtype, edge)
    if sharpen_taps is not None:
        soft = blur(np.asarray(x).astype(dtype), sharpen_taps, dtype, edge)
    return apply(x, rows, bl, d, soft, dtype, wrong.get("half_pixel", True), wrong.get("bloom_factor", 2))


# ------------------------------------------------------------------------------------------------ allowances
def blur_ceiling(radius, peak):
    """Two passes of radius + 3 rounded operations on weights that sum to 1."""
    return 2.0 * (radius + 4) * 2.0 ** -23 * peak


def blur_allowance(x, taps):
    """(allowed, the emulation's own error, the ceiling) per element of a blur case: max(4 x the float32 emulation's error against float64,
    4 * 2^-24 max|x|)."""
    peak = float(np.max(np.abs(x)))
    own = float(np.max(np.abs(blur(x, taps, F32).astype(F64) - blur(x, taps, F64))))
    return max(4.0 * own, 4.0 * 2.0 ** -24 * peak), own, blur_ceiling(taps.shape[1] - 1, peak)


def apply_allowance(x, rows, bloom, d, soft):
    """(allowed, own): 4 x the float32 emulation's own error against float64 on this case (for frames with a vignette)."""
    own = float(np.max(np.abs(apply(x, rows, bloom, d, soft, F32).astype(F64) - apply(x, rows, bloom, d, soft, F64))))
    return 4.0 * own, own


def chain_allowance(x, rows, d, bloom_taps, sharpen_taps):
    """(allowed, own) per element of the whole chain against float64.  The chain is linear behind the two blurs: an error e_soft of the soft
    image reaches the result as |sharpen| e_soft, an error e_bloom of the blurred map as at most 2 max(bloom_rgb) e_bloom (the bilinear
    weights sum to 1), and the vignette's factor is at most 1 for strengths in [0, 1].  So: the two blurs' own allowances (blur_allowance on
    the emulation's inputs) scaled by those gains, plus 4 x the float32 emulation's own error on the whole chain, which covers extract and
    apply (bit for bit the emulation's on the device, up to the vignette's sqrt and divisions)."""
    own = float(np.max(np.abs(lens(x, rows, d, bloom_taps, sharpen_taps, F32).astype(F64) - lens(x, rows, d, bloom_taps, sharpen_taps, F64))))
    allowed = 4.0 * own
    if bloom_taps is not None:
        allowed += 2.0 * float(np.abs(rows[:, BLOOM:BLOOM + 3]).max()) * blur_allowance(extract(x, rows, d, F32), bloom_taps)[0]
    if sharpen_taps is not None:
        allowed += float(np.abs(rows[:, SHARPEN]).max()) * blur_allowance(x, sharpen_taps)[0]
    return allowed, own


# ------------------------------------------------------------------------------------------------ operands of the GPU case lists
BLUR_PLANES = ((1, 1), (3, 5), (17, 33), (TILE - 1, TILE + 1), (TILE, TILE), (TILE + 1, TILE - 1))


def blur_cases():
    """Every plane x radius 0, 1, the plane's width (every tap clamped; at most 64) and 64; batch 2 x 2 planes; frame 0 holds the delta,
    frame 1 the wide kernel; odd cases take a tap stride beyond radius + 1.  (h, w) = (64, 64) takes the vector instance, (3, 5) ... the
    scalar one; ``skew`` cases (below) move a vector-sized plane off its alignment."""
    cases = []
    for n, (h, w) in enumerate(BLUR_PLANES):
        for radius in sorted({0, 1, min(w, RMAX), RMAX}):
            cases.append(dict(shape=(2, 2, h, w), radius=radius, stride=radius + 1 + (3 if (n + radius) % 2 else 0), seed=100 * n + radius))
    return cases


def blur_operands(case, kind):
    """(x [B,P,H,W] float32, taps [B, stride] float32 with junk behind the radius).  kind "dyadic": integers in -4 .. 4 and taps 2^-1 ..
    2^-3 — every partial sum of either pass is a multiple of 2^-6 below 2^15: exact in float32 in any order, fused or not; "real":
    uniform [-1, 1] and Gaussians of sigma radius / 3.  Frame 0 always holds the delta."""
    rng = np.random.default_rng(case["seed"])
    b, p, h, w = case["shape"]
    radius = case["radius"]
    taps = np.full((b, case["stride"]), 1e30, F32)
    if kind == "dyadic":
        x = rng.integers(-4, 5, case["shape"]).astype(F32)
        taps[:, :radius + 1] = 2.0 ** -rng.integers(1, 4, (b, radius + 1))
    else:
        x = rng.uniform(-1, 1, case["shape"]).astype(F32)
        taps[:, :radius + 1] = gaussian_taps(np.full(b, radius / 3.0), radius)
    taps[0, :radius + 1] = 0
    taps[0, 0] = 1
    return x, taps


def image(b, h, w, seed, spread=1.3):
    """A test image: smooth colour fields plus noise, beyond [-1, 1] in places (the quantisers clamp later, the lens must cope)."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([np.sin(0.37 * xx + 0.11 * yy + c) * np.cos(0.23 * yy - 0.07 * xx + 2 * c) for c in range(3)])
    return (spread * (0.7 * base[None] + 0.5 * rng.uniform(-1, 1, (b, 3, h, w)))).astype(F32)


def sample_rows(b, seed, vignette=False, identity_every=0):
    rng = np.random.default_rng(seed)
    rows = np.stack([make_row(threshold=rng.uniform(0.3, 0.7), knee=rng.uniform(0.05, 0.2), bloom_rgb=rng.uniform(0.3, 1.0, 3),
                              sharpen=rng.uniform(-0.5, 1.0), vignette=rng.uniform(0.2, 0.8) if vignette else 0,
                              inner=rng.uniform(0.1, 0.5), outer=rng.uniform(0.8, 1.2)) for _ in range(b)])
    if identity_every:
        rows[::identity_every] = make_row()
    return rows
