"""The frame feedback of csrc/feedback.hip (include/maua_hip.h states it) restated in numpy: ``dtype=np.float64`` is the definition,
``dtype=np.float32`` the all-float32 emulation in the header's order.

How the order is fixed.  The definition has NO fused multiply-add: every product, sum and difference below is rounded on its own, in the
order the parentheses give.  numpy rounds every float32 operation on its own, so the emulation is that by construction; the kernel file
switches the compiler's contraction of a * b + c off for every function in it (``#pragma clang fp contract(off)``) and writes each
operation as its own expression — the toolchain's __fmul_rn / __fadd_rn are plain operators that fuse after inlining, which is why they are
not what pins it.  floorf, fminf, fmaxf and the float -> int conversion of an integral value are exact on both sides.  So the device is
expected to equal the emulation in every bit wherever no NaN is involved; the GPU tests demand that on dyadic operands and hold real
operands to the allowance below.

Continuity.  ``combine``, the bilinear form a + f (b - a) and all four border rules are continuous in the source coordinate: at an
integer coordinate the two taps either side give the same value (f = 0 selects tap i, f -> 1 tends to tap i + 1, which IS the next
interval's tap i), and the border rules act on tap indices — mirror and wrap are periodic in the index, replicate is constant beyond the
edge, zero is the constant -1 there.  A coordinate that rounds to the other side of an integer in float32 therefore moves the result by
|d coordinate| x (the difference of two neighbouring taps), a rounding error, never by a whole tap.  The allowance rests on this.

Also here: the composition of zoom / rotate / translate into the row's inverse matrix (float64), the deliberately wrong variants
(``defect=``) the host tests tell apart, the case list shared by the host and GPU tests, and the allowance (never computed from the
device's output)."""
import functools
import math

import numpy as np

ROW = 16
A, B, TX, C, D, TY, GAIN, TINT, DRY, LIMIT, STILL = 0, 1, 2, 3, 4, 5, 6, 7, 10, 11, 12
MODES = ("add", "max", "screen")
BORDERS = ("zero", "replicate", "mirror", "wrap")
F32, F64 = np.float32, np.float64
COORD_MAX = 2.0 ** 30
EPS = 2.0 ** -24  # half an ulp of 1: the relative error of one float32 rounding
DEFECTS = ("signed decay", "forward matrix", "no recursion", "mirror 2n", "no carry")
IDENTITY = (1, 0, 0, 0, 1, 0)


def make_row(matrix=IDENTITY, gain=0, tint=(1, 1, 1), dry=1, limit=4, still=None):
    """One row.  ``still`` None: set exactly when the float32 matrix is the identity."""
    row = np.zeros(ROW, F32)
    row[A:TY + 1], row[GAIN], row[TINT:TINT + 3], row[DRY], row[LIMIT] = matrix, gain, tint, dry, limit
    row[STILL] = float(is_identity_matrix(row)) if still is None else float(still)
    return row


def is_identity_matrix(row):
    return bool((np.asarray(row[A:TY + 1], F32) == np.asarray(IDENTITY, F32)).all())


def is_neutral(row):
    return bool(row[GAIN] == 0 and row[DRY] == 1)


def inverse_matrix(zoom, rotate_deg, translate, h, w):
    """(a, b, tx, c, d, ty) in float64, in pixels: what an output pixel's offset from the centre is multiplied by to find its source.
    Each recirculation shows the old picture magnified by ``zoom`` about the centre, turned counter-clockwise (as seen on the screen, y
    pointing down) by ``rotate_deg`` and moved by ``translate`` = (fraction of w to the right, fraction of h down):
        d_out = zoom R d_src + t,  R = [[cos, sin], [-sin, cos]]   =>   d_src = (1 / zoom) R^T (d_out - t)."""
    th = math.radians(float(rotate_deg))
    co, si = math.cos(th), math.sin(th)
    ia, ib, ic, id_ = co / zoom, -si / zoom, si / zoom, co / zoom
    px, py = float(translate[0]) * w, float(translate[1]) * h
    return ia, ib, -(ia * px + ib * py), ic, id_, -(ic * px + id_ * py)


# ------------------------------------------------------------------------------------------------ the definition
def clamp01(a):
    return np.where(np.isnan(a), a.dtype.type(0), np.minimum(np.maximum(a, a.dtype.type(0)), a.dtype.type(1)))


def fold_index(i, n, border, defect=None):
    """Integer tap indices -> (index inside 0 .. n - 1, valid).  Invalid (zero border, outside): a black tap."""
    i = np.asarray(i, np.int64)
    valid = np.ones(i.shape, bool)
    if border == "zero":
        valid = (i >= 0) & (i < n)
        return np.clip(i, 0, n - 1), valid
    if border == "replicate":
        return np.clip(i, 0, n - 1), valid
    if border == "wrap":
        return np.mod(i, n), valid
    if border != "mirror":
        raise ValueError(border)
    if defect == "mirror 2n":  # the reflection that repeats the edge element: period 2 n
        m = np.mod(i, 2 * n)
        return np.where(m >= n, 2 * n - 1 - m, m), valid
    if n == 1:
        return np.zeros_like(i), valid
    p = 2 * (n - 1)
    m = np.mod(i, p)
    return np.where(m > n - 1, p - m, m), valid


def coordinates(row, h, w, T, defect=None):
    """(sx, sy) [h, w] in T, clamped to +-2^30."""
    m = np.asarray(row[A:TY + 1], F32).astype(T)
    if defect == "forward matrix":  # the row's matrix taken for the forward map: sample through its inverse
        a, b, tx, c, d, ty = m.astype(F64)
        det = a * d - b * c
        m = np.array([d / det, -b / det, -(d * tx - b * ty) / det, -c / det, a / det, -(-c * tx + a * ty) / det]).astype(T)
    a, b, tx, c, d, ty = (T(v) for v in m)
    cx, cy = T(w - 1) * T(0.5), T(h - 1) * T(0.5)
    ys, xs = np.meshgrid(np.arange(h).astype(T), np.arange(w).astype(T), indexing="ij")
    dx, dy = xs - cx, ys - cy
    sx = ((a * dx + b * dy) + tx) + cx
    sy = ((c * dx + d * dy) + ty) + cy
    lim = T(COORD_MAX)
    return np.fmin(np.fmax(sx, -lim), lim).astype(T), np.fmin(np.fmax(sy, -lim), lim).astype(T)


def gather(prev, row, border, T, defect=None):
    """p [3, h, w]: the bilinear tap of ``prev`` [3, h, w] (T) at the row's source coordinates."""
    _, h, w = prev.shape
    sx, sy = coordinates(row, h, w, T, defect)
    flx, fly = np.floor(sx), np.floor(sy)
    fx, fy = (sx - flx).astype(T), (sy - fly).astype(T)
    ix, iy = flx.astype(np.int64), fly.astype(np.int64)
    x0, vx0 = fold_index(ix, w, border, defect)
    x1, vx1 = fold_index(ix + 1, w, border, defect)
    y0, vy0 = fold_index(iy, h, border, defect)
    y1, vy1 = fold_index(iy + 1, h, border, defect)
    black = T(-1)

    def tap(y, x, ok):
        return np.where(ok[None], prev[:, y, x], black).astype(T)

    v00, v01 = tap(y0, x0, vy0 & vx0), tap(y0, x1, vy0 & vx1)
    v10, v11 = tap(y1, x0, vy1 & vx0), tap(y1, x1, vy1 & vx1)
    with np.errstate(invalid="ignore", over="ignore"):
        top = (v00 + fx * (v01 - v00)).astype(T)
        bottom = (v10 + fx * (v11 - v10)).astype(T)
        return (top + fy * (bottom - top)).astype(T)


def combine_frame(cur, p, row, mode, T, defect=None):
    """out [3, h, w] of one non-neutral frame: cur, p in T."""
    dry, limit = T(row[DRY]), T(row[LIMIT])
    g = (T(row[GAIN]) * np.asarray(row[TINT:TINT + 3], F32).astype(T)).astype(T)[:, None, None]  # gain x tint, rounded once
    with np.errstate(invalid="ignore", over="ignore"):
        if defect == "signed decay":  # the trail decays towards grey: no unit space
            u_prev, u_cur = p, cur
        else:
            u_prev, u_cur = T(0.5) * p + T(0.5), T(0.5) * cur + T(0.5)
        a, b = (dry * u_cur).astype(T), (g * u_prev).astype(T)
        if mode == "add":
            u = a + b
        elif mode == "max":
            u = np.fmax(a, b)
        elif mode == "screen":
            u = T(1) - (T(1) - clamp01(a)) * (T(1) - clamp01(b))
        else:
            raise ValueError(mode)
        u = np.fmin(u.astype(T), limit)
        if defect == "signed decay":
            return u.astype(T)
        return (T(2) * u - T(1)).astype(T)


def run(cur, rows, mode, border, state=None, dtype=F64, defect=None):
    """One call of the entry: cur [B, 3, h, w], rows [B, 16] -> (out [B, 3, h, w], the new state [3, h, w]), both ``dtype``.
    ``state`` None: black."""
    T = dtype
    cur = np.asarray(cur)
    x = cur.astype(T)
    b, _, h, w = x.shape
    prev = np.full((3, h, w), -1, T) if state is None else np.asarray(state).astype(T)
    out = np.empty_like(x)
    for i in range(b):
        row = np.asarray(rows[i], F32)
        if is_neutral(row):
            out[i] = cur[i] if cur.dtype == T else x[i]  # (the bits themselves)
        else:
            out[i] = combine_frame(x[i], gather(prev, row, border, T, defect), row, mode, T, defect)
        prev = x[i] if defect == "no recursion" else out[i]
    return out, prev.copy()


def run_calls(cur, rows, mode, border, splits=None, dtype=F64, defect=None):
    """Consecutive calls over the frames cut at ``splits`` (e.g. (2,) : frames 0 .. 1, then the rest), the state carried from call to
    call (``defect="no carry"``: every call starts from black) -> out [B, 3, h, w]."""
    edges = [0] + list(splits or ()) + [len(cur)]
    outs, state = [], None
    for lo, hi in zip(edges[:-1], edges[1:]):
        out, state = run(cur[lo:hi], rows[lo:hi], mode, border, None if defect == "no carry" else state, dtype, defect)
        outs.append(out)
    return np.concatenate(outs)


# ------------------------------------------------------------------------------------------------ allowance
def allowance(e32, e64):
    """What a float32 implementation in the header's order may differ from float64 by, per case: 4 x the emulation's own error, with a
    floor of 8 ulp of the value range (the largest magnitude the float64 result reaches, at least 1)."""
    e64 = np.asarray(e64, F64)
    scale = max(1.0, float(np.abs(e64).max()))
    return max(4.0 * float(np.abs(np.asarray(e32, F64) - e64).max()), 16 * EPS * scale)


def ceiling(cur, rows, out64):
    """An upper bound of the emulation's error after the case's frames, for rows with gain |tint| <= 1 (every case of CASES).
    One frame, values bounded by M = max(1, max |out|, max |cur|):
      * the state's error e enters through a convex combination of four taps (<= e), is halved into unit space, multiplied by
        g <= 1 and doubled on the way out: it is passed on at most unchanged — the growth is LINEAR in the number of frames;
      * the frame's own roundings: 3 lerps of 3 operations on magnitudes <= 2 M, the two unit maps, the products, the combine (screen: 5
        operations on values <= 1), the limit (exact) and the way out: fewer than 24 roundings of magnitudes <= 2 M, doubled at the end:
        <= 96 EPS M;
      * the coordinate: 5 roundings per axis on magnitudes <= S = (|a| + |b|) (w + h) / 2 + |t| + max(w, h) (matrix entries bounded by 4 here),
        d <= 5 . 2 EPS S, which moves the tap by at most d x (the difference of neighbouring taps <= 2 M) per axis (continuity, above).
    Sum over the frames."""
    m = max(1.0, float(np.abs(out64).max()), float(np.abs(np.asarray(cur, F64)).max()))
    _, _, h, w = np.asarray(cur).shape
    total = 0.0
    for row in rows:
        mat = np.abs(np.asarray(row[A:TY + 1], F64))
        s = (mat[[0, 1, 3, 4]].max() * 2) * (w + h) / 2 + max(mat[2], mat[5]) + max(w, h)
        total += 96 * EPS * m + 2 * (10 * EPS * s) * 2 * m
    return total


# ------------------------------------------------------------------------------------------------ operands and the case list
def image(shape, tag, dyadic):
    """[B, 3, h, w] float32 in about [-1, 1.2]: a smooth part and noise; ``dyadic``: on a 2^-8 grid."""
    rng = np.random.default_rng(int.from_bytes(repr(("feedback", tag, tuple(shape))).encode(), "little") % (2 ** 32))
    b, c, h, w = shape
    ys, xs = np.meshgrid(np.linspace(0, 1, h), np.linspace(0, 1, w), indexing="ij")
    smooth = np.sin(3.1 * xs + np.arange(c)[:, None, None])[None] * np.cos(2.3 * ys + np.arange(b)[:, None, None, None])
    x = 0.6 * smooth + 0.5 * rng.uniform(-1, 1, shape) + 0.1
    if dyadic:
        x = np.round(x * 256) / 256
    return x.astype(F32)


PLANES = ((1, 1), (3, 5), (17, 33), (64, 68), (65, 63))
BATCHES = (1, 2, 5)
KINDS = ("still", "translate", "zoomrot", "mixed", "neutral mid")


def rows_of(kind, batch, h, w, dyadic):
    """[batch, 16]: the rows of a case.  Dyadic: gains and tints powers of two, integer translations, no zoom or rotation (``zoomrot``
    then turns by exact quarter turns and zooms by 2 / 0.5: every coordinate and weight stays exact)."""
    rows = []
    for i in range(batch):
        if dyadic:
            gain, tint, dry = 0.5, (1.0, 0.5, 0.25), (1.0, 0.5)[i % 2]
        else:
            gain, tint, dry = 0.83 - 0.05 * (i % 3), (1.0, 0.9 - 0.1 * (i % 2), 0.71), 1.0 - 0.13 * (i % 2)
        if kind == "still":
            m = IDENTITY
        elif kind == "translate":
            m = (1, 0, (2, -1, 7)[i % 3], 0, 1, (-1, 3, -5)[i % 3])
        elif kind == "zoomrot":
            if dyadic:
                m = ((0, -1, 0, 1, 0, 0), (0.5, 0, 1, 0, 0.5, 0), (2, 0, 0, 0, 2, -1))[i % 3]
            else:
                m = inverse_matrix(1.03 + 0.02 * i, 7.0 - 3.0 * i, (0.013, -0.021), h, w)
        elif kind == "mixed":  # still, still, moving, still, moving
            if i in (2, 4):
                m = (1, 0, 1, 0, 1, -2) if dyadic else inverse_matrix(0.97, -4.0, (0.0, 0.03), h, w)
            else:
                m = IDENTITY
        elif kind == "neutral mid":  # a neutral row in the middle (the only one of a batch of 1), moving rows round it
            m = (1, 0, -1, 0, 1, 1) if dyadic else inverse_matrix(1.05, 2.5, (0.02, 0.01), h, w)
            if i == batch // 2:
                gain, dry = 0.0, 1.0
        else:
            raise ValueError(kind)
        rows.append(make_row(m, gain, tint, dry, limit=(1.5 if i % 2 else 4.0)))
    return np.stack(rows)


def cases():
    """Every GPU case: (plane, batch, kind, dyadic); each is run for every mode x border."""
    return [(p, b, k, d) for p in PLANES for b in BATCHES for k in KINDS for d in (True, False)]


@functools.lru_cache(maxsize=None)
def case_operands(plane, batch, kind, dyadic):
    h, w = plane
    cur = image((batch, 3, h, w), kind, dyadic)
    rows = rows_of(kind, batch, h, w, dyadic)
    cur.setflags(write=False)
    rows.setflags(write=False)
    return cur, rows


@functools.lru_cache(maxsize=None)
def case_reference(plane, batch, kind, dyadic, mode, border, splits=None):
    """(out32, out64, allowance): computed once, shared, read-only."""
    cur, rows = case_operands(plane, batch, kind, dyadic)
    e32 = run_calls(cur, rows, mode, border, splits, F32)
    e64 = run_calls(cur, rows, mode, border, splits, F64)
    e32.setflags(write=False)
    e64.setflags(write=False)
    return e32, e64, allowance(e32, e64)
