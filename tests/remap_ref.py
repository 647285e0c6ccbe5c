"""References for maua_bend_remap_f32 (include/maua_hip.h: mirror, kaleidoscope, swirl, ripple, displace).

``remap64`` is the contract of the header in float64, in its own words (numpy's floor-modulo, hypot, where).  ``remap32`` is a stand-in
for the device: the kernel's arithmetic restated step by step in numpy float32 (without the fused multiply-adds and with numpy's
float32 libm instead of the device's).  ``bound`` is the per-element error bound the tests hold the device (and the stand-in) to, and
``coordinate_allowance`` its delta; ``DEFECTS`` are deliberate mistakes that bound must reject.

Parameter rows are the DEVICE's rows [rows, 4] (radians, unit normals); ``rows_from_degrees`` is the host's conversion for the ops whose
public parameters are angles in degrees."""
import numpy as np

MIRROR, KALEIDOSCOPE, SWIRL, RIPPLE, DISPLACE = range(5)
OP_NAMES = ("mirror", "kaleidoscope", "swirl", "ripple", "displace")
REFLECT, CLAMP = 0, 1
CHUNK = 16  # REMAP_CHUNK of csrc/bend_remap.hip: channels a thread walks with one set of taps
DEFECTS = ("half pixel", "period 2n", "swapped weights", "sectors + 1", "field frame + 1", "degrees as radians")
F32 = np.float32


def bad_row(op, p):
    """True where the device passes the sample through: a non-finite used parameter, or p1 <= 0 for swirl / ripple."""
    used = {MIRROR: 3, KALEIDOSCOPE: 3, SWIRL: 2, RIPPLE: 3, DISPLACE: 2}[op]
    p = np.asarray(p, np.float64)
    return bool(not np.isfinite(p[:used]).all() or (op in (SWIRL, RIPPLE) and p[1] <= 0))


def rows_from_degrees(op, rows, as_radians=False):
    """Device rows of the public parameters (angle columns in degrees): mirror (angle, offset) -> (cos, sin, offset, 0); kaleidoscope
    (sectors, angle, rotation) and swirl (strength, radius): the angle columns converted.  ``as_radians``: the defect of handing the
    degrees over as they are."""
    rows = np.asarray(rows, np.float64)
    k = 1.0 if as_radians else np.pi / 180.0
    out = np.zeros((rows.shape[0], 4))
    if op == MIRROR:
        out[:, 0], out[:, 1], out[:, 2] = np.cos(rows[:, 0] * k), np.sin(rows[:, 0] * k), rows[:, 1]
    elif op == KALEIDOSCOPE:
        out[:, 0], out[:, 1], out[:, 2] = rows[:, 0], rows[:, 1] * k, rows[:, 2] * k
    elif op == SWIRL:
        out[:, 0], out[:, 1] = rows[:, 0] * k, rows[:, 1]
    else:
        out[:, : rows.shape[1]] = rows
    return out.astype(np.float32)


# ---------------------------------------------------------------------------------------------------------------- float64 reference
def _pixels(h, w, dtype=np.float64):
    oy, ox = np.meshgrid(np.arange(h, dtype=dtype), np.arange(w, dtype=dtype), indexing="ij")
    return ox, oy


def _bilinear64(planes, sx, sy, swap=False):
    """planes [..., n_y, n_x] at coordinates already inside the planes; x1 = min(x0 + 1, n - 1)."""
    ny, nx = planes.shape[-2:]
    x0 = np.clip(np.floor(sx).astype(np.int64), 0, nx - 1)
    y0 = np.clip(np.floor(sy).astype(np.int64), 0, ny - 1)
    x1, y1 = np.minimum(x0 + 1, nx - 1), np.minimum(y0 + 1, ny - 1)
    wx, wy = sx - x0, sy - y0
    if swap:
        wx, wy = wy, wx
    top = (1 - wx) * planes[..., y0, x0] + wx * planes[..., y0, x1]
    bottom = (1 - wx) * planes[..., y1, x0] + wx * planes[..., y1, x1]
    return (1 - wy) * top + wy * bottom


def displacement64(field, h, w, position, defect=None):
    """D(o, p1) [2, h, w]: the bank [F, 2, fh, fw] stretched over the map, blended between the two frames round the loop position."""
    field = np.asarray(field, np.float64)
    frames, _, fh, fw = field.shape
    ox, oy = _pixels(h, w)
    u = ox * ((fw - 1) / (w - 1)) if w > 1 else np.zeros_like(ox)
    v = oy * ((fh - 1) / (h - 1)) if h > 1 else np.zeros_like(oy)
    t = int(np.floor(position))
    ft = position - t
    t0 = (t + (1 if defect == "field frame + 1" else 0)) % frames
    t1 = (t0 + 1) % frames
    return (1 - ft) * _bilinear64(field[t0], u, v) + ft * _bilinear64(field[t1], u, v)


def coords64(op, h, w, p, field=None, defect=None):
    """Unfolded source coordinate (sx, sy) [h, w] of every output pixel for the device row ``p``."""
    p = np.asarray(p, np.float32).astype(np.float64)
    ox, oy = _pixels(h, w)
    cx, cy = (w - 1) / 2, (h - 1) / 2
    dx, dy = ox - cx, oy - cy
    r = np.hypot(dx, dy)
    if op == MIRROR:
        t = dx * p[0] + dy * p[1] - p[2]
        sx, sy = np.where(t < 0, ox - 2 * t * p[0], ox), np.where(t < 0, oy - 2 * t * p[1], oy)
    elif op == KALEIDOSCOPE:
        n = float(np.clip(np.rint(p[0]), 1, 64)) + (1 if defect == "sectors + 1" else 0)
        ws = 2 * np.pi / n
        a = np.mod(np.arctan2(dy, dx) - p[1], ws)
        a = np.where(a > ws / 2, ws - a, a) + p[1] + p[2]
        sx, sy = cx + r * np.cos(a), cy + r * np.sin(a)
    elif op == SWIRL:
        phi = p[0] * np.exp(-r / p[1])
        sx, sy = cx + np.cos(phi) * dx - np.sin(phi) * dy, cy + np.sin(phi) * dx + np.cos(phi) * dy
    elif op == RIPPLE:
        k = p[0] * np.sin(2 * np.pi * (r / p[1] - p[2]))
        q = np.divide(k, r, out=np.zeros_like(r), where=r > 0)
        sx, sy = ox + q * dx, oy + q * dy
    else:
        d = displacement64(field, h, w, float(p[1]), defect)
        sx, sy = ox + p[0] * d[0], oy + p[0] * d[1]
    if defect == "half pixel":
        sx, sy = sx + 0.5, sy + 0.5
    return sx, sy


def fold64(s, n, border, defect=None):
    """s into [0, n - 1]: reflected about the first and last element (period 2 (n - 1)) or clamped."""
    if n == 1:
        return np.zeros_like(s)
    if border == REFLECT:
        if defect == "period 2n":  # the reflection that repeats the edge: about -1/2 and n - 1/2
            m = np.mod(s + 0.5, 2 * n)
            s = np.where(m > n, 2 * n - m, m) - 0.5
        else:
            m = np.mod(s, 2 * (n - 1))
            s = np.where(m > n - 1, 2 * (n - 1) - m, m)
    return np.clip(s, 0, n - 1)


def remap64(x, op, border, rows, field=None, sel=None, defect=None):
    """(y, fsx, fsy): the float64 result for x [B, C, h, w] with the device row ``rows[b]`` per sample and the channel selection ``sel``
    (boolean [C] or None); fsx, fsy [B, h, w] are the folded coordinates (of a sample that passes through: its own pixels)."""
    x = np.asarray(x, np.float64)
    b, c, h, w = x.shape
    y = x.copy()
    ox, oy = _pixels(h, w)
    fsx, fsy = np.broadcast_to(ox, (b, h, w)).copy(), np.broadcast_to(oy, (b, h, w)).copy()
    for i in range(b):
        if bad_row(op, rows[i]):
            continue
        sx, sy = coords64(op, h, w, rows[i], field, defect)
        fsx[i], fsy[i] = fold64(sx, w, border, defect), fold64(sy, h, border, defect)
        full = _bilinear64(x[i], fsx[i], fsy[i], swap=defect == "swapped weights")
        if sel is None:
            y[i] = full
        else:
            y[i, sel] = full[sel]
    return y, fsx, fsy


# ---------------------------------------------------------------------------------------------------------------- float32 stand-in
def _fold32(s, n, border):
    last = F32(n - 1)
    if border == REFLECT and n > 1:
        period = F32(2) * last
        s = np.abs(s)
        s = s - period * np.floor(s / period)
        s = np.where(s > last, period - s, s)
    with np.errstate(invalid="ignore"):
        return np.minimum(np.fmax(s, F32(0)), last).astype(F32)  # fmax: a NaN becomes 0, as on the device


def _taps32(s, n):
    i0 = np.clip(s.astype(np.int32), 0, n - 1)
    return i0, np.minimum(i0 + 1, n - 1), (s - i0.astype(F32)).astype(F32)


def _lerp32(a, b, t):
    return (t * (b - a) + a).astype(F32)


def _plane32(f, i0, i1, j0, j1, wu, wv):
    return _lerp32(_lerp32(f[j0, i0], f[j0, i1], wu), _lerp32(f[j1, i0], f[j1, i1], wu), wv)


def coords32(op, h, w, p, field=None):
    """The kernel's source coordinate in float32 steps (unfolded)."""
    p = np.asarray(p, F32)
    fx, fy = _pixels(h, w, F32)
    cx, cy = F32(0.5) * F32(w - 1), F32(0.5) * F32(h - 1)
    dx, dy = fx - cx, fy - cy
    two_pi = F32(6.28318530717958648)
    with np.errstate(all="ignore"):
        if op == MIRROR:
            t = dx * p[0] + dy * p[1] - p[2]
            sx, sy = np.where(t < 0, fx - F32(2) * t * p[0], fx), np.where(t < 0, fy - F32(2) * t * p[1], fy)
        elif op == KALEIDOSCOPE:
            n = np.minimum(np.maximum(np.rint(p[0]), F32(1)), F32(64))
            ws = two_pi / n
            r = np.sqrt(dx * dx + dy * dy)
            a = np.arctan2(dy, dx) - p[1]
            a = a - ws * np.floor(a / ws)
            a = np.where(a > F32(0.5) * ws, ws - a, a)
            a = a + (p[1] + p[2])
            sx, sy = cx + r * np.cos(a), cy + r * np.sin(a)
        elif op == SWIRL:
            r = np.sqrt(dx * dx + dy * dy)
            phi = p[0] * np.exp(-r / p[1])
            cs, sn = np.cos(phi), np.sin(phi)
            sx, sy = cx + (cs * dx - sn * dy), cy + (sn * dx + cs * dy)
        elif op == RIPPLE:
            r = np.sqrt(dx * dx + dy * dy)
            q = p[0] * np.sin(two_pi * (r / p[1] - p[2])) / r
            sx, sy = np.where(r > 0, fx + q * dx, fx), np.where(r > 0, fy + q * dy, fy)
        else:
            field = np.asarray(field, F32)
            frames, _, fh, fw = field.shape
            ku = F32(fw - 1) / F32(w - 1) if w > 1 else F32(0)
            kv = F32(fh - 1) / F32(h - 1) if h > 1 else F32(0)
            u = np.minimum(np.maximum(fx * ku, F32(0)), F32(fw - 1))
            v = np.minimum(np.maximum(fy * kv, F32(0)), F32(fh - 1))
            i0, i1, wu = _taps32(u, fw)
            j0, j1, wv = _taps32(v, fh)
            t = np.floor(p[1])
            ft = F32(p[1] - t)
            tw = np.minimum(np.fmax(t - F32(frames) * np.floor(t / F32(frames)), F32(0)), F32(frames - 1))
            t0 = min(int(tw), frames - 1)
            t1 = 0 if t0 + 1 == frames else t0 + 1
            ddx = _lerp32(_plane32(field[t0, 0], i0, i1, j0, j1, wu, wv), _plane32(field[t1, 0], i0, i1, j0, j1, wu, wv), ft)
            ddy = _lerp32(_plane32(field[t0, 1], i0, i1, j0, j1, wu, wv), _plane32(field[t1, 1], i0, i1, j0, j1, wu, wv), ft)
            sx, sy = fx + p[0] * ddx, fy + p[0] * ddy
    return sx.astype(F32), sy.astype(F32)


def remap32(x, op, border, rows, field=None, sel=None):
    """(y, fsx, fsy, sx, sy) in float32: the stand-in's result, its folded and its unfolded coordinates [B, h, w]."""
    x = np.asarray(x, F32)
    b, c, h, w = x.shape
    y = x.copy()
    fx, fy = _pixels(h, w, F32)
    sx, sy = np.broadcast_to(fx, (b, h, w)).copy(), np.broadcast_to(fy, (b, h, w)).copy()
    fsx, fsy = sx.copy(), sy.copy()
    for i in range(b):
        if bad_row(op, rows[i]):
            continue
        sx[i], sy[i] = coords32(op, h, w, rows[i], field)
        fsx[i], fsy[i] = _fold32(sx[i], w, border), _fold32(sy[i], h, border)
        x0, x1, wx = _taps32(fsx[i], w)
        y0, y1, wy = _taps32(fsy[i], h)
        v00, v01, v10, v11 = x[i][:, y0, x0], x[i][:, y0, x1], x[i][:, y1, x0], x[i][:, y1, x1]
        full = _lerp32(_lerp32(v00, v01, wx), _lerp32(v10, v11, wx), wy)
        lo, hi = np.minimum(np.minimum(v00, v01), np.minimum(v10, v11)), np.maximum(np.maximum(v00, v01), np.maximum(v10, v11))
        full = np.minimum(np.maximum(full, lo), hi)
        if sel is None:
            y[i] = full
        else:
            y[i, sel] = full[sel]
    return y, fsx, fsy, sx, sy


# ---------------------------------------------------------------------------------------------------------------- the bound
def coordinate_allowance(op, shape, border, rows, field=None, factor=4.0):
    """delta of ``bound`` for one (op, shape, parameter set): ``factor`` x the largest deviation, in pixels, between the float32
    stand-in's coordinates and the float64 ones (unfolded and folded; the fold is a contraction, so a device whose unfolded coordinate is
    within delta has its folded one within delta too).  The factor 4 leaves room for the device's libm and its fused multiply-adds
    differing from numpy's float32 functions by a few ulp: each is one more rounding pattern of the same expression, whose deviation from
    float64 is of the size of the stand-in's."""
    b, c, h, w = shape
    deviation = 0.0
    for i in range(len(rows)):
        if bad_row(op, rows[i]):
            continue
        sx64, sy64 = coords64(op, h, w, rows[i], field)
        sx32, sy32 = coords32(op, h, w, rows[i], field)
        deviation = max(deviation, float(np.abs(sx32 - sx64).max()), float(np.abs(sy32 - sy64).max()))
        deviation = max(deviation, float(np.abs(_fold32(sx32, w, border) - fold64(sx64, w, border)).max()),
                        float(np.abs(_fold32(sy32, h, border) - fold64(sy64, h, border)).max()))
    return factor * deviation


def bound(x, fsx, fsy, delta):
    """Per-element error bound [B, C, h, w] of a bilinear sample whose coordinate is off by at most ``delta`` pixels per axis:
    (Lx + Ly) delta + 8 * 2^-23 * max|tap|, Lx / Ly the largest difference of horizontally / vertically adjacent elements in the 4 x 4
    neighbourhood (x0 - 1 .. x0 + 2, y0 - 1 .. y0 + 2, clipped to the map) of the folded float64 coordinate — a Lipschitz constant of the
    bilinear interpolant on every cell a coordinate within 1 pixel can fall into; the second term covers the blend's own roundings."""
    x = np.asarray(x, np.float64)
    b, c, h, w = x.shape
    out = np.empty_like(x)
    for i in range(b):
        x0 = np.clip(np.floor(fsx[i]).astype(np.int64), 0, w - 1)
        y0 = np.clip(np.floor(fsy[i]).astype(np.int64), 0, h - 1)
        cols = [np.clip(x0 + k, 0, w - 1) for k in (-1, 0, 1, 2)]
        rws = [np.clip(y0 + k, 0, h - 1) for k in (-1, 0, 1, 2)]
        nb = [[x[i][:, rws[r], cols[q]] for q in range(4)] for r in range(4)]  # [4][4] of [C, h, w]
        lx = np.max([np.abs(nb[r][q + 1] - nb[r][q]) for r in range(4) for q in range(3)], axis=0)
        ly = np.max([np.abs(nb[r + 1][q] - nb[r][q]) for r in range(3) for q in range(4)], axis=0)
        tap = np.max([np.abs(nb[r][q]) for r in (1, 2) for q in (1, 2)], axis=0)
        out[i] = (lx + ly) * delta + 8 * 2.0 ** -23 * tap
    return out


# ---------------------------------------------------------------------------------------------------------------- shared test cases
# The smallest shapes that can still go wrong: an axis of length 1 and r = 0; odd sizes with the centre on a pixel; the wide layer-0 map;
# ragged tiles and 33 channels (two chunks of 16 + 1); more than one block per plane.  5 and 8 channels are below the chunk.
SHAPES = [(1, 1, 1, 1), (2, 5, 5, 7), (8, 32, 4, 8), (3, 33, 33, 65), (1, 8, 130, 258)]
FIELD_SHAPE = (4, 2, 6, 9)


def public_rows(op, h, w):
    """Four parameter rows of moderate size for an h x w map, in the public units (angles in degrees): mirror (angle, offset),
    kaleidoscope (sectors, angle, rotation), swirl (strength, radius), ripple (amplitude, wavelength, phase), displace (amplitude,
    loop position).  The second ripple is the hardest case of the issue (amplitude 9, wavelength 3.3, phase -1.7)."""
    s = float(max(min(h, w), 2))
    return np.array({MIRROR: [[30, 0.15 * s], [90, 0], [200, -0.2 * s], [-45, 0.4 * s]],
                     KALEIDOSCOPE: [[6, 17, 28], [3, -57, 115], [1, 0, 40], [64, 3, -8]],
                     SWIRL: [[70, 0.6 * s], [-170, 0.25 * s], [400, s], [20, 0.1 * s]],
                     RIPPLE: [[0.12 * s, 0.4 * s, 0.25], [9, 3.3, -1.7], [-0.3 * s, 0.8 * s, 3.6], [1.0, 2.0, 0.5]],
                     DISPLACE: [[0.2 * s, 0.4], [-0.35 * s, 5.75], [1.5, -2.25], [0.5 * s, 3.0]]}[op], np.float64)


def device_rows(op, h, w):
    return rows_from_degrees(op, public_rows(op, h, w))


def plain_map(shape, tag="x"):
    """Seeded N(0, 1) map without outliers (a 1e6 among the taps would make the bound too loose to catch anything)."""
    from maua_stylegan2_amd import seeding

    return seeding.seeded_array(51, f"remap {tag}{tuple(shape)}", shape)


def field_bank(shape=FIELD_SHAPE, tag="field"):
    from maua_stylegan2_amd import seeding

    return seeding.seeded_array(52, f"remap {tag}{tuple(shape)}", shape)


def selection(kind, c):
    """Boolean [c] channel selection, or None for a NULL mask."""
    if kind == "none":
        return None
    sel = np.zeros(c, bool)
    if kind == "all":
        sel[:] = True
    elif kind == "third":
        sel[::3] = True
    return sel
