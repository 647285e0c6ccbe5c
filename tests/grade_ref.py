"""The numpy twin of csrc/grade.hip (no device): the definition of the colour grade, the row helpers, and the case list of the GPU tests.

Two levels, one code path (``grade(..., dtype=)``):
  float64   the definition: every operation of include/maua_hip.h's statement in double;
  float32   the same operations, in the same order, each rounded to float32 on its own (numpy never contracts a multiply-add): equal to the
            device bit for bit wherever power == 1.  Its powf is the float64 power of the float32 base rounded once (the device's powf
            is within a few ulp of that, not equal), so with power != 1 it sets the tolerance instead (tests/test_grade_gpu.py).

A row is 24 float32: slope[3] offset[3] power[3] M[9, row-major: out_c = sum_k M[c][k] t_k] bias[3] lut_mix reserved[2].  A LUT is
[N, N, N, 3] indexed [blue, green, red] (.cube order: red fastest), domain [0, 1].

``variant``: deliberately WRONG definitions ("trilinear", "transposed", "power_first"; "bt601" is a wrong row helper, saturation_matrix's
``weights``) that the GPU case list must tell from the right one (tests/test_grade_host.py).
"""
import numpy as np

F32 = np.float32
ROW = 24
SLOPE, OFFSET, POWER, MATRIX, BIAS, MIX = 0, 3, 6, 9, 18, 21
REC709 = (0.2126, 0.7152, 0.0722)
BT601 = (0.299, 0.587, 0.114)
# tetra's comparison chain: (hi, mid, lo) axes (0 = red) per case, in the order the chain tests them
ORDERS = np.array([[0, 1, 2], [0, 2, 1], [2, 0, 1], [2, 1, 0], [1, 2, 0], [1, 0, 2]])


# ------------------------------------------------------------------------------------------------------------------------ row helpers
def identity_row():
    row = np.zeros(ROW, np.float64)
    row[SLOPE:SLOPE + 3] = 1
    row[POWER:POWER + 3] = 1
    row[MATRIX:MATRIX + 9] = np.eye(3).reshape(-1)
    return row


def exposure_slope(stops):
    return 2.0 ** np.float64(stops)


def contrast_slope_offset(contrast, pivot=0.5):
    """c (t - pivot) + pivot = c t + pivot (1 - c)."""
    return np.float64(contrast), np.float64(pivot) * (1.0 - np.float64(contrast))


def gamma_power(gamma):
    return 1.0 / np.float64(gamma)


def saturation_matrix(s, weights=REC709):
    """ASC CDL saturation: out = luma + s (in - luma), luma with Rec. 709 weights."""
    w = np.asarray(weights, np.float64)
    return (1.0 - s) * np.tile(w, (3, 1)) + s * np.eye(3)


def hue_matrix(degrees):
    """The hueRotate matrix of the SVG / CSS filter specification (feColorMatrix type="hueRotate"), luma-preserving with its rounded
    weights 0.213 / 0.715 / 0.072; 0 degrees is the identity exactly."""
    if degrees == 0:
        return np.eye(3)
    a = np.deg2rad(np.float64(degrees))
    base = np.array([[0.213, 0.715, 0.072]] * 3)
    cos = np.array([[0.787, -0.715, -0.072], [-0.213, 0.285, -0.072], [-0.213, -0.715, 0.928]])
    sin = np.array([[-0.213, -0.715, 0.928], [0.143, 0.140, -0.283], [-0.787, 0.715, 0.072]])
    return base + np.cos(a) * cos + np.sin(a) * sin


def make_row(exposure=0.0, contrast=1.0, pivot=0.5, slope=1.0, offset=0.0, power=1.0, gamma=None, white_balance=None, saturation=1.0, hue=0.0,
             matrix=None, bias=0.0, lut_mix=1.0, sat_weights=REC709):
    """One row (float64 [24]) from the user-level parameters, as ar.Grade composes them: gain = 2^exposure * white_balance * slope, then the
    offset, then the contrast about the pivot (slope = gain * c, offset = offset * c + pivot (1 - c)); power = power / gamma; matrix =
    hue . saturation . user matrix (the user matrix is applied first)."""
    row = identity_row()
    gain = exposure_slope(exposure) * np.broadcast_to(np.asarray(1.0 if white_balance is None else white_balance, np.float64), 3) * np.broadcast_to(
        np.asarray(slope, np.float64), 3)
    c, off_c = contrast_slope_offset(contrast, pivot)
    row[SLOPE:SLOPE + 3] = gain * c
    row[OFFSET:OFFSET + 3] = np.broadcast_to(np.asarray(offset, np.float64), 3) * c + off_c
    row[POWER:POWER + 3] = np.broadcast_to(np.asarray(power, np.float64), 3) * (1.0 if gamma is None else gamma_power(np.broadcast_to(np.asarray(gamma, np.float64), 3)))
    user = np.eye(3) if matrix is None else np.asarray(matrix, np.float64).reshape(3, 3)
    row[MATRIX:MATRIX + 9] = (hue_matrix(hue) @ saturation_matrix(saturation, sat_weights) @ user).reshape(-1)
    row[BIAS:BIAS + 3] = np.broadcast_to(np.asarray(bias, np.float64), 3)
    row[MIX] = lut_mix
    return row


def is_identity(rows, has_lut):
    """[n] bool: the identity rule on float32 rows [n, >= 24]."""
    rows = np.asarray(rows, F32)[:, :ROW]
    ident = identity_row().astype(F32)
    same = (rows[:, :MIX] == ident[None, :MIX]).all(axis=1)
    return same & ((rows[:, MIX] == 0) | (not has_lut))


# ------------------------------------------------------------------------------------------------------------------------ the definition
def clamp01(a):
    """fminf(fmaxf(a, 0), 1): a NaN becomes 0."""
    return np.clip(np.where(np.isnan(a), a.dtype.type(0), a), a.dtype.type(0), a.dtype.type(1))


def _pow(t, p, dtype):
    """t ** p for t in [0, 1]: the float64 power of the base, rounded once to ``dtype``; 0 stays 0."""
    with np.errstate(all="ignore"):
        return np.power(t.astype(np.float64), np.float64(p)).astype(dtype)


def tetra_setup(m, n, dtype=np.float64):
    """m [..., 3] in [0, 1] -> (cell index i [..., 3], order code [...], weights [..., 4]) of the tetrahedral interpolation in an n^3 lattice."""
    p = m * dtype(n - 1)
    i = np.minimum(p.astype(np.int64), n - 2)
    f = p - i.astype(dtype)
    fr, fg, fb = f[..., 0], f[..., 1], f[..., 2]
    a = fr >= fg
    code = np.select([a & (fg >= fb), a & (fr >= fb), a, fb >= fg, fb >= fr], [0, 1, 2, 3, 4], default=5)
    order = ORDERS[code]
    hi, mid, lo = (np.take_along_axis(f, order[..., k:k + 1], axis=-1)[..., 0] for k in range(3))
    w = np.stack([dtype(1) - hi, hi - mid, mid - lo, lo], axis=-1)
    assert w.dtype == dtype
    return i, code, w


def tetra_vertices(i, code):
    """The four lattice points [..., 4, 3] (red, green, blue indices) of the tetrahedron: c000, + hi's axis, + mid's axis, c111."""
    order = ORDERS[code]
    eye = np.eye(3, dtype=np.int64)
    v0 = i
    v1 = v0 + eye[order[..., 0]]
    v2 = v1 + eye[order[..., 1]]
    return np.stack([v0, v1, v2, i + 1], axis=-2)


def tetra(lut, m, dtype=np.float64, max_index=None):
    """Tetrahedral interpolation of lut [N, N, N, 3] at m [..., 3]; ``max_index``: a list that receives the largest index read."""
    lut = np.asarray(lut).astype(dtype)
    n = lut.shape[0]
    i, code, w = tetra_setup(m, n, dtype)
    v = tetra_vertices(i, code)
    if max_index is not None:
        max_index.append(int(v.max()))
    c = lut[v[..., 2], v[..., 1], v[..., 0]]  # [..., 4, 3]
    return ((w[..., 0:1] * c[..., 0, :] + w[..., 1:2] * c[..., 1, :]) + w[..., 2:3] * c[..., 2, :]) + w[..., 3:4] * c[..., 3, :]


def trilinear(lut, m, dtype=np.float64):
    """(the wrong variant) trilinear interpolation in the same cell."""
    lut = np.asarray(lut).astype(dtype)
    n = lut.shape[0]
    p = m * dtype(n - 1)
    i = np.minimum(p.astype(np.int64), n - 2)
    f = p - i.astype(dtype)
    out = np.zeros(m.shape, dtype)
    for db in (0, 1):
        for dg in (0, 1):
            for dr in (0, 1):
                wgt = (f[..., 0] if dr else 1 - f[..., 0]) * (f[..., 1] if dg else 1 - f[..., 1]) * (f[..., 2] if db else 1 - f[..., 2])
                out = out + wgt[..., None] * lut[i[..., 2] + db, i[..., 1] + dg, i[..., 0] + dr]
    return out.astype(dtype)


def barycentric(lut, m):
    """tetra written independently (float64): sort the fractions, walk from c000 to c111 adding the axis of the largest remaining fraction."""
    lut = np.asarray(lut, np.float64)
    n = lut.shape[0]
    flat = np.asarray(m, np.float64).reshape(-1, 3)
    out = np.empty_like(flat)
    for k, px in enumerate(flat):
        p = px * (n - 1)
        i = np.minimum(np.floor(p).astype(int), n - 2)
        f = p - i
        axes = sorted(range(3), key=lambda a: -f[a])  # (stable: ties keep r, g, b order, any order gives the same value)
        fs = [1.0] + [f[a] for a in axes] + [0.0]
        pos = i.copy()
        acc = (fs[0] - fs[1]) * lut[pos[2], pos[1], pos[0]]
        for j, a in enumerate(axes):
            pos[a] += 1
            acc = acc + (fs[j + 1] - fs[j + 2]) * lut[pos[2], pos[1], pos[0]]
        out[k] = acc
    return out.reshape(np.shape(m))


def grade(x, rows, lut=None, dtype=np.float64, variant=None):
    """x [B, 3, H, W] float32, rows [B, >= 24] float32, lut [N, N, N, 3] float32 or None -> y [B, 3, H, W] of ``dtype``.  Identity rows pass
    x through (as ``dtype``; for float32 the very bits)."""
    x = np.asarray(x, F32)
    rows = np.asarray(rows, F32)
    assert x.ndim == 4 and x.shape[1] == 3 and rows.shape[0] == x.shape[0] and rows.shape[1] >= ROW
    ident = is_identity(rows, lut is not None)
    out = np.empty(x.shape, dtype)
    half, one, two = dtype(0.5), dtype(1), dtype(2)
    for b in range(x.shape[0]):
        if ident[b]:
            out[b] = x[b] if dtype == F32 else x[b].astype(dtype)
            continue
        r = rows[b].astype(dtype)
        px = np.moveaxis(x[b], 0, -1).astype(dtype)  # [H, W, 3]
        v = clamp01(px * half + half)
        if variant == "power_first":
            v = np.stack([v[..., c] if r[POWER + c] == 1 else _pow(v[..., c], r[POWER + c], dtype) for c in range(3)], axis=-1)
        t = clamp01(v * r[SLOPE:SLOPE + 3] + r[OFFSET:OFFSET + 3])
        if variant != "power_first":
            t = np.stack([t[..., c] if r[POWER + c] == 1 else _pow(t[..., c], r[POWER + c], dtype) for c in range(3)], axis=-1)
        mat = r[MATRIX:MATRIX + 9].reshape(3, 3)
        if variant == "transposed":
            mat = mat.T
        m = np.stack([((mat[c, 0] * t[..., 0] + mat[c, 1] * t[..., 1]) + mat[c, 2] * t[..., 2]) + r[BIAS + c] for c in range(3)], axis=-1)
        m = clamp01(m)
        if lut is not None and r[MIX] != 0:
            l = trilinear(lut, m, dtype) if variant == "trilinear" else tetra(lut, m, dtype)
            m = clamp01(m + r[MIX] * (l - m))
        y = m * two - one
        assert y.dtype == dtype
        out[b] = np.moveaxis(y, -1, 0)
    return out


def quant8(y):
    """maua_frames_to_u8 on [B, 3, H, W] float32 -> [B, H, W, 3] uint8."""
    y = np.asarray(y, F32)
    y = np.where(np.isnan(y), F32(-1), y).astype(F32)
    q = ((np.clip(y, F32(-1), F32(1)) + F32(1)) * F32(127.5)).astype(np.uint8)
    return np.ascontiguousarray(q.transpose(0, 2, 3, 1))


def pad_lut(lut):
    """[N, N, N, 3] -> the device layout [N^3, 4] float32: every entry padded to four floats."""
    lut = np.asarray(lut, F32)
    n = lut.shape[0]
    out = np.zeros((n ** 3, 4), F32)
    out[:, :3] = lut.reshape(-1, 3)
    return out


# ------------------------------------------------------------------------------------------------------------------------ case list
def sample_lut(n, seed=0):
    """A smooth but strongly non-linear table with a little seeded roughness: tetrahedral and trilinear interpolation differ on it."""
    g = np.linspace(0, 1, n)
    b, gg, r = np.meshgrid(g, g, g, indexing="ij")
    rng = np.random.default_rng(seed + n)
    table = np.stack([np.clip(r * gg + 0.3 * b, 0, 1), np.clip(gg ** 2 + 0.5 * r * b, 0, 1), np.clip(1 - (1 - b) * (1 - r * gg), 0, 1)], axis=-1)
    # (the roughness shrinks with the cell, so the table's slope — what multiplies a rounding error of m — stays about 2 for every n)
    return np.clip(table + rng.uniform(-0.2, 0.2, table.shape) / (n - 1), 0, 1).astype(F32)


def case_image(b, h, w, n_lut, seed, lo=-1.2):
    """[b, 3, h, w] float32 in about [lo, 1.2] with the special values planted where the shape has room: -1, 1, beyond, lattice points and
    cell boundaries of the n_lut lattice (as x = 2 k / (n - 1) - 1 and its float32 neighbours), NaN and the infinities."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(lo, 1.2, (b, 3, h, w)).astype(F32)
    special = [-1.0, 1.0, -1.5, 1.5, 0.0, np.nan, np.inf, -np.inf]
    if n_lut:
        k = np.arange(n_lut, dtype=np.float64)
        lattice = (2 * k / (n_lut - 1) - 1).astype(F32)
        special += list(lattice[:6]) + list(np.nextafter(lattice[:6], F32(2))) + list(np.nextafter(lattice[:6], F32(-2)))
    flat = x.reshape(-1)
    pos = rng.permutation(flat.size)[:min(len(special) * 3, max(flat.size // 3, 1))]
    flat[pos] = np.asarray(special * 3, F32)[:len(pos)]
    if b * h * w >= 4:  # whole pixels on the lattice, on a cell's diagonal and on its faces (ties in the comparison chain)
        n = n_lut or 5
        px = x.transpose(0, 2, 3, 1).reshape(-1, 3)
        px[0] = 2 * np.array([1, 2, 0], np.float64) / max(n - 1, 1) - 1
        px[1] = F32(0.25)
        px[2] = (F32(0.25), F32(0.25), F32(-0.5))
        px[3] = (F32(-0.5), F32(0.25), F32(0.25))
        x = np.ascontiguousarray(px.reshape(b, h, w, 3).transpose(0, 3, 1, 2))
    return x


def case_rows(kind, b, power=False, mix=1.0, seed=0):
    """float32 [b, 24]: ``kind`` "identity", "graded" (every frame another non-identity row) or "mixed" (identity rows between them)."""
    rng = np.random.default_rng(100 + seed)
    rows = np.empty((b, ROW), np.float64)
    for k in range(b):
        ident = kind == "identity" or (kind == "mixed" and k % 2 == 0)
        if ident:
            rows[k] = identity_row()
            rows[k, MIX] = 0.0 if kind == "mixed" else mix
            continue
        if power:  # (gentler: the power cases are compared with float64 under a tolerance, so they are kept well conditioned)
            rows[k] = make_row(exposure=rng.uniform(-0.3, 0.3), contrast=rng.uniform(0.9, 1.15), pivot=0.45, slope=rng.uniform(0.9, 1.1, 3),
                               offset=rng.uniform(-0.03, 0.03, 3), power=rng.uniform(0.6, 2.0, 3), saturation=rng.uniform(0.7, 1.3),
                               hue=rng.uniform(-30, 30), matrix=np.eye(3) + rng.uniform(-0.05, 0.05, (3, 3)), bias=rng.uniform(-0.03, 0.03, 3),
                               lut_mix=mix)
            continue
        rows[k] = make_row(exposure=rng.uniform(-0.7, 0.7), contrast=rng.uniform(0.7, 1.4), pivot=0.45, slope=rng.uniform(0.8, 1.2, 3),
                           offset=rng.uniform(-0.08, 0.08, 3), power=rng.uniform(0.5, 2.2, 3) if power else 1.0,
                           saturation=rng.uniform(0.3, 1.6), hue=rng.uniform(-60, 60), matrix=np.eye(3) + rng.uniform(-0.1, 0.1, (3, 3)),
                           bias=rng.uniform(-0.05, 0.05, 3), lut_mix=mix)
    if kind == "identity":
        rows[:, MIX] = 0.0
    return rows.astype(F32)


# (b, h, w): the issue's shapes; plane % 4 == 0 -> the vector path (16, 256, 4096, 4290 pixels), otherwise the scalar path (1, 3, 35)
SHAPES = [(1, 1, 1), (1, 1, 3), (2, 5, 7), (3, 16, 16), (1, 64, 64), (2, 33, 130)]
LUT_SIZES = (0, 2, 3, 17, 33)


def gpu_cases():
    """The GPU case list with power == 1 (bit-for-bit cases): dicts of shape, rows kind, LUT size (0: none), lut_mix, row stride, seed."""
    cases = []
    seed = 0
    for shape in SHAPES:
        for n_lut, mix in ((0, 1.0), (2, 1.0), (3, 0.5), (17, 1.0), (33, 0.5), (17, 0.0)):
            for kind in ("graded", "mixed"):
                seed += 1
                cases.append(dict(shape=shape, kind=kind, n_lut=n_lut, mix=mix, stride=24 if seed % 2 else 32, seed=seed))
    return cases


def power_cases():
    """The cases with power != 1 in the full chain (compared with float64 under ``allowance``)."""
    return [dict(shape=shape, kind="graded", n_lut=n_lut, mix=mix, stride=24, seed=1000 + k)
            for k, (shape, n_lut, mix) in enumerate([((2, 5, 7), 0, 1.0), ((3, 16, 16), 17, 1.0), ((1, 64, 64), 33, 0.5), ((2, 33, 130), 3, 1.0)])]


EPS32 = 2.0 ** -24
CEILING = 1e-5


def allowance(x, rows, lut):
    """allow = 4 max(err_f32, 16 * 2^-24) of the case itself, err_f32 = max |float32 emulation - float64 definition|: the device may differ
    from the definition by what the float32 arithmetic itself does on these inputs, times 4 for its powf (a few ulp where the emulation's
    is rounded once).  The cases are built so that allow stays under CEILING (tests/test_grade_host.py)."""
    err = float(np.max(np.abs(grade(x, rows, lut, F32).astype(np.float64) - grade(x, rows, lut, np.float64))))
    return 4.0 * max(err, 16 * EPS32), err


def pow_bound(t, p):
    """The bound on |y - (2 t^p - 1)| for y = fl(2 powf(t, p) - 1) with a powf within 16 ulp (what OpenCL allows pow), taken twice for the
    unknown direction of the rounding of t^p itself (2 x 16 ulp), doubled by the scaling, plus the rounding of the subtraction."""
    pw = np.power(t.astype(np.float64), np.float64(p))
    return 2 * 32 * np.spacing(pw.astype(F32)).astype(np.float64) + 0.5 * np.spacing(np.abs(2 * pw - 1).astype(F32)).astype(np.float64)


def build_case(case, power=False):
    """(x, rows [b, 24], lut or None) of a case."""
    b, h, w = case["shape"]
    x = case_image(b, h, w, case["n_lut"], case["seed"], lo=-0.8 if power else -1.2)
    rows = case_rows(case["kind"], b, power=power, mix=case["mix"], seed=case["seed"])
    lut = sample_lut(case["n_lut"], case["seed"]) if case["n_lut"] else None
    return x, rows, lut
