"""CPU: the coordinate-remap bends (maua_bend_remap_f32; audioreactive/bend.py: Mirror, Kaleidoscope, Swirl, Ripple, Displace) without
a device — the float64 reference of tests/remap_ref.py against torch's grid_sample, the error bound of the GPU tests (it accepts the
float32 stand-in everywhere and rejects six deliberate defects on every shape), the modules' validation and column rule, and the
entry's argument checks."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import remap_ref as rr

SHAPES = rr.SHAPES
REAL_SHAPES = [s for s in rr.SHAPES if s[2] > 1 and s[3] > 1]  # with a non-degenerate axis
ids = lambda s: "x".join(map(str, s))  # noqa: E731


def batch_rows(op, shape):
    rows = rr.device_rows(op, shape[2], shape[3])
    return rows[np.arange(shape[0]) % len(rows)]


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_reference_equals_grid_sample(shape):
    """remap64 == grid_sample(bilinear, reflection | border, align_corners=True) in float64 on the reference's own source coordinates."""
    b, c, h, w = shape
    x = rr.plain_map(shape)
    field = rr.field_bank()
    xt = torch.from_numpy(x).double()
    for op in range(5):
        rows = batch_rows(op, shape)
        grid = np.zeros((b, h, w, 2))
        for i in range(b):
            sx, sy = rr.coords64(op, h, w, rows[i], field)
            grid[i, ..., 0] = 2 * sx / (w - 1) - 1 if w > 1 else 0.0
            grid[i, ..., 1] = 2 * sy / (h - 1) - 1 if h > 1 else 0.0
        for border, mode in ((rr.REFLECT, "reflection"), (rr.CLAMP, "border")):
            want = F.grid_sample(xt, torch.from_numpy(grid), mode="bilinear", padding_mode=mode, align_corners=True).numpy()
            got, _, _ = rr.remap64(x, op, border, rows, field)
            err = float(np.abs(got - want).max())
            assert err < 1e-10, (rr.OP_NAMES[op], mode, err)


@pytest.mark.parametrize("shape", SHAPES, ids=ids)
def test_bound_accepts_the_float32_stand_in_everywhere(shape):
    x = rr.plain_map(shape)
    field = rr.field_bank()
    for op in range(5):
        rows = batch_rows(op, shape)
        for border in (rr.REFLECT, rr.CLAMP):
            delta = rr.coordinate_allowance(op, shape, border, rows, field)
            want, fsx, fsy = rr.remap64(x, op, border, rows, field)
            got = rr.remap32(x, op, border, rows, field)[0]
            limit = rr.bound(x, fsx, fsy, delta)
            excess = np.abs(got - want) - limit
            print(f"[{rr.OP_NAMES[op]} {ids(shape)} border {border}] delta {delta:.2e} px, max error {np.abs(got - want).max():.2e}, "
                  f"largest error / bound {float((np.abs(got - want) / np.maximum(limit, 1e-300)).max()):.3f}")
            assert delta < 0.01, "the parameter sets are chosen so that float32 coordinates are good to a hundredth of a pixel"
            assert bool((excess <= 0).all()), (rr.OP_NAMES[op], border, float(excess.max()))


# defect -> the ops whose parameter sets expose it (period 2n: only where coordinates leave the map, under the reflecting border)
DEFECT_OPS = {"half pixel": range(5), "period 2n": (rr.MIRROR, rr.DISPLACE), "swapped weights": range(5),
              "sectors + 1": (rr.KALEIDOSCOPE,), "field frame + 1": (rr.DISPLACE,),
              "degrees as radians": (rr.MIRROR, rr.KALEIDOSCOPE, rr.SWIRL)}


@pytest.mark.parametrize("defect", rr.DEFECTS)
@pytest.mark.parametrize("shape", REAL_SHAPES, ids=ids)
def test_bound_rejects_the_defect(shape, defect):
    b, c, h, w = shape
    x = rr.plain_map(shape)
    field = rr.field_bank()
    for op in DEFECT_OPS[defect]:
        rows = batch_rows(op, shape)
        for border in (rr.REFLECT,) if defect == "period 2n" else (rr.REFLECT, rr.CLAMP):
            delta = rr.coordinate_allowance(op, shape, border, rows, field)
            want, fsx, fsy = rr.remap64(x, op, border, rows, field)
            if defect == "degrees as radians":
                wrong = rr.rows_from_degrees(op, rr.public_rows(op, h, w), as_radians=True)
                got = rr.remap64(x, op, border, wrong[np.arange(b) % len(wrong)], field)[0]
            else:
                got = rr.remap64(x, op, border, rows, field, defect=defect)[0]
            out = int((np.abs(got - want) > rr.bound(x, fsx, fsy, delta)).sum())
            assert out >= 1, f"{defect} on {rr.OP_NAMES[op]} (border {border}) stays inside the bound on every element"


def test_reference_known_answers():
    """The identities the GPU test asserts bit for bit hold in the float32 stand-in, and pass-through rules in both references."""
    field = np.zeros((3, 2, 2, 2), np.float32)
    field[:, 0], field[:, 1] = 2.0, -1.0
    for shape in [(2, 3, 5, 7), (1, 2, 4, 8), (1, 1, 33, 65)]:
        x = rr.plain_map(shape, "known")
        b, c, h, w = shape
        for border in (rr.REFLECT, rr.CLAMP):
            for op, row in ((rr.SWIRL, [0, 3.5, 0, 0]), (rr.RIPPLE, [0, 2.5, 0.3, 0]), (rr.DISPLACE, [0, 1.25, 0, 0])):
                assert np.array_equal(rr.remap32(x, op, border, np.array([row] * b, np.float32), field)[0], x)
            flipped = rr.remap32(x, rr.MIRROR, border, np.array([[0, 1, 0, 0]] * b, np.float32))[0]
            assert np.array_equal(flipped[:, :, : h // 2], x[:, :, ::-1][:, :, : h // 2]) and np.array_equal(flipped[:, :, h // 2:], x[:, :, h // 2:])
            shifted = rr.remap32(x, rr.DISPLACE, border, np.array([[1, 3.0, 0, 0]] * b, np.float32), field)[0]  # position F wraps to 0
            xs, ys = np.arange(w) + 2, np.arange(h) - 1
            if border == rr.REFLECT:
                fold = lambda i, n: np.where(np.mod(i, 2 * (n - 1)) > n - 1, 2 * (n - 1) - np.mod(i, 2 * (n - 1)), np.mod(i, 2 * (n - 1)))  # noqa: E731
                xs, ys = fold(xs, w), fold(ys, h)
            else:
                xs, ys = np.clip(xs, 0, w - 1), np.clip(ys, 0, h - 1)
            assert np.array_equal(shifted, x[:, :, ys][:, :, :, xs])
            for op, row in ((rr.SWIRL, [1, 0, 0, 0]), (rr.RIPPLE, [1, -2, 0, 0]), (rr.MIRROR, [math.nan, 1, 0, 0]),
                            (rr.KALEIDOSCOPE, [6, math.inf, 0, 0]), (rr.DISPLACE, [1, math.nan, 0, 0])):
                bad = np.array([row] * b, np.float32)
                assert rr.bad_row(op, bad[0])
                assert np.array_equal(rr.remap32(x, op, border, bad, field)[0], x) and np.array_equal(rr.remap64(x, op, border, bad, field)[0], x)
    assert not rr.bad_row(rr.SWIRL, [1, 2, math.nan, math.nan]) and not rr.bad_row(rr.DISPLACE, [1, 2, math.inf, 0])  # unused columns


# ------------------------------------------------------------------------------------------------------------------ the modules
NAMES = ("Mirror", "Kaleidoscope", "Swirl", "Ripple", "Displace")


def test_the_five_bends_are_exported_and_capturable():
    import maua_stylegan2_amd.audioreactive as ar
    from maua_stylegan2_amd import render

    n = 12
    env = torch.linspace(0.0, 30.0, n)
    field = torch.from_numpy(rr.field_bank())
    for name in NAMES:
        assert issubclass(getattr(ar, name), ar.NetworkBend), name
    assert issubclass(ar.RemapBend, torch.nn.Module)
    bends = [{"layer": 2, "modulation": env, "transform": lambda m: ar.Mirror(m, offset=1.0)},
             {"layer": 3, "modulation": env, "transform": lambda m: ar.Kaleidoscope(m, sectors=5, channels=[0, 2])},
             {"layer": 4, "modulation": env, "transform": lambda m: ar.Swirl(m, radius=6.0, channels=[1], border="clamp")},
             {"layer": 5, "modulation": env, "transform": lambda m: ar.Ripple(m, wavelength=4.0)},
             {"layer": 6, "modulation": torch.stack([env, 0.25 * torch.arange(n)], 1), "transform": lambda m: ar.Displace(m, field)}]
    seq, ok = render._sequence_bends(bends, n)
    assert ok and [b["transform"].sequence_rows for b in seq] == [n] * 5
    for b in seq:
        t = b["transform"]
        assert t.capturable and hasattr(t.sequential, "run_static") and tuple(t.sequential.table.shape) == (n, 4)
    assert [b["transform"].sequential.op for b in seq] == [0, 1, 2, 3, 4]
    assert [b["transform"].sequential.border for b in seq] == [0, 0, 1, 0, 0]
    for bend in bends:  # a table of another length than the sequence never reaches a captured forward
        assert render._sequence_bends([bend], n + 1) == (None, False)
    assert ar.Swirl(env[:1], radius=3.0).sequence_rows == 1


def test_column_rule_and_units():
    """[n] is the first parameter, [n, k] the first k in the op's order; the others come from the keywords; angles arrive in degrees and
    leave as radians (the mirror's as a unit normal)."""
    import maua_stylegan2_amd.audioreactive as ar

    n = 5
    a = torch.tensor([0.0, 30.0, 90.0, 180.0, -45.0])
    rad = torch.deg2rad(a)
    col = torch.linspace(1.0, 3.0, n)
    zero = torch.zeros(n)

    def table(bend):
        return bend.sequential.table

    def same(t, *cols):
        return torch.allclose(t, torch.stack(list(cols) + [zero] * (4 - len(cols)), 1), rtol=0, atol=1e-6)

    assert same(table(ar.Mirror(a)), torch.cos(rad), torch.sin(rad), zero)
    assert same(table(ar.Mirror(a, offset=2.5)), torch.cos(rad), torch.sin(rad), zero + 2.5)
    assert same(table(ar.Mirror(torch.stack([a, col], 1), offset=2.5)), torch.cos(rad), torch.sin(rad), col)  # the column wins
    assert same(table(ar.Kaleidoscope(a)), zero + 6, zero, rad)
    assert same(table(ar.Kaleidoscope(a, angle=90.0, sectors=3)), zero + 3, zero + math.pi / 2, rad)
    assert same(table(ar.Kaleidoscope(torch.stack([a, a, col.round()], 1))), col.round(), rad, rad)
    assert same(table(ar.Swirl(a, radius=7.0)), rad, zero + 7)
    assert same(table(ar.Swirl(torch.stack([a, col], 1))), rad, col)
    assert same(table(ar.Ripple(col, wavelength=4.0)), col, zero + 4, zero)
    assert same(table(ar.Ripple(torch.stack([col, col + 1], 1), phase=0.5)), col, col + 1, zero + 0.5)
    assert same(table(ar.Ripple(torch.stack([col, col + 1, a], 1))), col, col + 1, a)
    field = torch.zeros(3, 2, 4, 4)
    assert same(table(ar.Displace(col, field)), col, zero)
    assert same(table(ar.Displace(col, field, position=1.5)), col, zero + 1.5)
    assert same(table(ar.Displace(torch.stack([col, a], 1), field)), col, a)
    assert ar.Displace(col, field).sequential.field.shape == (3, 2, 4, 4) and ar.Swirl(a, radius=1.0).sequential.field is None
    sub = ar.Swirl(a, radius=2.0, channels=[1, 3]).sequential
    assert sub.channels.tolist() == [1, 3] and sub._channel_mask(4).tolist() == [0, 1, 0, 1]
    # the table agrees with the reference helper's conversion
    pub = rr.public_rows(rr.KALEIDOSCOPE, 16, 16)
    t = table(ar.Kaleidoscope(torch.from_numpy(pub[:, [2, 1, 0]]).float()))
    assert np.allclose(t.numpy(), rr.rows_from_degrees(rr.KALEIDOSCOPE, pub), rtol=0, atol=1e-6)


def test_constructor_validation():
    import maua_stylegan2_amd.audioreactive as ar

    n = 4
    ok = torch.ones(n)
    nan = torch.tensor([0.0, float("nan"), 1.0, 2.0])
    inf = torch.tensor([0.0, float("inf"), 1.0, 2.0])
    field = torch.zeros(2, 2, 3, 3)
    for make in (lambda m: ar.Mirror(m), lambda m: ar.Kaleidoscope(m), lambda m: ar.Swirl(m, radius=2.0),
                 lambda m: ar.Ripple(m, wavelength=2.0), lambda m: ar.Displace(m, field)):
        for bad in (nan, inf):
            with pytest.raises(ValueError, match="NaN"):
                make(bad)
        with pytest.raises(ValueError, match="modulation"):
            make(torch.ones(n, 5))
        with pytest.raises(ValueError, match="modulation"):
            make(torch.tensor(1.0))
        with pytest.raises(ValueError, match="modulation"):
            make(torch.ones(n, 2, 2))
    with pytest.raises(ValueError, match="NaN"):
        ar.Mirror(ok, offset=float("nan"))
    for sectors in (0, 65, -3, 0.4):
        with pytest.raises(ValueError, match="sectors"):
            ar.Kaleidoscope(ok, sectors=sectors)
    with pytest.raises(ValueError, match="sectors"):
        ar.Kaleidoscope(torch.stack([ok, ok, torch.tensor([1.0, 2.0, 70.0, 3.0])], 1))
    ar.Kaleidoscope(ok, sectors=1), ar.Kaleidoscope(ok, sectors=64), ar.Kaleidoscope(ok, sectors=64.4)
    for radius in (0.0, -1.0):
        with pytest.raises(ValueError, match="radius"):
            ar.Swirl(ok, radius=radius)
        with pytest.raises(ValueError, match="wavelength"):
            ar.Ripple(ok, wavelength=radius)
    with pytest.raises(ValueError, match="radius"):
        ar.Swirl(ok)  # neither a column nor the keyword
    with pytest.raises(ValueError, match="wavelength"):
        ar.Ripple(ok)
    with pytest.raises(ValueError, match="radius"):
        ar.Swirl(torch.stack([ok, torch.tensor([1.0, 0.0, 1.0, 1.0])], 1))
    for bad_field in (torch.zeros(2, 3, 3), torch.zeros(2, 3, 4, 4), torch.zeros(2, 2, 0, 4), torch.zeros(2, 1, 2, 4, 4)):
        with pytest.raises(ValueError, match="field"):
            ar.Displace(ok, bad_field)
    with pytest.raises(ValueError, match="field"):
        ar.Displace(ok, torch.full((2, 2, 3, 3), float("nan")))
    with pytest.raises(ValueError, match="border"):
        ar.Swirl(ok, radius=1.0, border="wrap")
    with pytest.raises(ValueError):
        ar.RemapBend("twist", torch.zeros(n, 4), None)
    with pytest.raises(ValueError, match="parameters"):
        ar.RemapBend("swirl", torch.ones(n, 3), None)
    with pytest.raises(ValueError, match="field"):
        ar.RemapBend("swirl", torch.ones(n, 4), None, field=field)
    with pytest.raises(ValueError, match="field"):
        ar.RemapBend("displace", torch.ones(n, 4), None)
    with pytest.raises(RuntimeError, match="channels"):
        ar.RemapBend("swirl", torch.ones(n, 4), [0, 8], n_channels=8)
    assert not any(hasattr(ar, name) for name in ("REMAP_OPS", "REMAP_BORDERS", "MAX_SECTORS"))


# ------------------------------------------------------------------------------------------------------------------ the entry
def test_header_binding_and_library_agree(built_lib):
    import ctypes
    import os
    import re

    from conftest import REPO
    from maua_stylegan2_amd import _lib
    from maua_stylegan2_amd.audioreactive import bend

    text = open(os.path.join(REPO, "include", "maua_hip.h")).read()
    assert re.search(r"#define\s+MAUA_BEND_REMAP_PARAMS\s+4\b", text) and bend._REMAP_PARAMS == 4
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    decl = re.search(r"\bint\s+maua_bend_remap_f32\s*\(([^)]*)\)", code)
    assert decl and len(decl.group(1).split(",")) == 17
    assert "maua_bend_remap_f32" in _lib.exported_symbols() and len(_lib._SIGNATURES["maua_bend_remap_f32"][1]) == 17
    lib = ctypes.CDLL(built_lib)
    assert hasattr(lib, "maua_bend_remap_f32")
    lib.maua_abi_version.restype = ctypes.c_int
    assert lib.maua_abi_version() == 8 == _lib.ABI_VERSION  # additive: the version stays


def test_entry_rejects_bad_arguments_without_gpu(built_lib):
    """Argument validation runs before any HIP call."""
    from maua_stylegan2_amd import _lib

    lib = _lib.load()
    fake, fake2, fake3, fake4 = 0x1000, 0x2000, 0x3000, 0x4000  # never dereferenced: every call below is refused

    def remap(x=fake, y=fake2, batch=2, channels=4, h=4, w=4, op=2, border=0, param=fake3, rows=2, field=None, frames=0, fh=0, fw=0,
              src=None):
        return lib.maua_bend_remap_f32(x, y, batch, channels, h, w, op, border, param, rows, field, frames, fh, fw, None, src, None)

    assert remap(x=None) == -22 and remap(y=None) == -22 and remap(param=None) == -22
    assert remap(y=fake) == -22                                                 # in place: a gather cannot be
    assert remap(batch=0) == -22 and remap(batch=65) == -22 and remap(batch=-1) == -22
    assert remap(channels=0) == -22 and remap(channels=65536) == -22
    assert remap(h=0) == -22 and remap(w=0) == -22 and remap(w=-3) == -22
    assert remap(h=1 << 15, w=1 << 14) == -22                                   # a plane of 2 GiB
    assert remap(op=-1) == -22 and remap(op=5) == -22 and remap(border=-1) == -22 and remap(border=2) == -22
    assert remap(rows=0) == -22 and remap(rows=-2) == -22 and remap(rows=3) == -22  # without a frame source: one row, or one per sample
    assert remap(op=4) == -22                                                   # displace without a field
    assert remap(op=4, field=fake4, frames=0, fh=2, fw=2) == -22 and remap(op=4, field=fake4, frames=2, fh=0, fw=2) == -22
    assert remap(op=4, field=fake4, frames=2, fh=2, fw=-1) == -22 and remap(op=4, field=None, frames=2, fh=2, fw=2) == -22
    assert remap(op=4, field=fake4, frames=1, fh=1 << 15, fw=1 << 14) == -22
