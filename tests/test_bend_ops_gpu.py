"""GPU: maua_bend_point_f32 and maua_bend_morph_f32 (include/maua_hip.h, csrc/bend_ops.hip) through the C ABI against torch's CPU ops.
Every op is exact in fp32, so the comparison is ``torch.equal`` (values, not bit patterns: -0 and +0 tie in a maximum): ablate 0, invert
1 - x, scalar multiply x * p, binary threshold x > p, erode -max_pool2d(-x, 2r + 1, 1, r), dilate max_pool2d(x, 2r + 1, 1, r).  Red zones
(tests/redzone.py) round every buffer of both entries; the Python modules of audioreactive/bend.py on top."""
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from maua_stylegan2_amd import seeding
from redzone import Guard

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

SHAPES = [(1, 3, 1, 1), (2, 5, 5, 7), (8, 32, 4, 8), (3, 16, 33, 65), (1, 8, 256, 256)]
SUBSETS = ("none", "empty", "all", "third")
MAX_RADIUS = 16
FRAME0 = 3


def lib():
    from maua_stylegan2_amd import _lib

    return _lib.load()


def stream(dev):
    from maua_stylegan2_amd import _lib

    return _lib.stream_ptr(dev)


def frame_source(dev, frame0):
    """A maua_frame_source_t in device memory that holds nothing but the frame a launch starts at."""
    from maua_stylegan2_amd import _lib

    fs = _lib.FrameSource()
    fs.frame0 = frame0
    return torch.frombuffer(bytearray(bytes(fs)), dtype=torch.uint8).to(dev)


def feature_map(shape, tag="x"):
    """Seeded N(0,1) map with ties (values rounded to 1/4), zeros of both signs and a few large values."""
    x = torch.from_numpy(seeding.seeded_array(41, f"{tag}{shape}", shape)).float()
    flat = x.view(-1)
    flat[::3] = torch.round(flat[::3] * 4) / 4
    flat[::7] = 0.0
    flat[3::14] = -0.0
    flat[5::31] *= 1e6
    return x


def selection(kind, c):
    """Boolean [c] selection, or None for a NULL mask."""
    if kind == "none":
        return None
    sel = torch.zeros(c, dtype=torch.bool)
    if kind == "all":
        sel[:] = True
    elif kind == "third":
        sel[::3] = True
    return sel


def apply_selection(x, full, sel):
    if sel is None:
        return full
    out = x.clone()
    out[:, sel] = full[:, sel]
    return out


def point_full(x, op, p):
    p = p.view(-1, 1, 1, 1)
    return [torch.zeros_like(x), 1 - x, x * p, (x > p).float()][op]


def morph_full(x, op, radii):
    out = torch.empty_like(x)
    for b, r in enumerate(radii):
        r = min(max(int(r), 0), MAX_RADIUS)  # the device clamps
        xb = x[b: b + 1]
        out[b: b + 1] = F.max_pool2d(xb, 2 * r + 1, 1, r) if op == 1 else -F.max_pool2d(-xb, 2 * r + 1, 1, r)
    return out


def parameter_modes(batch, values):
    """(name, table, rows, frame0 or None, per-sample values): one row; one row per sample; a longer sequence read through a frame
    source at frame0 > 0 (the rows before and after the batch hold other values)."""
    per_sample = [values[(2 * b + 1) % len(values)] for b in range(batch)]
    sequence = [values[(b + 2) % len(values)] for b in range(FRAME0)] + per_sample[::-1] + [values[0], values[-1]]
    modes = [("per-sample", per_sample, batch, None, per_sample),
             ("frame source", sequence, len(sequence), FRAME0, per_sample[::-1])]
    return modes + [(f"one row ({v})", [v], 1, None, [v] * batch) for v in values]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_point_ops_equal_torch(gpu, shape):
    b, c, h, w = shape
    x = feature_map(shape)
    xd = x.to(gpu)
    thresholds = [0.0, 0.25, -0.5, float(x.view(-1)[1])]  # ties: x > p is strict
    launches = 0
    for op in range(4):
        modes = parameter_modes(b, thresholds if op == 3 else [0.0, 1.0, -2.5, 0.3])
        if op < 2:
            modes = modes[:1]  # no parameter: the table is ignored (and NULL below)
        for name, table, rows, frame0, per_sample in modes:
            full = point_full(x, op, torch.tensor(per_sample))
            td = torch.tensor(table, dtype=torch.float32, device=gpu) if op >= 2 else None
            src = frame_source(gpu, frame0) if frame0 is not None else None
            for kind in SUBSETS:
                sel = selection(kind, c)
                want = apply_selection(x, full, sel)
                mask = None if sel is None else sel.to(torch.uint8).to(gpu)
                for in_place in (False, True):
                    xin = xd.clone()
                    y = xin if in_place else torch.full_like(xd, float("nan"))
                    rc = lib().maua_bend_point_f32(xin.data_ptr(), y.data_ptr(), b, c, h * w, op, None if td is None else td.data_ptr(),
                                                   rows, None if mask is None else mask.data_ptr(),
                                                   None if src is None else src.data_ptr(), stream(gpu))
                    assert rc == 0
                    assert torch.equal(y.cpu(), want), (op, name, kind, in_place)
                    assert in_place or torch.equal(xin, xd)
                    launches += 1
    assert launches == (1 + 1 + 6 + 6) * 4 * 2


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_morph_ops_equal_max_pool2d(gpu, shape):
    b, c, h, w = shape
    x = feature_map(shape)
    xd = x.to(gpu)
    radii = [0, 1, 3, 16, 40, -2]  # 16 >= the side of the three small maps; 40 (>= every side but 256) and -2 are clamped on the device
    full = functools.lru_cache(maxsize=None)(lambda op, rs: morph_full(x, op, rs))
    launches = 0
    for op in (0, 1):
        for name, table, rows, frame0, per_sample in parameter_modes(b, radii):
            td = torch.tensor(table, dtype=torch.int32, device=gpu)
            src = frame_source(gpu, frame0) if frame0 is not None else None
            for kind in SUBSETS:
                sel = selection(kind, c)
                want = apply_selection(x, full(op, tuple(per_sample)), sel)
                mask = None if sel is None else sel.to(torch.uint8).to(gpu)
                y = torch.full_like(xd, float("nan"))
                rc = lib().maua_bend_morph_f32(xd.data_ptr(), y.data_ptr(), b, c, h, w, op, td.data_ptr(), rows,
                                               None if mask is None else mask.data_ptr(), None if src is None else src.data_ptr(),
                                               stream(gpu))
                assert rc == 0
                assert torch.equal(y.cpu(), want), (op, name, kind)
                launches += 1
    assert launches == 2 * 8 * 4
    assert torch.equal(xd.cpu(), x)


def test_radius_zero_is_the_identity_and_growth_is_monotone(gpu):
    x = feature_map((2, 4, 19, 23), "mono")
    xd = x.to(gpu)

    def run(op, r):
        y = torch.empty_like(xd)
        rd = torch.tensor([r], dtype=torch.int32, device=gpu)
        assert lib().maua_bend_morph_f32(xd.data_ptr(), y.data_ptr(), 2, 4, 19, 23, op, rd.data_ptr(), 1, None, None, stream(gpu)) == 0
        return y.cpu()

    assert torch.equal(run(0, 0), x) and torch.equal(run(1, 0), x)
    for r in (1, 2, 5, 16):
        assert bool((run(1, r) >= run(1, r - 1)).all()) and bool((run(0, r) <= run(0, r - 1)).all())
    assert bool((run(1, 16)[:, :, 2:17, 6:17] == x.amax(dim=(2, 3), keepdim=True)).all())  # the window covers the whole map there


@pytest.mark.parametrize("op", [0, 1], ids=["erode", "dilate"])
def test_a_nan_stays_inside_the_windows_that_contain_it(gpu, op):
    shape, r, at = (1, 2, 40, 70), 2, (0, 1, 17, 64)  # (the window straddles the tile boundary at column 64)
    clean = feature_map(shape, "nan")
    x = clean.clone()
    x[at] = float("nan")
    rd = torch.tensor([r], dtype=torch.int32, device=gpu)

    def run(t):
        td, y = t.to(gpu), torch.empty(shape, device=gpu)
        assert lib().maua_bend_morph_f32(td.data_ptr(), y.data_ptr(), *shape, op, rd.data_ptr(), 1, None, None, stream(gpu)) == 0
        return y.cpu()

    got, ref = run(x), run(clean)
    inside = torch.zeros(shape, dtype=torch.bool)
    inside[at[0], at[1], at[2] - r: at[2] + r + 1, at[3] - r: at[3] + r + 1] = True
    assert int(inside.sum()) == (2 * r + 1) ** 2
    assert bool(torch.isnan(got[inside]).all()), "every window that contains the NaN must give NaN"
    assert torch.equal(got[~inside], ref[~inside]), "outputs whose window does not contain the NaN must not change"
    want = morph_full(x, op, [r])
    assert torch.equal(torch.isnan(got), torch.isnan(want)) and torch.equal(got[~inside], want[~inside])
    # the point ops: a NaN stays in its element; it compares false in the threshold
    y = torch.empty(shape, device=gpu)
    p = torch.tensor([0.5], device=gpu)
    for pop in range(4):
        assert lib().maua_bend_point_f32(x.to(gpu).data_ptr(), y.data_ptr(), shape[0], shape[1], shape[2] * shape[3], pop, p.data_ptr(), 1,
                                         None, None, stream(gpu)) == 0
        want = point_full(x, pop, torch.tensor([0.5]))
        assert torch.equal(torch.nan_to_num(y.cpu(), nan=123.0), torch.nan_to_num(want, nan=123.0)), pop


ODD = (3, 8, 33, 65)  # (8 channels: a uint8 window of tests/redzone.py holds whole dwords, so the mask's red zone starts at its end)


@pytest.mark.parametrize("in_place", [False, True], ids=["out-of-place", "in-place"])
@pytest.mark.parametrize("op", range(4), ids=["ablate", "invert", "multiply", "threshold"])
def test_point_entry_red_zones(gpu, op, in_place):
    b, c, h, w = ODD
    x = feature_map(ODD, "rz")
    guard = Guard(gpu)
    param = guard.inp(torch.linspace(-1.0, 1.0, FRAME0 + b), "param")
    mask = guard.inp(selection("third", c).to(torch.uint8), "mask", torch.uint8)
    src = frame_source(gpu, FRAME0)
    if in_place:
        xw = guard.out(ODD, "y")
        xw.copy_(x)
        yw = xw
    else:
        xw, yw = guard.inp(x, "x"), guard.out(ODD, "y")
    rc = lib().maua_bend_point_f32(xw.data_ptr(), yw.data_ptr(), b, c, h * w, op, param.data_ptr(), FRAME0 + b, mask.data_ptr(),
                                   src.data_ptr(), stream(gpu))
    assert rc == 0
    guard.check(written=("y",))
    want = apply_selection(x, point_full(x, op, torch.linspace(-1.0, 1.0, FRAME0 + b)[FRAME0:]), selection("third", c))
    assert torch.equal(yw.cpu(), want)


@pytest.mark.parametrize("radius", [0, 1, 16])
@pytest.mark.parametrize("op", [0, 1], ids=["erode", "dilate"])
def test_morph_entry_red_zones(gpu, op, radius):
    b, c, h, w = ODD
    x = feature_map(ODD, "rz")
    guard = Guard(gpu)
    radii = [5] * FRAME0 + [radius, 2, radius]
    rd = guard.inp(torch.tensor(radii), "radius", torch.int32)
    mask = guard.inp(selection("third", c).to(torch.uint8), "mask", torch.uint8)
    src = frame_source(gpu, FRAME0)
    xw, yw = guard.inp(x, "x"), guard.out(ODD, "y")
    rc = lib().maua_bend_morph_f32(xw.data_ptr(), yw.data_ptr(), b, c, h, w, op, rd.data_ptr(), len(radii), mask.data_ptr(),
                                   src.data_ptr(), stream(gpu))
    assert rc == 0
    guard.check(written=("y",))
    assert torch.equal(yw.cpu(), apply_selection(x, morph_full(x, op, radii[FRAME0:]), selection("third", c)))
    assert torch.equal(xw.cpu(), x)


def test_rejected_arguments_launch_nothing(gpu):
    b, c, h, w = 2, 3, 5, 7
    guard = Guard(gpu)
    x = guard.inp(feature_map((b, c, h, w), "rej"), "x")
    y = guard.out((b, c, h, w), "y")
    p = guard.inp(torch.ones(b), "param")
    rd = guard.inp(torch.ones(b), "radius", torch.int32)
    st = stream(gpu)
    point = lib().maua_bend_point_f32
    morph = lib().maua_bend_morph_f32
    X, Y, P, R = x.data_ptr(), y.data_ptr(), p.data_ptr(), rd.data_ptr()
    assert point(None, Y, b, c, h * w, 0, None, 0, None, None, st) == -22 and point(X, None, b, c, h * w, 0, None, 0, None, None, st) == -22
    assert point(X, Y, 0, c, h * w, 0, None, 0, None, None, st) == -22 and point(X, Y, 65, c, h * w, 0, None, 0, None, None, st) == -22
    assert point(X, Y, b, 0, h * w, 0, None, 0, None, None, st) == -22 and point(X, Y, b, c, 0, 0, None, 0, None, None, st) == -22
    assert point(X, Y, b, c, h * w, 4, P, b, None, None, st) == -22 and point(X, Y, b, c, h * w, -1, P, b, None, None, st) == -22
    assert point(X, Y, b, c, h * w, 2, None, 0, None, None, st) == -22 and point(X, Y, b, c, h * w, 3, None, 0, None, None, st) == -22
    assert point(X, Y, b, c, h * w, 2, P, 0, None, None, st) == -22 and point(X, Y, b, c, h * w, 2, P, b + 1, None, None, st) == -22
    assert morph(None, Y, b, c, h, w, 0, R, b, None, None, st) == -22 and morph(X, None, b, c, h, w, 0, R, b, None, None, st) == -22
    assert morph(X, X, b, c, h, w, 0, R, b, None, None, st) == -22, "the morphological entry has no in-place form"
    assert morph(X, Y, b, c, h, w, 0, None, b, None, None, st) == -22 and morph(X, Y, b, c, h, w, 2, R, b, None, None, st) == -22
    assert morph(X, Y, 0, c, h, w, 0, R, b, None, None, st) == -22 and morph(X, Y, b, c, 0, w, 0, R, b, None, None, st) == -22
    assert morph(X, Y, b, c, h, -1, 0, R, b, None, None, st) == -22 and morph(X, Y, b, c, h, w, 0, R, 0, None, None, st) == -22
    assert morph(X, Y, b, c, h, w, 0, R, b + 1, None, None, st) == -22
    assert guard.untouched("y")
    guard.check()


def test_modules_eager_and_static_forms(gpu):
    """PointBend / MorphBend and the six NetworkBend classes: ``forward`` on a batch (one row, or rows cut to the batch), ``run_static``
    on the whole sequence through a frame source; operands are uploaded once and reused; channels are validated at first use."""
    import maua_stylegan2_amd.audioreactive as ar

    n, b, c, h, w = 9, 4, 12, 16, 32
    x = feature_map((b, c, h, w), "mod")
    xd = x.to(gpu)
    idx = [1, 4, 5, 11]
    sel = torch.zeros(c, dtype=torch.bool)
    sel[idx] = True
    env = torch.linspace(-1.0, 2.0, n)
    radii = torch.tensor([0.2, 1.4, 2.5, 0.6, 3.0, 16.0, 0.0, 1.0, 2.0])
    gate = torch.tensor([0.0, 1.0, 0.6, 0.4, 1.0, 0.0, 0.0, 1.0, 1.0])
    r_int = torch.round(radii).int().tolist()
    cases = [(lambda m: ar.ScalarMultiply(m, channels=idx), env, lambda t, m: t * m.view(-1, 1, 1, 1)),
             (lambda m: ar.BinaryThreshold(m, channels=torch.tensor(idx)), env, lambda t, m: (t > m.view(-1, 1, 1, 1)).float()),
             (lambda m: ar.Ablate(m, channels=idx), gate, lambda t, m: t * (m <= 0.5).float().view(-1, 1, 1, 1)),
             (lambda m: ar.Dilate(m, channels=idx), radii, lambda t, m: morph_full(t, 1, torch.round(m).int().tolist())),
             (lambda m: ar.Erode(m, channels=idx), radii, lambda t, m: morph_full(t, 0, torch.round(m).int().tolist()))]
    src = frame_source(gpu, FRAME0)
    for make, mod, oracle in cases:
        eager = make(mod[FRAME0: FRAME0 + b].to(gpu))
        want = apply_selection(x, oracle(x, mod[FRAME0: FRAME0 + b]), sel)
        assert torch.equal(eager(xd).cpu(), want)
        one = make(mod[4:5].to(gpu))  # one row serves every sample
        assert torch.equal(one(xd).cpu(), apply_selection(x, oracle(x, mod[4:5].expand(b)), sel))
        whole = make(mod.to(gpu))
        assert whole.sequence_rows == n and whole.capturable
        out = torch.full_like(xd, float("nan"))
        assert whole.run_static(xd, out, src.data_ptr()) is out
        assert torch.equal(out.cpu(), want)
        held = dict(whole.sequential._dev)
        whole.run_static(xd, out, src.data_ptr())
        assert whole.sequential._dev.keys() == held.keys() and all(whole.sequential._dev[k] is v for k, v in held.items()), \
            "operands must be uploaded once"
        with pytest.raises(RuntimeError, match="parameter rows"):
            make(mod[:b + 1].to(gpu))(xd)
    assert r_int[2] == 2  # (2.5 rounds to even)
    for static, oracle in ((ar.Invert(channels=idx), lambda t: 1 - t), (ar.Ablate(channels=idx), torch.zeros_like),
                           (ar.Invert(), lambda t: 1 - t)):
        want = apply_selection(x, oracle(x), sel if static.sequential.channels is not None else None)
        assert torch.equal(static(xd).cpu(), want)
        out = torch.full_like(xd, float("nan"))
        static.run_static(xd, out, src.data_ptr())
        assert torch.equal(out.cpu(), want)
    # one static instance on maps of two widths: both masks stay alive (a captured graph keeps reading the first)
    shared = ar.Invert(channels=idx)
    narrow = xd[:, :, :, :8].contiguous()  # same channels, another plane size: the same operands serve it
    wide = torch.cat([xd, xd], 1)
    first = shared.sequential._operands(xd, per_frame=False)
    assert torch.equal(shared(wide).cpu()[:, :c], apply_selection(x, 1 - x, sel)) and torch.equal(shared(wide).cpu()[:, c:], x)
    assert shared.sequential._operands(xd, per_frame=False)[1] is first[1] and len(shared.sequential._dev) == 2
    assert shared.sequential._operands(narrow, per_frame=False)[1] is first[1]
    for bad in (ar.Invert(channels=[0, c]), ar.Dilate(torch.ones(b), channels=[-1])):
        with pytest.raises(RuntimeError, match="channels"):
            bad(xd)
    from maua_stylegan2_amd import _lib
    with pytest.raises(RuntimeError, match="CUDA"):
        ar.Invert()(x)
    assert _lib.ABI_VERSION == 8
