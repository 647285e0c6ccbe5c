"""GPU: maua_bend_remap_f32 (include/maua_hip.h, csrc/bend_remap.hip) through the C ABI, red zones (tests/redzone.py) round x, y, param,
field and mask.  Bit-exact known answers (``torch.equal``) where fp32 arithmetic makes the remap an index permutation; everything else
against the float64 reference of tests/remap_ref.py computed from the same float32 parameter rows, every element held to
(Lx + Ly) delta + 8 * 2^-23 max|tap| with delta = 4 x the float32 stand-in's own coordinate deviation (remap_ref.coordinate_allowance:
computed here on the CPU per op, shape and parameter set, never from the device's output).  Unselected channels and bad rows are
compared with ``torch.equal``.  The Python modules of audioreactive/bend.py on top."""
import numpy as np
import pytest
import torch

import remap_ref as rr
from redzone import Guard

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

SUBSETS = ("none", "empty", "all", "third")
FRAME0 = 3
ids = lambda s: "x".join(map(str, s))  # noqa: E731


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


def parameter_modes(batch, values):
    """(name, table, frame0 or None, per-sample rows): one row; one row per sample; a longer sequence read through a frame source at
    frame0 > 0 (the rows before and after the batch hold other values)."""
    values = np.asarray(values, np.float32)
    per_sample = values[(2 * np.arange(batch) + 1) % len(values)]
    sequence = np.concatenate([values[(np.arange(FRAME0) + 2) % len(values)], per_sample[::-1], values[:1], values[-1:]])
    return [("one row", values[:1], None, np.repeat(values[:1], batch, 0)),
            ("per-sample", per_sample, None, per_sample),
            ("frame source", sequence, FRAME0, per_sample[::-1])]


def launch(guard, dev, xw, shape, op, border, table, frame0, field=None, mask=None, name="y"):
    """One guarded launch; returns the output window."""
    b, c, h, w = shape
    yw = guard.out(shape, name)
    src = frame_source(dev, frame0) if frame0 is not None else None
    fshape = (0, 0, 0) if field is None else (field.shape[0], field.shape[2], field.shape[3])
    rc = lib().maua_bend_remap_f32(xw.data_ptr(), yw.data_ptr(), b, c, h, w, op, border, table.data_ptr(), table.shape[0],
                                   None if field is None else field.data_ptr(), *fshape, None if mask is None else mask.data_ptr(),
                                   None if src is None else src.data_ptr(), stream(dev))
    assert rc == 0, rc
    return yw


@pytest.mark.parametrize("op", range(5), ids=rr.OP_NAMES)
@pytest.mark.parametrize("shape", rr.SHAPES, ids=ids)
def test_remap_within_the_bound_of_the_float64_reference(gpu, shape, op):
    b, c, h, w = shape
    x = rr.plain_map(shape)
    field = rr.field_bank() if op == rr.DISPLACE else None
    values = rr.device_rows(op, h, w)
    launches, worst = 0, 0.0
    for border in (rr.REFLECT, rr.CLAMP):
        for mode, table, frame0, rows in parameter_modes(b, values):
            delta = rr.coordinate_allowance(op, shape, border, rows, field)
            full, fsx, fsy = rr.remap64(x, op, border, rows, field)
            limit = rr.bound(x, fsx, fsy, delta)
            guard = Guard(gpu)
            xw, tw = guard.inp(x, "x"), guard.inp(table, "param")
            fw = None if field is None else guard.inp(field, "field")
            outs = []
            for kind in SUBSETS:
                sel = rr.selection(kind, c)
                mask = None if sel is None else guard.inp(sel.astype(np.uint8), f"mask {kind}", torch.uint8)
                outs.append((kind, sel, launch(guard, gpu, xw, shape, op, border, tw, frame0, fw, mask, f"y {kind}")))
                launches += 1
            guard.check(written=tuple(f"y {kind}" for kind in SUBSETS))
            assert torch.equal(xw.cpu(), torch.from_numpy(x))
            for kind, sel, yw in outs:
                got = yw.cpu().numpy()
                on = np.ones(c, bool) if sel is None else sel
                assert np.array_equal(got[:, ~on], x[:, ~on]), (mode, kind, "an unselected channel must be copied through")
                err = np.abs(got[:, on] - full[:, on])
                ratio = float(np.divide(err, limit[:, on], out=np.zeros_like(err), where=limit[:, on] > 0).max()) if on.any() else 0.0
                worst = max(worst, ratio)
                assert bool((err <= limit[:, on]).all()), (rr.OP_NAMES[op], border, mode, kind, f"delta {delta:.2e}", float(err.max()), ratio)
    print(f"[{rr.OP_NAMES[op]} {ids(shape)}] largest error / bound over {launches} launches: {worst:.3f}")
    assert launches == 2 * 3 * 4


KNOWN_SHAPES = [(2, 3, 5, 7), (1, 17, 4, 8), (2, 2, 33, 65), (1, 1, 256, 256)]


@pytest.mark.parametrize("border", [rr.REFLECT, rr.CLAMP], ids=["reflect", "clamp"])
@pytest.mark.parametrize("shape", KNOWN_SHAPES, ids=ids)
def test_bit_exact_known_answers(gpu, shape, border):
    b, c, h, w = shape
    x = torch.from_numpy(rr.plain_map(shape, "known"))
    frames = 3
    field = np.zeros((frames, 2, 2, 3), np.float32)
    field[:, 0], field[:, 1] = 2.0, -1.0   # a constant whole-pixel flow: 2 to the right, 1 up
    field[1] += 5.0                        # (frame 1 differs, so a loop position that did not wrap would show)
    noisy = rr.field_bank()
    guard = Guard(gpu)
    xw = guard.inp(x, "x")
    fw, nw = guard.inp(field, "field"), guard.inp(noisy, "noisy field")
    n_out = [0]

    def run(op, row, f=None):
        n_out[0] += 1
        tw = guard.inp(np.array([row], np.float32), f"param {n_out[0]}")
        return launch(guard, gpu, xw, shape, op, border, tw, None, f, None, f"y {n_out[0]}").cpu()

    # the identities
    assert torch.equal(run(rr.SWIRL, [0, 3.5, 0, 0]), x), "a swirl of strength 0"
    assert torch.equal(run(rr.RIPPLE, [0, 2.5, 0.3, 0]), x), "a ripple of amplitude 0"
    assert torch.equal(run(rr.DISPLACE, [0, 1.25, 0, 0], nw), x), "a displacement of amplitude 0"
    # mirror with n = (0, 1), offset 0: the rows above the centre are the flipped rows below it
    flipped = run(rr.MIRROR, [0, 1, 0, 0])
    assert torch.equal(flipped[:, :, : h // 2], x.flip(2)[:, :, : h // 2]) and torch.equal(flipped[:, :, h // 2:], x[:, :, h // 2:])
    # a constant integer field at amplitude 1 is an index shift, reflect- or clamp-indexed
    xs, ys = np.arange(w) + 2, np.arange(h) - 1
    if border == rr.REFLECT:
        xs, ys = rr.fold64(xs, w, rr.REFLECT).astype(np.int64), rr.fold64(ys, h, rr.REFLECT).astype(np.int64)
    else:
        xs, ys = np.clip(xs, 0, w - 1), np.clip(ys, 0, h - 1)
    want = x[:, :, torch.from_numpy(ys)][:, :, :, torch.from_numpy(xs)]
    shifted = run(rr.DISPLACE, [1, 0, 0, 0], fw)
    assert torch.equal(shifted, want)
    # a loop position of F wraps to frame 0 (frame 1 would shift by 7 and 4), also with a real field
    assert torch.equal(run(rr.DISPLACE, [1, frames, 0, 0], fw), shifted)
    assert torch.equal(run(rr.DISPLACE, [1.5, noisy.shape[0], 0, 0], nw), run(rr.DISPLACE, [1.5, 0, 0, 0], nw))
    assert torch.equal(run(rr.DISPLACE, [1, -frames, 0, 0], fw), shifted)
    # a bad row passes the sample through
    nan, inf = float("nan"), float("inf")
    for op, row, f in ((rr.MIRROR, [nan, 1, 0, 0], None), (rr.MIRROR, [0, 1, inf, 0], None), (rr.KALEIDOSCOPE, [6, -inf, 0, 0], None),
                       (rr.KALEIDOSCOPE, [nan, 0, 0, 0], None), (rr.SWIRL, [1, 0, 0, 0], None), (rr.SWIRL, [1, -3, 0, 0], None),
                       (rr.SWIRL, [inf, 2, 0, 0], None), (rr.RIPPLE, [1, 0, 0, 0], None), (rr.RIPPLE, [1, 2, nan, 0], None),
                       (rr.DISPLACE, [nan, 0, 0, 0], nw), (rr.DISPLACE, [1, inf, 0, 0], nw)):
        assert torch.equal(run(op, row, f), x), (rr.OP_NAMES[op], row)
    guard.check(written=tuple(f"y {i + 1}" for i in range(n_out[0])))


def test_a_bad_row_passes_only_its_sample_through(gpu):
    """Per-sample rows with bad ones among them, and a subset of channels: samples with a bad row are copies, the others are bent."""
    shape = (4, 20, 9, 11)
    b, c, h, w = shape
    x = rr.plain_map(shape, "bad")
    rows = np.array([[0.7, 4.0, 0, 0], [0.7, 0.0, 0, 0], [np.nan, 4.0, 0, 0], [-1.1, 2.0, np.inf, 0]], np.float32)  # (p2 is unused)
    sel = rr.selection("third", c)
    guard = Guard(gpu)
    xw, tw = guard.inp(x, "x"), guard.inp(rows, "param")
    mask = guard.inp(sel.astype(np.uint8), "mask", torch.uint8)
    got = launch(guard, gpu, xw, shape, rr.SWIRL, rr.REFLECT, tw, None, None, mask).cpu().numpy()
    guard.check(written=("y",))
    want, fsx, fsy = rr.remap64(x, rr.SWIRL, rr.REFLECT, rows, None, sel)
    assert np.array_equal(got[1], x[1]) and np.array_equal(got[2], x[2]) and np.array_equal(got[:, ~sel], x[:, ~sel])
    limit = rr.bound(x, fsx, fsy, rr.coordinate_allowance(rr.SWIRL, shape, rr.REFLECT, rows))
    assert bool((np.abs(got - want) <= limit).all())
    assert not np.array_equal(got[0, sel], x[0, sel]) and not np.array_equal(got[3, sel], x[3, sel])


def test_degenerate_field_and_axes(gpu):
    """A 1 x 1 field (one flow for the whole map), a 1-wide and a 1-high map: the coordinate scale of a length-1 axis is 0."""
    field = rr.field_bank((2, 2, 1, 1), "dot")
    for shape in [(2, 3, 1, 9), (2, 3, 9, 1), (1, 2, 6, 5)]:
        x = rr.plain_map(shape, "thin")
        for op, f in ((rr.DISPLACE, field), (rr.DISPLACE, rr.field_bank((3, 2, 1, 4), "row")), (rr.RIPPLE, None), (rr.KALEIDOSCOPE, None)):
            rows = rr.device_rows(op, shape[2], shape[3])[: shape[0]]
            for border in (rr.REFLECT, rr.CLAMP):
                guard = Guard(gpu)
                xw, tw = guard.inp(x, "x"), guard.inp(rows, "param")
                fw = None if f is None else guard.inp(f, "field")
                got = launch(guard, gpu, xw, shape, op, border, tw, None, fw).cpu().numpy()
                guard.check(written=("y",))
                want, fsx, fsy = rr.remap64(x, op, border, rows, f)
                limit = rr.bound(x, fsx, fsy, rr.coordinate_allowance(op, shape, border, rows, f))
                assert bool((np.abs(got - want) <= limit).all()), (shape, rr.OP_NAMES[op], border)


@pytest.mark.parametrize("border", [rr.REFLECT, rr.CLAMP], ids=["reflect", "clamp"])
def test_large_finite_parameters_stay_inside_the_buffers(gpu, border):
    """Finite parameters of any size: finite output, every output inside the range of its source plane (a bilinear blend is a convex
    combination), red zones intact.  No comparison against the reference."""
    shape = (3, 8, 33, 65)
    b, c, h, w = shape
    x = rr.plain_map(shape, "large")
    field = rr.field_bank()
    big = 3.0e38
    cases = [(rr.MIRROR, [[0.6, 0.8, 1e9, 0], [0.6, 0.8, -big, 0], [big, -big, 7.0, 0]]),
             (rr.KALEIDOSCOPE, [[1e9, 1e9, -1e9, 0], [6, big, big, 0], [-big, 17453.29, 0.5, 0]]),
             (rr.SWIRL, [[17453.29, 10.0, 0, 0], [big, 1e-38, 0, 0], [-big, big, 0, 0]]),   # (1e6 degrees = 17453.29 rad)
             (rr.RIPPLE, [[1e9, 3.0, 0.2, 0], [big, 1e-38, big, 0], [-1e9, big, -big, 0]]),
             (rr.DISPLACE, [[1e9, 0.5, 0, 0], [big, big, 0, 0], [-big, -1e9 - 0.5, 0, 0]])]
    lo = torch.from_numpy(x).amin(dim=(2, 3), keepdim=True)
    hi = torch.from_numpy(x).amax(dim=(2, 3), keepdim=True)
    for op, rows in cases:
        guard = Guard(gpu)
        xw, tw = guard.inp(x, "x"), guard.inp(np.array(rows, np.float32), "param")
        fw = guard.inp(field, "field") if op == rr.DISPLACE else None
        got = launch(guard, gpu, xw, shape, op, border, tw, None, fw).cpu()
        guard.check(written=("y",))  # (also: every element written and finite)
        assert bool(torch.isfinite(got).all())
        assert bool(((got >= lo) & (got <= hi)).all()), rr.OP_NAMES[op]


def test_rejected_arguments_launch_nothing(gpu):
    b, c, h, w = 2, 3, 5, 7
    guard = Guard(gpu)
    x = guard.inp(rr.plain_map((b, c, h, w), "rej"), "x")
    y = guard.out((b, c, h, w), "y")
    p = guard.inp(np.ones((b, 4), np.float32), "param")
    f = guard.inp(rr.field_bank(), "field")
    st = stream(gpu)
    X, Y, P, FL = x.data_ptr(), y.data_ptr(), p.data_ptr(), f.data_ptr()

    def remap(x=X, y=Y, batch=b, channels=c, h=h, w=w, op=2, border=0, param=P, rows=b, field=None, frames=0, fh=0, fw=0):
        return lib().maua_bend_remap_f32(x, y, batch, channels, h, w, op, border, param, rows, field, frames, fh, fw, None, None, st)

    assert remap(x=None) == -22 and remap(y=None) == -22 and remap(param=None) == -22 and remap(y=X) == -22
    assert remap(batch=0) == -22 and remap(batch=65) == -22 and remap(channels=0) == -22 and remap(h=0) == -22 and remap(w=-1) == -22
    assert remap(op=5) == -22 and remap(op=-1) == -22 and remap(border=2) == -22 and remap(rows=0) == -22 and remap(rows=b + 1) == -22
    assert remap(op=4) == -22 and remap(op=4, field=FL, frames=0, fh=6, fw=9) == -22 and remap(op=4, field=FL, frames=4, fh=6, fw=0) == -22
    assert guard.untouched("y")
    guard.check()
    assert remap(op=4, field=FL, frames=4, fh=6, fw=9) == 0 and remap() == 0  # (the same calls with valid arguments are served)
    guard.check(written=("y",))


def test_modules_eager_and_static_forms(gpu):
    """RemapBend and the five NetworkBend classes: ``forward`` on a batch (one row, or rows cut to the batch) equals ``run_static`` on the
    whole sequence through a frame source, both agree with the reference, and a second static call allocates nothing."""
    import maua_stylegan2_amd.audioreactive as ar

    n, b, c, h, w = 9, 4, 20, 16, 32
    shape = (b, c, h, w)
    x = rr.plain_map(shape, "mod")
    xd = torch.from_numpy(x).to(gpu)
    idx = [1, 4, 5, 19]
    sel = np.zeros(c, bool)
    sel[idx] = True
    field = rr.field_bank()
    ramp = torch.linspace(-1.0, 1.0, n)
    cases = [(rr.MIRROR, lambda m: ar.Mirror(m, offset=1.5, channels=idx), 90 * ramp, lambda m: np.stack([m, 0 * m + 1.5], 1)),
             (rr.KALEIDOSCOPE, lambda m: ar.Kaleidoscope(m, angle=10.0, sectors=5, channels=torch.tensor(idx)), 180 * ramp,
              lambda m: np.stack([0 * m + 5, 0 * m + 10, m], 1)),
             (rr.SWIRL, lambda m: ar.Swirl(m, radius=9.0, channels=idx, border="clamp"), 200 * ramp, lambda m: np.stack([m, 0 * m + 9], 1)),
             (rr.RIPPLE, lambda m: ar.Ripple(m, wavelength=7.0, channels=idx), torch.stack([2 * ramp, 5 + ramp, ramp], 1)[:, :2],
              lambda m: np.concatenate([m, 0 * m[:, :1]], 1)),
             (rr.DISPLACE, lambda m: ar.Displace(m, torch.from_numpy(field), channels=idx), torch.stack([3 * ramp, 0.6 * torch.arange(n)], 1),
              lambda m: m)]
    src = frame_source(gpu, FRAME0)
    for op, make, mod, public in cases:
        border = rr.CLAMP if op == rr.SWIRL else rr.REFLECT
        f = field if op == rr.DISPLACE else None
        rows = make(mod).sequential.table.numpy()  # the float32 rows the device is given ...
        assert np.allclose(rows, rr.rows_from_degrees(op, public(mod.numpy().astype(np.float64))), rtol=0, atol=1e-6)  # ... are these
        eager = make(mod[FRAME0: FRAME0 + b].to(gpu))
        assert np.allclose(eager.sequential.table.cpu().numpy(), rows[FRAME0: FRAME0 + b], rtol=0, atol=1e-6)
        cut = eager.sequential.table.cpu().numpy()  # (the conversion from degrees ran on the device: to the last bit what it computed)
        want, fsx, fsy = rr.remap64(x, op, border, cut, f, sel)
        limit = rr.bound(x, fsx, fsy, rr.coordinate_allowance(op, shape, border, cut, f))
        got = eager(xd)
        assert got.data_ptr() != xd.data_ptr() and bool((np.abs(got.cpu().numpy() - want) <= limit).all()), rr.OP_NAMES[op]
        whole = make(mod.to(gpu))
        assert whole.sequence_rows == n and whole.capturable
        out = torch.full_like(xd, float("nan"))
        assert whole.run_static(xd, out, src.data_ptr()) is out
        assert torch.equal(out, got), "the static form reads the same rows through the frame source"
        held, held_field = dict(whole.sequential._dev), dict(whole.sequential._field_dev)
        torch.cuda.synchronize()
        before = torch.cuda.memory_stats(gpu)["allocation.all.allocated"]
        whole.run_static(xd, out, src.data_ptr())
        torch.cuda.synchronize()
        assert torch.cuda.memory_stats(gpu)["allocation.all.allocated"] == before, "a second call must allocate nothing"
        assert whole.sequential._dev.keys() == held.keys() and all(whole.sequential._dev[k] is v for k, v in held.items())
        assert all(whole.sequential._field_dev[k] is v for k, v in held_field.items()) and len(held_field) == (op == rr.DISPLACE)
        assert torch.equal(out, got)
        one = make(mod[4:5].to(gpu))  # one row serves every sample
        row = one.sequential.table.cpu().numpy()
        assert np.allclose(row, rows[4:5], rtol=0, atol=1e-6)
        want1 = rr.remap64(x, op, border, np.repeat(row, b, 0), f, sel)
        limit1 = rr.bound(x, want1[1], want1[2], rr.coordinate_allowance(op, shape, border, row, f))
        assert bool((np.abs(one(xd).cpu().numpy() - want1[0]) <= limit1).all())
        with pytest.raises(RuntimeError, match="parameter rows"):
            make(mod[:b + 1].to(gpu))(xd)
    with pytest.raises(RuntimeError, match="channels"):
        ar.Swirl(torch.ones(b), radius=2.0, channels=[0, c])(xd)
    with pytest.raises(RuntimeError, match="CUDA"):
        ar.Swirl(torch.ones(b), radius=2.0)(torch.from_numpy(x))
