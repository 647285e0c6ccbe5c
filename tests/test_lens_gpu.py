"""GPU: maua_lens_extract_f32 / maua_lens_blur_f32 / maua_lens_apply_f32 (csrc/lens.hip) called through the C ABI between red zones
(tests/redzone.py), against the numpy twin tests/lens_ref.py.

extract and apply fix their order and contract nothing: bit for bit against the float32 emulation (apply: wherever vignette == 0; with a
vignette — a square root and two more divisions — within 4 x the emulation's own error against float64).  The blur fixes no order: bit
for bit against float64 on dyadic operands, where any order is exact; on real operands per element within max(4 x the emulation's own
error on that case, 4 * 2^-24 max|x|), an allowance that must itself stay under 2 (R + 4) 2^-23 max|x|.  No allowance is computed from
the device's output."""
import ctypes

import numpy as np
import pytest
import torch

import lens_ref as lr
from maua_stylegan2_amd import _lib
from redzone import Guard

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
EINVAL, ENOSYS = -22, -38


def _inp(g, a, name, skew=False):
    """``a`` in a guarded window; ``skew``: 4 bytes off a 16-byte boundary."""
    a = np.ascontiguousarray(a, F32)
    if not skew:
        t = g.inp(a, name)
        assert t.data_ptr() % 16 == 0
        return t
    return g.inp(np.concatenate([[F32(0)], a.reshape(-1)]), name)[1:].view(a.shape)


def _out(g, shape, name, skew=False):
    """An output window; ``skew``: one float further in, the float in front zeroed so that no canary is left once the rest is written."""
    if not skew:
        return g.out(shape, name)
    full = g.out((int(np.prod(shape)) + 1,), name)
    full[0] = 0
    return full[1:].view(shape)


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _plan(h, w, radius, src):
    plan = (ctypes.c_int * 6)()
    assert _lib.load().maua_lens_blur_plan(h, w, radius, src, ctypes.addressof(plan)) == 0
    return list(plan)


# ------------------------------------------------------------------------------------------------------------------ blur
def _blur(gpu, x, taps, radius, skew=False):
    """One guarded launch -> (dst as numpy, the planned instance)."""
    g = Guard(gpu)
    src, tp = _inp(g, x, "src", skew), _inp(g, taps, "taps")
    b, p, h, w = x.shape
    dst = _out(g, x.shape, "dst", skew)
    plan = _plan(h, w, radius, src.data_ptr())
    assert plan[4] <= 64 * 1024 and plan[5] == 1
    assert _lib.load().maua_lens_blur_f32(src.data_ptr(), dst.data_ptr(), b, p, h, w, radius, tp.data_ptr(), taps.shape[1], _lib.stream_ptr()) == 0
    g.check(written=("dst",))
    return dst.cpu().numpy(), plan[0]


def _assert_real(case, got, x, taps):
    t = taps[:, :case["radius"] + 1]
    allow, own, ceiling = lr.blur_allowance(x, t)
    assert allow <= ceiling, (case, allow, ceiling)
    err = np.abs(got.astype(F64) - lr.blur(x, t, F64))
    print(f"{case['shape']} R {case['radius']}: device error {err.max():.3e}, float32 emulation's own {own:.3e}, allowed {allow:.3e}, ceiling {ceiling:.3e}")
    assert (err <= allow).all(), (case, float(err.max()), allow)
    assert np.array_equal(_bits(got[0]), _bits(x[0]))  # frame 0's delta copies: nobody read frame 1's taps for it


@pytest.mark.parametrize("plane", lr.BLUR_PLANES, ids=lambda p: "x".join(map(str, p)))
def test_blur_dyadic_operands_bit_for_bit_and_real_operands_within_the_allowance(gpu, plane):
    """Radii 0, 1, the plane's width (every tap clamped) and 64; batch 2 with the delta in frame 0 and the wide kernel in frame 1; tap
    strides of radius + 1 and beyond, with junk behind the taps."""
    cases = [c for c in lr.blur_cases() if c["shape"][2:] == plane]
    assert len(cases) == len({0, 1, min(plane[1], 64), 64})
    for case in cases:
        x, taps = lr.blur_operands(case, "dyadic")
        got, inst = _blur(gpu, x, taps, case["radius"])
        assert inst == (1 if plane[1] % 4 == 0 else 0)
        want = lr.blur(x, taps[:, :case["radius"] + 1], F64)
        assert np.array_equal(got.astype(F64), want), (case, float(np.abs(got - want).max()))
        x, taps = lr.blur_operands(case, "real")
        got, _ = _blur(gpu, x, taps, case["radius"])
        _assert_real(case, got, x, taps)


def test_the_blur_case_lists_reach_both_instances_and_skewed_pointers_take_the_scalar_one(gpu):
    seen = set()
    for case in lr.blur_cases():
        h, w = case["shape"][2:]
        seen.add(_plan(h, w, case["radius"], 4096)[0])
    assert seen == {0, 1}
    for h, w, radius in ((64, 64, 5), (17, 32, 17), (65, 128, 64)):
        case = dict(shape=(2, 2, h, w), radius=radius, stride=radius + 2, seed=h + radius)
        x, taps = lr.blur_operands(case, "dyadic")
        aligned, inst = _blur(gpu, x, taps, radius)
        skewed, inst_skewed = _blur(gpu, x, taps, radius, skew=True)
        assert (inst, inst_skewed) == (1, 0)
        assert np.array_equal(aligned.astype(F64), lr.blur(x, taps[:, :radius + 1], F64)) and np.array_equal(_bits(aligned), _bits(skewed))
        x, taps = lr.blur_operands(case, "real")
        _assert_real(case, _blur(gpu, x, taps, radius, skew=True)[0], x, taps)


def test_blur_over_several_tiles_on_both_axes_at_the_plan_rules_radii(gpu):
    """130 x 200 is 3 x 4 tiles with ragged last ones; 39 is the radius of bloom_size 0.1 at 1024 px, 5 a sharpen's; three planes as the
    bloom has them.  Gaussian taps per frame of different widths (frame 0 the delta)."""
    for (h, w), radius in (((130, 200), 39), ((130, 197), 5), ((192, 256), 12)):
        rng = np.random.default_rng(radius)
        x = rng.uniform(-1, 1, (2, 3, h, w)).astype(F32)
        taps = lr.gaussian_taps([0.0, radius / 3.0], radius)
        got, inst = _blur(gpu, x, taps, radius)
        assert inst == (w % 4 == 0)
        _assert_real(dict(shape=x.shape, radius=radius), got, x, taps)
        xd = rng.integers(-4, 5, x.shape).astype(F32)
        td = (2.0 ** -rng.integers(1, 4, (2, radius + 1))).astype(F32)
        assert np.array_equal(_blur(gpu, xd, td, radius)[0].astype(F64), lr.blur(xd, td, F64))


# ------------------------------------------------------------------------------------------------------------------ extract
def _extract_rows():
    """Threshold 0 (everything glows), threshold 1 (only the knee lets light through), knee 0 (a hard threshold), and an ordinary row."""
    return np.stack([lr.make_row(threshold=0.0, knee=0.1), lr.make_row(threshold=1.0, knee=0.25), lr.make_row(threshold=0.5, knee=0.0),
                     lr.make_row(threshold=0.6, knee=0.15)])


def _extract_image(h, w, seed):
    x = lr.image(4, h, w, seed, spread=1.6)  # beyond [-1, 1] in places
    flat = x.reshape(-1)
    flat[:: 37] = np.nan
    flat[5:: 101] = np.inf
    flat[7:: 113] = -np.inf
    flat[11:: 97] = 1.0
    flat[13:: 89] = -1.0
    return x


def _extract(gpu, x, rows, d, stride=16, skew=False):
    g = Guard(gpu)
    table = np.full((rows.shape[0], stride), 7.5, F32)
    table[:, :16] = rows
    img, rt = _inp(g, x, "img", skew), _inp(g, table, "rows")
    b, _, h, w = x.shape
    out = _out(g, (b, 3, -(-h // d), -(-w // d)), "out", skew)
    assert _lib.load().maua_lens_extract_f32(img.data_ptr(), out.data_ptr(), b, h, w, d, rt.data_ptr(), stride, _lib.stream_ptr()) == 0
    g.check(written=("out",))
    return out.cpu().numpy()


@pytest.mark.parametrize("d", lr.REDUCTIONS)
def test_extract_is_the_float32_twin_bit_for_bit(gpu, d):
    """h % d != 0 and w % d != 0 wherever d > 1 can have it: 5 x 7 and 67 x 131 take the scalar path (w % 4 != 0), 13 x 20 and 70 x 132 the
    vector path (w % 8 != 0: d = 8 meets a column block half outside), 67 x 131 and 70 x 132 several workgroups."""
    rows = _extract_rows()
    for n, (h, w) in enumerate(((5, 7), (13, 20), (67, 131), (70, 132), (1, 1), (8, 8))):
        x = _extract_image(h, w, seed=10 * d + n)
        want = lr.extract(x, rows, d, F32)
        assert np.isfinite(want).all() and (h * w < 35 or want.max() > 0.05)
        got = _extract(gpu, x, rows, d, stride=16 + 4 * (n % 2))
        same = _bits(got) == _bits(want)
        assert same.all(), (d, h, w, int((~same).sum()), float(np.abs(got - want).max()))
        if w % 4 == 0:
            assert np.array_equal(_bits(_extract(gpu, x, rows, d, skew=True)), _bits(want))
    # a grey of 0.4: it glows at threshold 0, is below threshold 1 - knee, and below a hard threshold of 0.5
    grey = np.full((4, 3, 8, 8), -0.2, F32)
    got = _extract(gpu, grey, rows, d)
    assert (got[0] > 0).all() and (got[1] == 0).all() and (got[2] == 0).all()


# ------------------------------------------------------------------------------------------------------------------ apply
def _apply_operands(b, h, w, d, seed, vignette=False, bloom_shape=None):
    x = lr.image(b, h, w, seed)
    rows = lr.sample_rows(b, seed, vignette=vignette, identity_every=3)
    rng = np.random.default_rng(seed + 1)
    bh, bw = bloom_shape or (-(-h // d), -(-w // d))
    bloom = rng.uniform(0, 1, (b, 3, bh, bw)).astype(F32)
    soft = lr.image(b, h, w, seed + 2)
    x[0].reshape(-1).view(np.uint32)[:4] = (0x7FC12345, 0xFFC00001, 0x7F800001, 0x7FFFFFFF)  # frame 0 is an identity frame: NaNs with payloads
    assert lr.is_identity(rows)[0] and not lr.is_identity(rows)[1:3].any()
    return x, rows, bloom, soft


def _apply(gpu, x, rows, bloom, d, soft, stride=16, skew=False, in_place=False):
    g = Guard(gpu)
    table = np.full((rows.shape[0], stride), 7.5, F32)
    table[:, :16] = rows
    img, rt = _inp(g, x, "img", skew), _inp(g, table, "rows")
    bl = None if bloom is None else _inp(g, bloom, "bloom")
    so = None if soft is None else _inp(g, soft, "soft", skew)
    b, _, h, w = x.shape
    out = img if in_place else _out(g, x.shape, "out", skew)
    bh, bw = (1, 1) if bloom is None else bloom.shape[2:]
    rc = _lib.load().maua_lens_apply_f32(img.data_ptr(), out.data_ptr(), b, h, w, rt.data_ptr(), stride, _lib.ptr(bl), bh, bw, d, _lib.ptr(so),
                                         _lib.stream_ptr())
    assert rc == 0
    g.check(written=() if in_place else ("out",), nonfinite_ok=("out",))
    return out.cpu().numpy()


APPLY_SHAPES = ((3, 16, 16, 2), (4, 33, 130, 4), (3, 64, 64, 8), (3, 5, 7, 1), (3, 37, 52, 8))


@pytest.mark.parametrize("shape", APPLY_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_apply_without_a_vignette_is_the_float32_twin_bit_for_bit(gpu, shape):
    """Each of the NULL bloom / NULL soft combinations, row strides 16 and 24, identity frames with NaN payloads, in place; w % 4 == 0 takes
    the vector path (one and four workgroups a frame), 33 x 130 and 5 x 7 the scalar path; skewed pointers move a vector shape to it."""
    b, h, w, d = shape
    x, rows, bloom, soft = _apply_operands(b, h, w, d, seed=sum(shape))
    for n, (bl, so) in enumerate(((bloom, soft), (bloom, None), (None, soft), (None, None))):
        want = lr.apply(x, rows, bl, d, so, F32)
        got = _apply(gpu, x, rows, bl, d, so, stride=16 + 8 * (n % 2))
        same = _bits(got) == _bits(want)
        assert same.all(), (shape, n, int((~same).sum()), float(np.nanmax(np.abs(got.astype(F64) - want))))
        assert np.array_equal(_bits(got[0]), _bits(x[0]))  # the identity frame: the input's bits
        assert np.array_equal(_bits(_apply(gpu, x, rows, bl, d, so, in_place=True)), _bits(want))
        if w % 4 == 0:
            assert np.array_equal(_bits(_apply(gpu, x, rows, bl, d, so, skew=True)), _bits(want))
    assert not np.array_equal(lr.apply(x, rows, bloom, d, None, F32)[1], x[1]) and not np.array_equal(lr.apply(x, rows, None, d, soft, F32)[1], x[1])


def test_apply_with_a_one_by_one_bloom_map_clamps_every_sample(gpu):
    for b, h, w, d in ((3, 16, 16, 8), (3, 9, 11, 4)):
        x, rows, bloom, soft = _apply_operands(b, h, w, d, seed=3, bloom_shape=(1, 1))
        want = lr.apply(x, rows, bloom, d, None, F32)
        assert np.array_equal(_bits(_apply(gpu, x, rows, bloom, d, None)), _bits(want))
        gain = 2 * rows[1, lr.BLOOM] * bloom[1, 0, 0, 0]
        assert np.allclose(want[1, 0] - x[1, 0], gain, atol=1e-6)  # a constant glow


@pytest.mark.parametrize("shape", APPLY_SHAPES[:4], ids=lambda s: "x".join(map(str, s)))
def test_apply_with_a_vignette_is_within_four_times_the_emulations_error(gpu, shape):
    b, h, w, d = shape
    x, rows, bloom, soft = _apply_operands(b, h, w, d, seed=sum(shape) + 50, vignette=True)
    x[0].reshape(-1)[:4] = 0.25  # (finite throughout: the comparison is by value)
    allow, own = lr.apply_allowance(x, rows, bloom, d, soft)
    assert 0 < allow < 2e-5  # (sanity only: 64 ulp of values below 4; the allowance itself is the measured one)
    got = _apply(gpu, x, rows, bloom, d, soft)
    err = np.abs(got.astype(F64) - lr.apply(x, rows, bloom, d, soft, F64))
    exact = int((_bits(got) == _bits(lr.apply(x, rows, bloom, d, soft, F32))).sum())
    print(f"{shape}: device error {err.max():.3e}, float32 emulation's own {own:.3e}, allowed {allow:.3e}; {exact} of {got.size} elements are the emulation's bits")
    assert (err <= allow).all()
    assert np.array_equal(_bits(got[0]), _bits(x[0]))


@pytest.mark.parametrize("h,w", [(1025, 1024), (1025, 1027)], ids=["vector", "scalar"])
def test_a_second_trip_of_the_grid_stride_loops(gpu, h, w):
    """1024 workgroups serve a frame: 262144 items a trip; apply has h * w / 4 (vector) or h * w (scalar) items, extract at d = 1 h * ceil(w / 4)."""
    assert h * (-(-w // 4)) > 1024 * 256
    x, rows, bloom, soft = _apply_operands(3, h, w, 8, seed=9)
    x, rows, bloom, soft = x[1:2], rows[1:2], bloom[1:2], soft[1:2]
    assert np.array_equal(_bits(_apply(gpu, x, rows, bloom, 8, soft)), _bits(lr.apply(x, rows, bloom, 8, soft, F32)))
    assert np.array_equal(_bits(_extract(gpu, x, rows, 1)), _bits(lr.extract(x, rows, 1, F32)))


# ------------------------------------------------------------------------------------------------------------------ the chain
def test_the_chain_as_lens_frames_launches_it(gpu):
    """render.lens_frames on the case the host test tells the wrong variants apart on: the entries' composition bit for bit (it launches
    exactly those), and the definition within lens_ref.chain_allowance."""
    import maua_stylegan2_amd.audioreactive as ar
    from maua_stylegan2_amd import render

    b, h, w = 3, 37, 50
    x = lr.image(b, h, w, 5)
    lens = ar.Lens(b, bloom=[0.8, 0.5, 1.0], bloom_size=0.25, bloom_threshold=0.5, bloom_knee=0.15, bloom_tint=(1, 0.8, 0.6), sharpen=[0.5, 0, -0.5],
                   sharpen_radius=1.0)
    d, rb, bt, rs, st = lens.plan(h, w)
    rows = np.array(lens.table)
    ops = render._lens_operands(lens, b, b, gpu)
    images = torch.from_numpy(x).to(gpu)
    scratch = {}
    got = render.lens_frames(images, ops, 0, b, scratch)
    assert got is images and len(scratch) == 2
    got = got.cpu().numpy()
    bloom, _ = _blur(gpu, _extract(gpu, x, rows, d), bt, rb)
    soft, _ = _blur(gpu, x, st, rs)
    assert np.array_equal(_bits(got), _bits(_apply(gpu, x, rows, bloom, d, soft)))
    allow, own = lr.chain_allowance(x, rows, d, bt, st)
    err = np.abs(got.astype(F64) - lr.lens(x, rows, d, bt, st, F64))
    print(f"chain: device error {err.max():.3e}, float32 emulation's own {own:.3e}, allowed {allow:.3e}")
    assert (err <= allow).all()
    # a batch further into a per-frame table, and a one-row table
    part = render.lens_frames(torch.from_numpy(x[1:]).to(gpu), ops, 1, 2, {}).cpu().numpy()
    assert np.array_equal(_bits(part), _bits(got[1:]))
    one = render._lens_operands(lens.slice(1, 2), 7, 4, gpu)
    again = render.lens_frames(torch.from_numpy(np.repeat(x[1:2], 3, 0)).to(gpu), one, 4, 3, {}).cpu().numpy()
    assert all(np.array_equal(_bits(again[k]), _bits(got[1])) for k in range(3))  # (the slice's sizes are the table's: the same plan and taps)
    # nothing is launched for a lens that is the identity throughout; a vignette alone launches apply only
    lib = _lib.load()
    with pytest.MonkeyPatch.context() as mp:
        for name in ("maua_lens_extract_f32", "maua_lens_blur_f32", "maua_lens_apply_f32"):
            mp.setattr(lib, name, lambda *a: pytest.fail("an identity lens launched"))
        same = render.lens_frames(torch.from_numpy(x).to(gpu), render._lens_operands(ar.Lens(), b, b, gpu), 0, b, scratch)
        assert np.array_equal(_bits(same.cpu().numpy()), _bits(x)) and len(scratch) == 2
    with pytest.MonkeyPatch.context() as mp:
        for name in ("maua_lens_extract_f32", "maua_lens_blur_f32"):
            mp.setattr(lib, name, lambda *a: pytest.fail("a vignette launched the bloom or the sharpen"))
        vig = ar.Lens(vignette=0.5)
        dark = render.lens_frames(torch.from_numpy(x).to(gpu), render._lens_operands(vig, b, b, gpu), 0, b, scratch).cpu().numpy()
        vig_rows = np.repeat(vig.table, b, 0)
        allow, _ = lr.apply_allowance(x, vig_rows, None, 1, None)
        assert len(scratch) == 2 and (np.abs(dark.astype(F64) - lr.apply(x, vig_rows, None, 1, None, F64)) <= allow).all()


# ------------------------------------------------------------------------------------------------------------------ all entries
def test_refusals_leave_the_outputs_untouched(gpu):
    lib, st = _lib.load(), _lib.stream_ptr()
    b, h, w, d, radius = 2, 6, 8, 2, 3
    x, rows, bloom, soft = _apply_operands(3, h, w, d, seed=1)
    x, rows, bloom, soft = x[1:], rows[1:], bloom[1:], soft[1:]
    g = Guard(gpu)
    img, rt, bl, so = _inp(g, x, "img"), _inp(g, rows, "rows"), _inp(g, bloom, "bloom"), _inp(g, soft, "soft")
    tp = _inp(g, lr.gaussian_taps([1.0, 1.0], radius), "taps")
    small, full = _out(g, (b, 3, 3, 4), "small"), _out(g, (b, 3, h, w), "full")

    def caller(fn, names, ok):
        return lambda **kw: fn(*[kw.get(n, v) for n, v in zip(names, ok)])

    extract = caller(lib.maua_lens_extract_f32, ("img", "out", "batch", "h", "w", "d", "rows", "stride", "stream"),
                     (img.data_ptr(), small.data_ptr(), b, h, w, d, rt.data_ptr(), 16, st))
    blur = caller(lib.maua_lens_blur_f32, ("src", "dst", "batch", "planes", "h", "w", "radius", "taps", "stride", "stream"),
                  (img.data_ptr(), full.data_ptr(), b, 3, h, w, radius, tp.data_ptr(), radius + 1, st))
    apply = caller(lib.maua_lens_apply_f32, ("img", "out", "batch", "h", "w", "rows", "stride", "bloom", "bh", "bw", "d", "soft", "stream"),
                   (img.data_ptr(), full.data_ptr(), b, h, w, rt.data_ptr(), 16, bl.data_ptr(), 3, 4, d, so.data_ptr(), st))
    for bad in (dict(img=None), dict(out=None), dict(rows=None), dict(h=0), dict(w=-1), dict(batch=-1), dict(stride=15), dict(d=0), dict(d=3), dict(d=16),
                dict(out=img.data_ptr() + 16)):
        assert extract(**bad) == EINVAL, ("extract", bad)
    for bad in (dict(src=None), dict(dst=None), dict(taps=None), dict(h=0), dict(w=0), dict(planes=0), dict(batch=-1), dict(radius=-1), dict(radius=65),
                dict(stride=radius), dict(dst=img.data_ptr()), dict(dst=img.data_ptr() + 16), dict(dst=img.data_ptr() - 16)):
        assert blur(**bad) == EINVAL, ("blur", bad)
    for bad in (dict(img=None), dict(out=None), dict(rows=None), dict(h=0), dict(w=0), dict(batch=-1), dict(stride=15), dict(d=3), dict(bh=0), dict(bw=-1),
                dict(out=img.data_ptr() + 16), dict(out=img.data_ptr() - 16), dict(out=so.data_ptr()), dict(out=bl.data_ptr())):
        assert apply(**bad) == EINVAL, ("apply", bad)
    assert apply(bloom=None, d=3, bh=0, bw=0, batch=0) == 0  # (without a bloom its geometry is not looked at)
    assert extract(batch=65536) == ENOSYS and blur(batch=65536) == ENOSYS and blur(planes=65536) == ENOSYS and apply(batch=65536) == ENOSYS
    # a thin plane: few enough pixels, but more 64 x 64 tiles than a launch's x holds at 256 lanes each
    assert blur(h=0x7FFFFF00, w=1) == ENOSYS and blur(h=1, w=0x7FFFFF00) == ENOSYS and blur(h=64 * 0xFFFFFF + 1, w=1) == ENOSYS
    for fn, ptrs in ((extract, dict(img=None, out=None, rows=None)), (blur, dict(src=None, dst=None, taps=None)), (apply, dict(img=None, out=None, rows=None))):
        assert fn(batch=0) == 0 and fn(batch=0, **ptrs) == 0  # a successful no-op
    assert g.untouched("small") and g.untouched("full")
    g.check()
    assert extract() == 0 and blur() == 0
    g.check(written=("small", "full"))
    assert np.array_equal(_bits(small.cpu().numpy()), _bits(lr.extract(x, rows, d, F32)))
    assert apply() == 0
    g.check(written=("full",))
    assert np.array_equal(_bits(full.cpu().numpy()), _bits(lr.apply(x, rows, bloom, d, soft, F32)))


def test_captured_launches_replay_to_the_same_bytes(gpu):
    """Each entry captured on a side stream, replayed once, then once more on new input: the captured launch reads its operands at replay."""
    lib = _lib.load()
    stream = torch.cuda.Stream(gpu)
    b, h, w, d, radius = 3, 33, 52, 4, 9
    x, rows, bloom, soft = _apply_operands(b, h, w, d, seed=21)
    other = lr.image(b, h, w, seed=22)
    taps = lr.gaussian_taps([0.0, 2.0, 3.0], radius)
    g = Guard(gpu)
    img, rt, bl, so, tp = _inp(g, x, "img"), _inp(g, rows, "rows"), _inp(g, bloom, "bloom"), _inp(g, soft, "soft"), _inp(g, taps, "taps")
    bh, bw = bloom.shape[2:]
    outs = {k: (_out(g, s, k + "-eager"), _out(g, s, k + "-graph")) for k, s in (("extract", (b, 3, bh, bw)), ("blur", x.shape), ("apply", x.shape))}

    def launch(kind, out):
        if kind == "extract":
            return lib.maua_lens_extract_f32(img.data_ptr(), out.data_ptr(), b, h, w, d, rt.data_ptr(), 16, _lib.stream_ptr())
        if kind == "blur":
            return lib.maua_lens_blur_f32(img.data_ptr(), out.data_ptr(), b, 3, h, w, radius, tp.data_ptr(), radius + 1, _lib.stream_ptr())
        return lib.maua_lens_apply_f32(img.data_ptr(), out.data_ptr(), b, h, w, rt.data_ptr(), 16, bl.data_ptr(), bh, bw, d, so.data_ptr(), _lib.stream_ptr())

    first = {}
    for kind, (eager, captured) in outs.items():
        assert launch(kind, eager) == 0
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            with _lib.HipGraph() as graph:
                rc = launch(kind, captured)
            assert rc == 0
            graph.replay()
            stream.synchronize()
            first[kind] = captured.cpu().numpy()
            assert np.array_equal(_bits(first[kind]), _bits(eager.cpu().numpy())), kind
            saved = img.clone()
            img.copy_(torch.from_numpy(other).to(gpu))
            graph.replay()
            stream.synchronize()
            second = captured.cpu().numpy()
            img.copy_(saved)
            torch.cuda.synchronize()
        if kind == "extract":
            assert np.array_equal(_bits(first[kind]), _bits(lr.extract(x, rows, d, F32))) and np.array_equal(_bits(second), _bits(lr.extract(other, rows, d, F32)))
        elif kind == "apply":
            assert np.array_equal(_bits(first[kind]), _bits(lr.apply(x, rows, bloom, d, soft, F32)))
            assert np.array_equal(_bits(second), _bits(lr.apply(other, rows, bloom, d, soft, F32)))
        else:
            for got, src in ((first[kind], x), (second, other)):  # (frame 0 of x carries the NaNs of apply's identity frame: frames 1 .. here)
                allow, _, ceiling = lr.blur_allowance(src[1:], taps[1:])
                assert allow <= ceiling and (np.abs(got[1:].astype(F64) - lr.blur(src[1:], taps[1:], F64)) <= allow).all()
    g.check(written=[k + s for k in outs for s in ("-eager", "-graph")], nonfinite_ok=[k + s for k in outs for s in ("-eager", "-graph")])
