"""GPU: maua_grade_f32 / maua_grade_to_u8 (csrc/grade.hip) called through the C ABI between red zones (tests/redzone.py), against the numpy
twin tests/grade_ref.py: bit for bit wherever power == 1 (the float32 emulation), under a derived tolerance where it is not.

The device raises t to the power with ``powf`` (OCML's pow, correctly rounded to a few ulp; the OpenCL specification allows pow 16 ulp,
which is what the bound below is written for)."""
import numpy as np
import pytest
import torch

import grade_ref as gr
from maua_stylegan2_amd import _lib
from redzone import Guard

pytestmark = pytest.mark.gpu
F32 = np.float32
EINVAL, ENOSYS = -22, -38


def _windows(g, x, rows, lut, stride, skew=False):
    """The operands of a launch in guarded windows: the image (``skew``: 4 bytes off a 16-byte boundary), the rows at ``stride`` floats with
    junk behind column 23, the LUT padded to four floats with a NaN in the unused one."""
    if skew:
        img = g.inp(np.concatenate([[F32(0)], x.reshape(-1)]), "img")[1:].view(x.shape)
    else:
        img = g.inp(x, "img")
    table = np.full((rows.shape[0], stride), 7.5, F32)
    table[:, :gr.ROW] = rows
    rt = g.inp(table, "rows")
    lt = None
    if lut is not None:
        padded = gr.pad_lut(lut)
        padded[:, 3] = np.nan
        lt = g.inp(padded, "lut")
        assert lt.data_ptr() % 16 == 0
    return img, rt, lt


def _out(g, kind, b, h, w, name, skew=False):
    """The output window; ``skew``: one element (4 bytes of fp32, 1 byte of uint8) further in, the element in front zeroed so that the
    window holds no canary once the launch has written the rest."""
    shape, dtype = ((b, 3, h, w), torch.float32) if kind == "f32" else ((b, h, w, 3), torch.uint8)
    if not skew:
        return g.out(shape, name, dtype)
    full = g.out((b * h * w * 3 + 1,), name, dtype)
    full[0] = 0
    return full[1:].view(shape)


def _call(kind, img, out, rt, lt, stride, lut_n, b=None, h=None, w=None):
    fn = _lib.load().maua_grade_f32 if kind == "f32" else _lib.load().maua_grade_to_u8
    b0, _, h0, w0 = img.shape
    return fn(img.data_ptr(), out if isinstance(out, int) else out.data_ptr(), b0 if b is None else b, h0 if h is None else h, w0 if w is None else w,
              rt.data_ptr(), stride, None if lt is None else lt.data_ptr(), lut_n, _lib.stream_ptr())


def _run(gpu, kind, x, rows, lut, stride=24, skew=False, written_check=True):
    """One guarded launch -> the output as numpy (float32 [b, 3, h, w] or uint8 [b, h, w, 3])."""
    g = Guard(gpu)
    img, rt, lt = _windows(g, x, rows, lut, stride, skew)
    b, _, h, w = x.shape
    out = _out(g, kind, b, h, w, "out", skew)
    assert _call(kind, img, out, rt, lt, stride, 0 if lut is None else lut.shape[0]) == 0
    g.check(written=("out",) if written_check else (), nonfinite_ok=("out",))
    return out.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _assert_case(gpu, case, skew=False):
    x, rows, lut = gr.build_case(case)
    want = gr.grade(x, rows, lut, F32)
    got = _run(gpu, "f32", x, rows, lut, case["stride"], skew)
    same = _bits(got) == _bits(want)
    assert same.all(), (case, int((~same).sum()), float(np.nanmax(np.abs(got.astype(np.float64) - want))))
    got8 = _run(gpu, "u8", x, rows, lut, case["stride"], skew)
    assert np.array_equal(got8, gr.quant8(want)), (case, int((got8 != gr.quant8(want)).sum()))


@pytest.mark.parametrize("shape", gr.SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_power_one_is_the_float32_twin_bit_for_bit(gpu, shape):
    """Every LUT size and mix, graded and mixed identity / graded batches, row strides 24 and 32; plane % 4 == 0 takes the vector path
    (16 x 16, 64 x 64: one and four workgroups per frame), everything else the scalar path (33 x 130: 17 workgroups)."""
    cases = [c for c in gr.gpu_cases() if c["shape"] == shape]
    assert len(cases) == 12
    for case in cases:
        _assert_case(gpu, case)


def test_skewed_pointers_take_the_scalar_path_to_the_same_bits(gpu):
    """A vector-sized plane whose image and output sit 4 bytes (uint8 output: 1 byte) off the alignment the vector path needs."""
    for case in [c for c in gr.gpu_cases() if c["shape"] in ((3, 16, 16), (1, 64, 64)) and c["n_lut"] in (0, 17)][:6]:
        _assert_case(gpu, case, skew=True)


@pytest.mark.parametrize("shape,n_lut", [((1, 1025, 1024), 17), ((1, 513, 513), 0)], ids=["vector", "scalar"])
def test_a_second_trip_of_the_grid_stride_loop(gpu, shape, n_lut):
    """1024 workgroups serve a frame: 262144 items a trip — 4 pixels each on the vector path, one on the scalar path."""
    b, h, w = shape
    assert (h * w % 4 == 0) == bool(n_lut) and h * w // (4 if n_lut else 1) > 1024 * 256
    case = dict(shape=shape, kind="graded", n_lut=n_lut, mix=0.5, stride=24, seed=77)
    x, rows, lut = gr.build_case(case)
    want = gr.grade(x, rows, lut, F32)
    got = _run(gpu, "f32", x, rows, lut)
    assert np.array_equal(_bits(got), _bits(want))
    assert np.array_equal(_run(gpu, "u8", x, rows, lut), gr.quant8(want))


def test_identity_rows_pass_the_frame_through(gpu):
    """fp32: the input's bits, NaN payloads included; uint8: maua_frames_to_u8's output — with and without a LUT (lut_mix 0), on both paths."""
    lib = _lib.load()
    for shape, n_lut in (((2, 5, 7), 0), ((3, 16, 16), 3), ((2, 33, 130), 17), ((1, 64, 64), 0)):
        b, h, w = shape
        x = gr.case_image(b, h, w, n_lut, seed=5)
        flat = x.reshape(-1).view(np.uint32)
        flat[:4] = (0x7FC12345, 0xFFC00001, 0x7F800001, 0x7FFFFFFF)  # NaNs with payloads, one of them signalling
        rows = gr.case_rows("identity", b)
        lut = gr.sample_lut(n_lut) if n_lut else None
        assert gr.is_identity(rows, lut is not None).all()
        got = _run(gpu, "f32", x, rows, lut)
        assert np.array_equal(_bits(got), _bits(x))
        got8 = _run(gpu, "u8", x, rows, lut)
        plain, xd = torch.empty((b, h, w, 3), dtype=torch.uint8, device=gpu), torch.from_numpy(x).to(gpu)
        assert lib.maua_frames_to_u8(xd.data_ptr(), plain.data_ptr(), b, h, w, _lib.stream_ptr()) == 0
        assert np.array_equal(got8, plain.cpu().numpy()) and np.array_equal(got8, gr.quant8(x))


def test_power_alone_is_within_the_bound_of_pow(gpu):
    """slope 1, offset 0, M = I, bias 0, no LUT: y = fl(2 powf(t, p) - 1) with t = clamp01(fl(x / 2 + 1 / 2)), the same float32 base the
    twin has; bound: gr.pow_bound (2 x 16 ulp of t^p, doubled by the scaling, plus the subtraction's rounding)."""
    rng = np.random.default_rng(11)
    x = rng.uniform(-1.1, 1.1, (3, 3, 16, 16)).astype(F32)
    x.reshape(-1)[:4] = (-1, 1, 0, np.nan)
    rows = np.stack([gr.make_row(power=p) for p in ([0.45, 2.2, 1.0], [1 / 3, 3.0, 0.9], [1.7, 0.5, 2.0])]).astype(F32)
    got = _run(gpu, "f32", x, rows, None).astype(np.float64)
    t = gr.clamp01(np.where(np.isnan(x), F32(-1), x) * F32(0.5) + F32(0.5))
    worst = 0.0
    for b in range(3):
        for c in range(3):
            p = rows[b, gr.POWER + c]
            want = 2 * np.power(t[b, c].astype(np.float64), np.float64(p)) - 1
            err, bound = np.abs(got[b, c] - want), gr.pow_bound(t[b, c], p)
            worst = max(worst, float(np.max(err / bound)))
            assert (err <= bound).all(), (b, c, float(p), float(np.max(err / bound)))
            assert (got[b, c][t[b, c] == 0] == -1).all()  # 0 stays 0
    print(f"powf alone: worst error / bound = {worst:.4f}")


@pytest.mark.parametrize("case", gr.power_cases(), ids=lambda c: f"{'x'.join(map(str, c['shape']))}-lut{c['n_lut']}")
def test_power_in_the_full_chain_is_within_four_times_the_emulations_error(gpu, case):
    x, rows, lut = gr.build_case(case, power=True)
    allow, own = gr.allowance(x, rows, lut)
    assert allow <= gr.CEILING
    want = gr.grade(x, rows, lut, np.float64)
    got = _run(gpu, "f32", x, rows, lut)
    err = float(np.max(np.abs(got.astype(np.float64) - want)))
    print(f"{case['shape']} lut {case['n_lut']}: device error {err:.3e}, float32 emulation's own {own:.3e}, allowed {allow:.3e}")
    assert err <= allow
    got8 = _run(gpu, "u8", x, rows, lut)
    assert np.array_equal(got8, gr.quant8(got))  # the quantiser applied to the device's own fp32 result, bit for bit
    assert np.max(np.abs(got8.astype(np.int32) - gr.quant8(want.astype(F32)).astype(np.int32))) <= 1


def test_in_place_equals_out_of_place(gpu):
    for case in [c for c in gr.gpu_cases() if c["shape"] in ((3, 16, 16), (2, 33, 130)) and c["n_lut"] in (0, 33)]:
        x, rows, lut = gr.build_case(case)
        want = _run(gpu, "f32", x, rows, lut, case["stride"])
        g = Guard(gpu)
        img, rt, lt = _windows(g, x, rows, lut, case["stride"])
        assert _call("f32", img, img, rt, lt, case["stride"], 0 if lut is None else lut.shape[0]) == 0
        g.check()
        assert np.array_equal(_bits(img.cpu().numpy()), _bits(want))


def test_refusals_leave_the_output_untouched(gpu):
    b, h, w = 2, 4, 8
    x = gr.case_image(b, h, w, 3, seed=1)
    rows = gr.case_rows("graded", b)
    for kind in ("f32", "u8"):
        g = Guard(gpu)
        img, rt, lt = _windows(g, x, rows, gr.sample_lut(3), 24)
        out = _out(g, kind, b, h, w, "out")
        fn = _lib.load().maua_grade_f32 if kind == "f32" else _lib.load().maua_grade_to_u8
        st = _lib.stream_ptr()
        ok = (img.data_ptr(), out.data_ptr(), b, h, w, rt.data_ptr(), 24, lt.data_ptr(), 3, st)

        def call(**kw):
            names = ("img", "out", "batch", "h", "w", "rows", "stride", "lut", "lut_n", "stream")
            return fn(*[kw.get(n, v) for n, v in zip(names, ok)])

        for bad in (dict(img=None), dict(out=None), dict(rows=None), dict(h=0), dict(w=-1), dict(batch=-1), dict(stride=23), dict(lut_n=1),
                    dict(lut_n=66), dict(lut=lt.data_ptr() + 4)):
            assert call(**bad) == EINVAL, (kind, bad)
        # partial overlaps: the output starting inside the image, and ending inside it (never dereferenced: refused)
        assert call(out=img.data_ptr() + 16) == EINVAL and call(out=img.data_ptr() - 16) == EINVAL
        if kind == "u8":
            assert call(out=img.data_ptr()) == EINVAL  # the uint8 output cannot be the image
        assert call(batch=65536) == ENOSYS
        assert call(batch=0) == 0 and call(batch=0, img=None, out=None, rows=None) == 0  # a successful no-op
        assert g.untouched("out")
        g.check()
        assert call() == 0
        g.check(written=("out",), nonfinite_ok=("out",))


def test_a_captured_launch_replays_to_the_same_bytes(gpu):
    stream = torch.cuda.Stream(gpu)
    case = dict(shape=(2, 33, 130), kind="mixed", n_lut=17, mix=0.5, stride=32, seed=21)
    x, rows, lut = gr.build_case(case)
    other = gr.case_image(2, 33, 130, 17, seed=22)
    for kind in ("f32", "u8"):
        g = Guard(gpu)
        img, rt, lt = _windows(g, x, rows, lut, 32)
        eager, captured = _out(g, kind, 2, 33, 130, "eager"), _out(g, kind, 2, 33, 130, "graph")
        assert _call(kind, img, eager, rt, lt, 32, 17) == 0
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            with _lib.HipGraph() as graph:
                rc = _call(kind, img, captured, rt, lt, 32, 17)
            assert rc == 0
            graph.replay()
            stream.synchronize()
            first = captured.cpu().numpy()
            img.copy_(torch.from_numpy(other).to(gpu))
            graph.replay()
            stream.synchronize()
        g.check(written=("eager", "graph"), nonfinite_ok=("eager", "graph"))
        want, want_other = gr.grade(x, rows, lut, F32), gr.grade(other, rows, lut, F32)
        if kind == "u8":
            want, want_other = gr.quant8(want), gr.quant8(want_other)
        # (bytes, not values: the identity frames of the fp32 output carry the image's NaNs)
        assert np.array_equal(first.view(np.uint8), eager.cpu().numpy().view(np.uint8)) and np.array_equal(first.view(np.uint8), want.view(np.uint8))
        assert np.array_equal(captured.cpu().numpy().view(np.uint8), want_other.view(np.uint8))
