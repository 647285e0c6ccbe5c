"""GPU: maua_fused_bias_act_f32 / _f16 / _f64 and maua_upfirdn2d_f16 / _f64 through the C ABI.

fused_bias_act: bit-equal to a numpy model that performs the same operations in the same order in the arithmetic type — add the bias
(index (i / step_b) % size_b), select by act * 10 + grad, multiply by alpha where the code does, multiply by scale.  The arithmetic type
is fp32 for f32 and f16 and fp64 for f64.  The chain has no multiply followed by an add, so contraction to a fused multiply-add cannot
change the fp32 and fp64 forms.  The f16 form IS contracted, at its last step: the compiler turns half(out * scale) into one mixed-precision
instruction (v_fma_mixlo_f16 out, scale, 0 in the kernel's assembly), so the product with `scale` is exact and the f16 result is rounded
ONCE, from that product — not from its fp32 rounding.  The model does the same (the product of two fp32 values is exact in fp64).  The
two roundings differ where the fp32 product lands on a tie between two halves: 4 of the 2,101,248 elements of second_trip_vector under
code 30, 22 under code 31, 1 of second_trip_scalar under code 31, none of the small cases — which is how the first run of this file on the
device found it (the fp32-rounded model missed exactly those elements).

upfirdn2d (typed): against a vectorised numpy float64 reference — zero-stuff, pad or crop, correlate with the flipped taps, decimate.
Bounds, elementwise:  f64  (kh * kw + 2) * 2^-53 * sum |k||x|;  f16  2^-11 * |want| + (kh * kw + 2) * 2^-24 * sum |k||x|  (inputs and taps
are rounded to half before the reference sees them; accumulation is fp32 with one output rounding).

Every buffer is a tests/redzone.py window.  Worst error / bound ratios are printed ([upfirdn2d_f16], [upfirdn2d_f64])."""
import numpy as np
import pytest
import torch

from maua_stylegan2_amd import _lib
from redzone import CANARY_BITS, Guard
from upfirdn_ref import pad_crop, upfirdn_out_shape, upfirdn_ref  # noqa: F401  (the float64 reference, shared with test_upfirdn2d_entries_*)

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

EINVAL = -22
CODES = [(1, 0), (1, 1), (1, 2), (3, 0), (3, 1), (3, 2), (7, 3)]  # act, grad: 10, 11, 12, 30, 31, 32 and an unknown code (the identity)
TYPES = {"f32": (np.float32, np.float32, torch.float32), "f16": (np.float16, np.float32, torch.float16), "f64": (np.float64, np.float64, torch.float64)}
GRID_ELEMENTS = 2048 * 256  # work items of one grid-stride trip of the bias_act kernels

# ---------------------------------------------------------------------------------------------------------------- fused_bias_act
# name -> n, size_b, step_b and what differs from the plain call
BIAS_ACT_CASES = {
    "vector_bias_wraps": dict(n=156, size_b=5, step_b=12),                    # 13 planes over 5 biases: the index wraps mid-tensor
    "size_x_not_4": dict(n=157, size_b=5, step_b=12),
    "step_b_not_4": dict(n=156, size_b=5, step_b=6),
    "x_off_alignment": dict(n=156, size_b=5, step_b=12, skew="x"),
    "y_off_alignment": dict(n=156, size_b=5, step_b=12, skew="y"),
    "ref_off_alignment": dict(n=156, size_b=5, step_b=12, skew="ref"),
    "in_place": dict(n=156, size_b=5, step_b=12, in_place=True),
    "in_place_scalar": dict(n=157, size_b=5, step_b=12, in_place=True),
    "no_ref": dict(n=156, size_b=5, step_b=12, ref=False),
    "no_bias": dict(n=156, size_b=5, step_b=12, bias=False),
    "size_b_zero": dict(n=156, size_b=0, step_b=12),
    "second_trip_vector": dict(n=2101248, size_b=5, step_b=4096, codes=[(3, 0), (3, 1)]),
    "second_trip_scalar": dict(n=524288 + 77, size_b=5, step_b=77, codes=[(3, 0), (3, 1)]),
}
F32_ONLY = ("x_off_alignment", "y_off_alignment", "ref_off_alignment")


def bias_act_model(x, b, ref, size_b, step_b, act, grad, alpha, scale, out_type, arith):
    """The kernel's chain in ``arith``; b / ref may be None.  For half the last multiply and the rounding to half are one step."""
    v = x.astype(arith)
    if b is not None and size_b > 0:
        v = v + b.astype(arith)[(np.arange(x.size) // step_b) % size_b]
    r = ref.astype(arith) if ref is not None else np.zeros(x.size, arith)
    a, s = arith(np.float32(alpha)), arith(np.float32(scale))
    code = act * 10 + grad
    if code in (12, 32):
        out = np.zeros(x.size, arith)
    elif code == 30:
        out = np.where(v > 0, v, v * a)
    elif code == 31:
        out = np.where(r > 0, v, v * a)
    else:
        out = v
    assert out.dtype == arith
    if out_type == np.float16:  # one instruction on the device: the exact product, rounded once to half
        return (out.astype(np.float64) * np.float64(s)).astype(np.float16)
    out = out * s
    assert out.dtype == arith
    return out.astype(out_type)


def bias_act_operands(case, out_type):
    n, size_b = case["n"], case["size_b"]
    r = np.random.default_rng(n + 3 * case["step_b"])
    x = r.standard_normal(n).astype(out_type)
    b = r.standard_normal(max(size_b, 1)).astype(out_type) if case.get("bias", True) else None
    ref = r.standard_normal(n).astype(out_type) if case.get("ref", True) else None
    return x, b, ref


def _bits(a):
    return a.view({2: np.uint16, 4: np.uint32, 8: np.uint64}[a.dtype.itemsize])


def _window(g, data, n, name, tdtype, skew, is_out):
    """A window of n elements; with ``skew`` it starts one element into a 16-byte aligned buffer and that element keeps the canary.
    Returns (window, whole buffer or None)."""
    if not is_out and not skew:
        return g.inp(data, name, tdtype), None
    full = g.out((n + skew,), name, tdtype)
    if data is not None:
        full[skew:].copy_(torch.from_numpy(data))
    return full[skew:], full


def _bias_act_launch(gpu, suffix, case, x, b, ref, act, grad, alpha, scale):
    lib = _lib.load()
    _, _, tdtype = TYPES[suffix]
    skew, n = case.get("skew"), x.size
    g = Guard(gpu)
    bt = g.inp(b, "b", tdtype) if b is not None else None
    rt, rfull = _window(g, ref, n, "ref", tdtype, int(skew == "ref"), False) if ref is not None else (None, None)
    if case.get("in_place"):
        yt, yfull = _window(g, x, n, "y", tdtype, 0, True)
        xt, xfull = yt, None
    else:
        xt, xfull = _window(g, x, n, "x", tdtype, int(skew == "x"), False)
        yt, yfull = _window(g, None, n, "y", tdtype, int(skew == "y"), True)
    if suffix == "f32":
        for t, off in ((xt, skew == "x"), (yt, skew == "y"), (rt, skew == "ref")):
            assert t is None or (t.data_ptr() % 16 != 0) == off
    fn = getattr(lib, f"maua_fused_bias_act_{suffix}")
    rc = fn(xt.data_ptr(), _lib.ptr(bt), _lib.ptr(rt), yt.data_ptr(), n, case["size_b"], case["step_b"], act, grad, alpha, scale,
            _lib.stream_ptr(gpu))
    assert rc == 0, rc
    g.check(written=() if skew == "y" else ("y",))
    for full, skewed in ((xfull, skew == "x"), (yfull, skew == "y"), (rfull, skew == "ref")):
        if skewed:
            assert bool((full[:1].view(torch.int32) == CANARY_BITS).all()), "write in front of a skewed window"
    return yt.cpu().numpy()


BIAS_ACT_RUNS = [(sfx, name) for sfx in ("f32", "f16", "f64") for name in BIAS_ACT_CASES if sfx == "f32" or name not in F32_ONLY]


@pytest.mark.parametrize("suffix,name", BIAS_ACT_RUNS)
def test_fused_bias_act_bit_equal_to_the_model(gpu, suffix, name):
    case = BIAS_ACT_CASES[name]
    out_type, arith, _ = TYPES[suffix]
    x, b, ref = bias_act_operands(case, out_type)
    if suffix == "f32":  # the path this case is here for
        vec = case["n"] % 4 == 0 and case["step_b"] % 4 == 0 and not case.get("skew")
        assert vec == (name in ("vector_bias_wraps", "in_place", "no_ref", "no_bias", "size_b_zero", "second_trip_vector"))
        if name.startswith("second_trip"):
            assert (case["n"] // 4 if vec else case["n"]) > GRID_ELEMENTS
    elif name.startswith("second_trip"):
        assert case["n"] > GRID_ELEMENTS
    for act, grad in case.get("codes", CODES):
        alpha, scale = 0.2, 1.4142135381698608
        got = _bias_act_launch(gpu, suffix, case, x, b, ref, act, grad, alpha, scale)
        want = bias_act_model(x, b, ref, case["size_b"], case["step_b"], act, grad, alpha, scale, out_type, arith)
        bad = int((_bits(got) != _bits(want)).sum())
        assert bad == 0, (suffix, name, act, grad, bad)
    print(f"[fused_bias_act_{suffix}] {name}: bit-equal to the model over {len(case.get('codes', CODES))} codes")


@pytest.mark.parametrize("suffix", ["f32", "f16", "f64"])
def test_fused_bias_act_empty_and_refusals(gpu, suffix):
    lib = _lib.load()
    out_type, _, tdtype = TYPES[suffix]
    fn = getattr(lib, f"maua_fused_bias_act_{suffix}")
    g = Guard(gpu)
    x, b, y = g.inp(np.ones(16, out_type), "x", tdtype), g.inp(np.ones(4, out_type), "b", tdtype), g.out((16,), "y", tdtype)
    st = _lib.stream_ptr(gpu)
    assert fn(x.data_ptr(), b.data_ptr(), None, y.data_ptr(), 0, 4, 4, 3, 0, 0.2, 1.0, st) == 0      # size_x == 0: nothing to do
    assert fn(None, None, None, None, 0, 0, 1, 3, 0, 0.2, 1.0, st) == 0
    assert fn(x.data_ptr(), b.data_ptr(), None, y.data_ptr(), 16, 4, 0, 3, 0, 0.2, 1.0, st) == EINVAL
    assert fn(x.data_ptr(), b.data_ptr(), None, y.data_ptr(), 16, 4, -4, 3, 0, 0.2, 1.0, st) == EINVAL
    assert fn(x.data_ptr(), b.data_ptr(), None, y.data_ptr(), -1, 4, 4, 3, 0, 0.2, 1.0, st) == EINVAL
    assert fn(None, b.data_ptr(), None, y.data_ptr(), 16, 4, 4, 3, 0, 0.2, 1.0, st) == EINVAL
    assert fn(x.data_ptr(), b.data_ptr(), None, None, 16, 4, 4, 3, 0, 0.2, 1.0, st) == EINVAL
    assert g.untouched("y")
    g.check()


# ---------------------------------------------------------------------------------------------------------------- upfirdn2d, typed
# name -> (major, in_h, in_w, minor, kh, kw, up_x, up_y, down_x, down_y, pad_x0, pad_x1, pad_y0, pad_y1)
UPFIRDN_CASES = {
    "minor_3": (2, 7, 9, 3, 3, 3, 1, 1, 1, 1, 1, 1, 1, 1),
    "per_axis_everything": (3, 6, 11, 1, 3, 5, 2, 3, 3, 1, 2, -1, 1, 3),
    "per_axis_minor_2": (2, 5, 4, 2, 3, 5, 2, 3, 3, 1, 2, -1, 1, 3),
    "taps_1x1": (2, 5, 6, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0),
    "one_output": (1, 2, 2, 1, 4, 4, 1, 1, 1, 1, 1, 1, 1, 1),
    "second_trip": (1, 1500, 1400, 1, 2, 2, 1, 1, 1, 1, 1, 0, 0, 1),
}
UPFIRDN_GRID_ELEMENTS = 8192 * 256


def upfirdn_ref_and_bound(x, k, params, suffix):
    """(want, bound) for operands already rounded to the tensor type."""
    x8, k8 = x.astype(np.float64), k.astype(np.float64)
    want = upfirdn_ref(x8, k8, *params)
    mag = upfirdn_ref(np.abs(x8), np.abs(k8), *params)
    taps = k.shape[0] * k.shape[1]
    if suffix == "f64":
        return want, (taps + 2) * 2.0 ** -53 * mag
    return want, 2.0 ** -11 * np.abs(want) + (taps + 2) * 2.0 ** -24 * mag


def upfirdn_operands(case, out_type):
    major, in_h, in_w, minor, kh, kw = case[:6]
    r = np.random.default_rng(in_h * 131 + in_w * 7 + kh + minor)
    return r.standard_normal((major, in_h, in_w, minor)).astype(out_type), (0.5 * r.standard_normal((kh, kw))).astype(out_type)


@pytest.mark.parametrize("name", list(UPFIRDN_CASES))
@pytest.mark.parametrize("suffix", ["f16", "f64"])
def test_upfirdn2d_typed_against_float64(gpu, suffix, name):
    lib = _lib.load()
    case = UPFIRDN_CASES[name]
    out_type, _, tdtype = TYPES[suffix]
    x, k = upfirdn_operands(case, out_type)
    want, bound = upfirdn_ref_and_bound(x, k, case[6:], suffix)
    shape = upfirdn_out_shape(case)
    assert want.shape == shape, (want.shape, shape)
    if name == "second_trip":
        assert want.size > UPFIRDN_GRID_ELEMENTS
    if name == "one_output":
        assert want.size == 1
    g = Guard(gpu)
    xt, kt, y = g.inp(x, "x", tdtype), g.inp(k, "k", tdtype), g.out(shape, "y", tdtype)
    rc = getattr(lib, f"maua_upfirdn2d_{suffix}")(xt.data_ptr(), kt.data_ptr(), y.data_ptr(), *case, _lib.stream_ptr(gpu))
    assert rc == 0, rc
    g.check(written=("y",))
    err = np.abs(y.cpu().numpy().astype(np.float64) - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    print(f"[upfirdn2d_{suffix}] {name}: worst error / bound {float(ratio.max()):.4f} (max error {float(err.max()):.3e})")
    assert float(ratio.max()) <= 1.0, (suffix, name, float(ratio.max()))


@pytest.mark.parametrize("suffix", ["f32", "f16", "f64"])
def test_upfirdn2d_empty_tensor_is_a_no_op_in_every_entry(gpu, suffix):
    """major == 0 returns 0 without a launch in all three entries; a negative major is refused."""
    lib = _lib.load()
    out_type, _, tdtype = TYPES[suffix]
    g = Guard(gpu)
    x, k, y = g.inp(np.ones(16, out_type), "x", tdtype), g.inp(np.ones(4, out_type), "k", tdtype), g.out((16,), "y", tdtype)
    fn = getattr(lib, f"maua_upfirdn2d_{suffix}")
    tail = (4, 4, 1, 2, 2, 1, 1, 1, 1, 1, 0, 1, 0)
    assert fn(x.data_ptr(), k.data_ptr(), y.data_ptr(), 0, *tail, _lib.stream_ptr(gpu)) == 0
    assert fn(x.data_ptr(), k.data_ptr(), y.data_ptr(), -1, *tail, _lib.stream_ptr(gpu)) == EINVAL
    assert g.untouched("y")
    g.check()
