"""float64 reference of upfirdn2d for the entry-level tests (tests/test_native_ops_entries_gpu.py, tests/test_upfirdn2d_entries_*.py):
zero-stuff by the up factors, pad or crop, correlate with the flipped taps, decimate by the down factors — vectorised numpy, one tap at a
time.  tests/test_upfirdn2d_entries_host.py checks it against the scalar loops of oracle/ops_oracle.py."""
import numpy as np


def pad_crop(a, p0, p1, axis):
    """Zero padding of ``a`` along ``axis`` by p0 in front and p1 behind; a negative pad crops."""
    a = np.moveaxis(a, axis, 0)
    if p0 < 0:
        a, p0 = a[-p0:], 0
    if p1 < 0:
        a, p1 = a[:max(a.shape[0] + p1, 0)], 0
    z = lambda n: np.zeros((n,) + a.shape[1:], a.dtype)  # noqa: E731
    return np.moveaxis(np.concatenate([z(p0), a, z(p1)]), 0, axis)


def upfirdn_ref(x, k, up_x, up_y, down_x, down_y, pad_x0, pad_x1, pad_y0, pad_y1):
    """x [major, in_h, in_w, minor], k [kh, kw], float64."""
    major, in_h, in_w, minor = x.shape
    kh, kw = k.shape
    canvas = np.zeros((major, in_h * up_y, in_w * up_x, minor))
    canvas[:, ::up_y, ::up_x] = x
    canvas = pad_crop(pad_crop(canvas, pad_y0, pad_y1, 1), pad_x0, pad_x1, 2)
    oh, ow = canvas.shape[1] - kh + 1, canvas.shape[2] - kw + 1
    kf = k[::-1, ::-1]
    out = np.zeros((major, oh, ow, minor))
    for i in range(kh):
        for j in range(kw):
            out += kf[i, j] * canvas[:, i:i + oh, j:j + ow]
    return out[:, ::down_y, ::down_x]


def upfirdn_out_shape(case):
    major, in_h, in_w, minor, kh, kw, up_x, up_y, down_x, down_y, px0, px1, py0, py1 = case
    return (major, (in_h * up_y + py0 + py1 - kh) // down_y + 1, (in_w * up_x + px0 + px1 - kw) // down_x + 1, minor)


def reference_and_bound(x, k, params):
    """(want, bound) of the fp32 entry for fp32 operands x [major, in_h, in_w, minor] and k [kh, kw]; params = the eight factors and pads.

    bound = (kh * kw + 2) * 2^-24 * upfirdn_ref(|x|, |k|), elementwise.  Derived, not measured: every kernel forms an output as ONE chain of
    at most kh * kw fp32 multiply / fma roundings over the taps that meet data, each rounding at most 2^-24 of a partial sum that the sum
    of |k||x| bounds (to first order; the + 2 is the slack the f16 / f64 forms of tests/test_native_ops_entries_gpu.py carry for the second
    order).  The tiled up2 / down2 kernels extend the taps to 4 x 4 with zeros: those terms are exact zeros and round nothing."""
    assert x.dtype == np.float32 and k.dtype == np.float32
    x8, k8 = x.astype(np.float64), k.astype(np.float64)
    want = upfirdn_ref(x8, k8, *params)
    mag = upfirdn_ref(np.abs(x8), np.abs(k8), *params)
    return want, (k.shape[0] * k.shape[1] + 2) * 2.0 ** -24 * mag
