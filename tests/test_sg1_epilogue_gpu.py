"""GPU: maua_sg1_epilogue_f32 (csrc/stylegan1.hip) through the C ABI against the five-module chain of the StyleGAN1 LayerEpilogue.

Reference: the chain in torch on the CPU in float64 — bias and weighted-noise add, leaky_relu(0.2), instance_norm (biased variance,
eps 1e-5), x * (s0 + 1) + s1.  Tolerance: nothing fixed; the same chain in torch CPU float32 is measured against float64 and the kernel
may be at most  4 * err_torch_fp32 + 16 * 2^-24 * max|want|  away (the factor 4: another summation order — 256 strided partial sums and
a tree here, torch's own order there).  Every operand and the output sit between red zones (tests/redzone.py)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from maua_stylegan2_amd import _lib
from redzone import Guard

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

U = 2.0 ** -24
EINVAL = -22
SHAPES = [(1, 1, 1, 1), (2, 3, 4, 4), (1, 2, 15, 17), (1, 2, 16, 16), (2, 2, 1, 257), (1, 5, 25, 40), (2, 4, 64, 64), (1, 2, 128, 128)]
COMBOS = [(b, n, s, i) for b in (False, True) for n in (False, True) for s in (False, True) for i in (0, 1)]


def _chain(x, bias, noise, noise_w, style, channels, instance_norm, dtype):
    """The five modules on the CPU in ``dtype``; absent operands (None) are skipped as the kernel skips them."""
    v = x.to(dtype)
    if bias is not None:
        v = v + bias.to(dtype).view(1, -1, 1, 1)
    if noise is not None:
        v = v + noise_w.to(dtype).view(1, -1, 1, 1) * noise.to(dtype)
    v = F.leaky_relu(v, 0.2)
    if instance_norm:
        if v.shape[2] * v.shape[3] > 1:
            v = F.instance_norm(v, eps=1e-5)
        else:  # (F.instance_norm refuses a single spatial element; its formula with the biased variance of one value, 0)
            v = (v - v.mean((2, 3), keepdim=True)) / torch.sqrt(v.var((2, 3), unbiased=False, keepdim=True) + 1e-5)
    if style is not None:
        st = style.to(dtype)
        v = v * (st[:, :channels, None, None] + 1) + st[:, channels:2 * channels, None, None]
    return v


def _operands(shape, with_bias, with_noise, with_style, noise_batch, style_stride, seed, x=None):
    batch, channels, h, w = shape
    r = np.random.default_rng(seed)
    f = lambda *s: torch.from_numpy(r.standard_normal(s).astype(np.float32))  # noqa: E731
    ops = dict(x=f(batch, channels, h, w) if x is None else x, bias=0.5 * f(channels) if with_bias else None,
               noise=f(noise_batch, 1, h, w) if with_noise else None, noise_w=0.7 * f(channels), style=None, style_stride=0)
    if with_style:
        stride = style_stride or 2 * channels
        ops["style_row"] = f(batch, stride)  # (columns beyond 2C belong to other layers: finite, never read into this result)
        ops["style"], ops["style_stride"] = ops["style_row"][:, :2 * channels], stride
    return ops


def _launch(gpu, shape, ops, instance_norm, in_place=False, noise_w_null=False):
    """One guarded call; returns (rc, guard, y)."""
    lib = _lib.load()
    batch, channels, h, w = shape
    g = Guard(gpu)
    bias = g.inp(ops["bias"], "bias") if ops["bias"] is not None else None
    noise = g.inp(ops["noise"], "noise") if ops["noise"] is not None else None
    nw = None if noise_w_null else g.inp(ops["noise_w"], "noise_w")
    style = g.inp(ops["style_row"], "style") if ops["style"] is not None else None
    nstride = 0 if noise is None or ops["noise"].shape[0] == 1 else h * w
    if in_place:
        y = x = g.out(shape, "y")
        x.copy_(ops["x"])
    else:
        x, y = g.inp(ops["x"], "x"), g.out(shape, "y")
    rc = lib.maua_sg1_epilogue_f32(x.data_ptr(), _lib.ptr(bias), _lib.ptr(noise), nstride, _lib.ptr(nw), _lib.ptr(style), ops["style_stride"],
                                   y.data_ptr(), batch, channels, h, w, instance_norm, _lib.stream_ptr(gpu))
    return rc, g, y


def _assert_close(y, shape, ops, instance_norm, label):
    channels = shape[1]
    args = (ops["x"], ops["bias"], ops["noise"], ops["noise_w"], ops["style"], channels, instance_norm)
    want = _chain(*args, torch.float64)
    err_torch = float((_chain(*args, torch.float32).double() - want).abs().max())
    err = float((y.cpu().double() - want).abs().max())
    bound = 4 * err_torch + 16 * U * float(want.abs().max())
    print(f"[sg1_epilogue] {label}: err_kernel {err:.3e} err_torch_fp32 {err_torch:.3e} ratio {err / err_torch if err_torch else float('nan'):.2f} "
          f"bound {bound:.3e} ({err / bound:.3f} of it)")
    assert err <= bound, (label, err, err_torch, bound)
    return want, bound


@pytest.mark.parametrize("shape", SHAPES)
def test_epilogue_shapes_against_the_float64_chain(gpu, shape):
    """Every operand present, per-sample noise: planes of 1 (variance 0), 16, 255, 256, 257, 1000, 4096 and 16384 elements."""
    ops = _operands(shape, True, True, True, shape[0], 0, sum(shape))
    rc, g, y = _launch(gpu, shape, ops, 1)
    assert rc == 0, rc
    g.check(written=("y",))
    _assert_close(y, shape, ops, 1, f"shape {shape}")


@pytest.mark.parametrize("shape", [(1, 2, 15, 17), (2, 3, 4, 4)])
@pytest.mark.parametrize("with_bias,with_noise,with_style,instance_norm", COMBOS)
def test_epilogue_operand_combinations(gpu, shape, with_bias, with_noise, with_style, instance_norm):
    """Each of bias / noise / style NULL or given, with and without the normalisation."""
    ops = _operands(shape, with_bias, with_noise, with_style, shape[0], 0, 7 + 8 * with_bias + 4 * with_noise + 2 * with_style + instance_norm)
    rc, g, y = _launch(gpu, shape, ops, instance_norm)
    assert rc == 0, rc
    g.check(written=("y",))
    _assert_close(y, shape, ops, instance_norm, f"shape {shape} bias {with_bias} noise {with_noise} style {with_style} norm {instance_norm}")


@pytest.mark.parametrize("shape", [(2, 3, 4, 4), (2, 2, 1, 257)])
def test_epilogue_noise_strides_style_stride_and_in_place(gpu, shape):
    """One shared noise map (stride 0) against one map per sample (stride = plane); a styles row wider than 2C; y == x gives the bits of
    the out-of-place call."""
    batch, channels = shape[:2]
    for noise_batch in (1, batch):
        ops = _operands(shape, True, True, True, noise_batch, 2 * channels + 5, 31 + noise_batch)
        rc, g, y = _launch(gpu, shape, ops, 1)
        assert rc == 0, rc
        g.check(written=("y",))
        _assert_close(y, shape, ops, 1, f"shape {shape} noise_batch {noise_batch} style_stride {2 * channels + 5}")
        rc, g2, y2 = _launch(gpu, shape, ops, 1, in_place=True)
        assert rc == 0, rc
        g2.check(written=("y",))
        assert torch.equal(y, y2)


def _numpy_fp32_variance_model(v, s0_plus_1, s1, one_pass):
    """The kernel's arithmetic for one plane of a multiple of 256 values in numpy float32: 256 strided partial sums, the wave64 butterfly,
    the four wave sums in order; ``one_pass``: E[v^2] - mean^2 instead of the centred second moment."""
    f32 = np.float32
    fma = lambda a, b, c: (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(f32)  # noqa: E731

    def block_sum(s):
        idx = np.arange(256)
        for off in (32, 16, 8, 4, 2, 1):
            s = (s + s[idx ^ off]).astype(f32)
        return f32(f32(f32(s[0] + s[64]) + s[128]) + s[192])

    rows = v.reshape(-1, 256)
    s1_, s2 = np.zeros(256, f32), np.zeros(256, f32)
    for row in rows:
        s1_ = (s1_ + row).astype(f32)
    mean = f32(block_sum(s1_) / f32(v.size))
    for row in rows:
        d = row if one_pass else (row - mean).astype(f32)
        s2 = fma(d, d, s2)
    var = f32(block_sum(s2) / f32(v.size))
    if one_pass:
        var = f32(var - f32(mean * mean))
    with np.errstate(invalid="ignore"):
        gain = f32(f32(1) / np.sqrt(f32(var + f32(1e-5)), dtype=f32) * s0_plus_1)
    return fma((v - mean).astype(f32), np.full_like(v, gain), np.full_like(v, s1))


def test_epilogue_variance_is_two_pass(gpu):
    """x = 100 + 0.01 N(0,1) on 128 x 128 planes: mean^2 is 1e8 times the variance, so E[v^2] - mean^2 in fp32 has no correct digit left
    while the centred second moment keeps all of them.  Checked on the CPU (below, on the same data): the numpy fp32 model of this kernel
    with a ONE-pass variance misses the bound by more than 100x (measured: about 4000x, or it is not finite), the two-pass model stays
    below it (measured: 0.16 of the bound) — so this case fails for a one-pass kernel and passes for the committed two-pass one."""
    shape = (1, 2, 128, 128)
    r = np.random.default_rng(5)
    x = torch.from_numpy((100 + 0.01 * r.standard_normal(shape)).astype(np.float32))
    ops = _operands(shape, False, False, True, 1, 0, 6, x=x)
    rc, g, y = _launch(gpu, shape, ops, 1)
    assert rc == 0, rc
    g.check(written=("y",))
    want, bound = _assert_close(y, shape, ops, 1, "conditioning case")
    st = ops["style"].numpy()
    for c in range(2):
        plane, ref = x[0, c].numpy().reshape(-1), want[0, c].numpy().reshape(-1)
        two = _numpy_fp32_variance_model(plane, np.float32(st[0, c] + np.float32(1)), st[0, 2 + c], False)
        one = _numpy_fp32_variance_model(plane, np.float32(st[0, c] + np.float32(1)), st[0, 2 + c], True)
        err_one = float(np.abs(one - ref).max()) if np.isfinite(one).all() else float("inf")
        print(f"[sg1_epilogue] conditioning, channel {c}: two-pass model {float(np.abs(two - ref).max()) / bound:.3f} of the bound, "
              f"one-pass model {err_one / bound:.0f}x the bound")
        assert float(np.abs(two - ref).max()) <= bound
        assert err_one > 100 * bound


def test_epilogue_refusals_leave_the_output_untouched(gpu):
    lib = _lib.load()
    shape = (2, 3, 4, 4)
    ops = _operands(shape, True, True, True, 2, 0, 99)
    rc, g, y = _launch(gpu, shape, ops, 1, noise_w_null=True)  # noise without noise_w
    assert rc == EINVAL and g.untouched("y")
    g = Guard(gpu)
    x, y = g.inp(ops["x"], "x"), g.out(shape, "y")
    st = _lib.stream_ptr(gpu)

    def call(x_, y_, batch, channels):
        return lib.maua_sg1_epilogue_f32(x_, None, None, 0, None, None, 0, y_, batch, channels, 4, 4, 1, st)

    assert call(x.data_ptr(), y.data_ptr(), 0, 3) == EINVAL
    assert call(x.data_ptr(), y.data_ptr(), 65536, 3) == EINVAL  # (the batch is a grid's y dimension)
    assert call(x.data_ptr(), y.data_ptr(), 2, 0) == EINVAL
    assert call(None, y.data_ptr(), 2, 3) == EINVAL
    assert call(x.data_ptr(), None, 2, 3) == EINVAL
    assert g.untouched("y")
    g.check()
