"""GPU: the weight packers (maua_pack_weight_*) through the C ABI, into guarded windows of exactly the documented size.

Every convolution test packs through ModulatedConv2d.packed*() into a torch allocation (rounded up by the allocator) and copies the
result into its guard; a pack that wrote a few floats past its documented size, or left garbage in the padded columns the convolution
kernels read as A operands, would go unnoticed there.

Simple layouts (maua_pack_weight_f32, _wino_f32, _wino43_f32, _upwino_f32): every element written, padded columns exactly 0.0, every
other value equal BIT FOR BIT to a float32 numpy evaluation of the formulas in include/maua_hip.h — single products and short sums whose
only multiplications are by powers of two (exact) or come last, so an fma contraction cannot change a bit; the one exception is wsq, the
sum of nine squares, which the kernel forms as an fma chain: it is compared with the fma chain (each step rounded once, formed in fp64)
and allowed 1 ulp.  The column interleave of the Winograd packs above 32 channels is the header's [o % 32][o / 32 % 2] inside every group
of 64, written out here on its own.

Tile-image layouts (maua_pack_weight_wino2d_f32, _up2d_f32, _sbf16_f32): the layout is the kernels' business and the convolution tests
check it; here the buffer contract (exact windows, all written, red zones intact, MAUA_EINVAL with an untouched window for the refused
shapes), then one minimal convolution from that guarded buffer in modes 5, 6, 7 and 8 against fp64."""
import numpy as np
import pytest
import torch

import conv_ref
from conv_ref import U32, conv_and_magnitude
from maua_stylegan2_amd import _lib
from redzone import Guard

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
_F = np.float32


def pad32(c):
    return (c + 31) // 32 * 32


def wino_pad(c):
    return (c + 63) // 64 * 64 if c > 32 else pad32(c)


def wino_column(o, cout):
    """Destination column of output channel o in the mode 2 / 3 packs: [o % 32][o / 32 % 2] inside its group of 64 above 32 channels."""
    return o if cout <= 32 else (o // 64) * 64 + (o % 32) * 2 + (o // 32) % 2


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def _expect(u_rows, cout, cin, cols, column):
    """[rows, cin, cols] from per-row [cout, cin] float32 arrays; padded columns +0.0."""
    out = np.zeros((len(u_rows), cin, cols), _F)
    for o in range(cout):
        for r, u in enumerate(u_rows):
            out[r, :, column(o, cout)] = u[o]
    return out


@pytest.mark.parametrize("cin", [3, 8, 18])
@pytest.mark.parametrize("cout", [3, 32, 40, 64, 96, 136])
def test_simple_layouts_bit_for_bit(gpu, cout, cin):
    lib = _lib.load()
    st = _lib.stream_ptr(gpu)
    rng = np.random.default_rng(1000 * cout + cin)
    w = rng.standard_normal((cout, cin, 3, 3)).astype(_F)
    g0, g1, g2 = w[..., 0], w[..., 1], w[..., 2]  # [cout, cin, ky]
    ident = lambda o, c: o  # noqa: E731
    g = Guard(gpu)
    w_in = g.inp(w, "w")
    # ---- maua_pack_weight_f32: wp[tap][i][o_pad] = w[o][i][tap], wsq[o][i] = sum over taps of w^2
    p32 = pad32(cout)
    wp, wsq = g.out((9 * cin * p32,), "wp"), g.out((cout * cin,), "wsq")
    wp_only, wsq_only = g.out((9 * cin * p32,), "wp_only"), g.out((cout * cin,), "wsq_only")
    assert lib.maua_pack_weight_f32(w_in.data_ptr(), wp.data_ptr(), wsq.data_ptr(), cout, cin, 9, st) == 0
    assert lib.maua_pack_weight_f32(w_in.data_ptr(), wp_only.data_ptr(), None, cout, cin, 9, st) == 0
    assert lib.maua_pack_weight_f32(w_in.data_ptr(), None, wsq_only.data_ptr(), cout, cin, 9, st) == 0
    # ktaps = 1 (a ToRGB weight [cout, cin, 1, 1]): wp[0][i][o_pad], wsq = w^2
    w1 = np.ascontiguousarray(w[:, :, 0, 0])
    w1_in = g.inp(w1, "w1")
    wp1, wsq1 = g.out((cin * p32,), "wp1"), g.out((cout * cin,), "wsq1")
    assert lib.maua_pack_weight_f32(w1_in.data_ptr(), wp1.data_ptr(), wsq1.data_ptr(), cout, cin, 1, st) == 0
    # ---- the three transformed packs
    pw = wino_pad(cout)
    wq2, wq3, wq4 = g.out((12 * cin * pw,), "wino"), g.out((18 * cin * pw,), "wino43"), g.out((12 * cin * p32,), "upwino")
    assert lib.maua_pack_weight_wino_f32(w_in.data_ptr(), wq2.data_ptr(), cout, cin, st) == 0
    assert lib.maua_pack_weight_wino43_f32(w_in.data_ptr(), wq3.data_ptr(), cout, cin, st) == 0
    assert lib.maua_pack_weight_upwino_f32(w_in.data_ptr(), wq4.data_ptr(), cout, cin, st) == 0
    g.check(written=("wp", "wsq", "wp_only", "wsq_only", "wp1", "wsq1", "wino", "wino43", "upwino"))

    taps = w.reshape(cout, cin, 9)
    want_wp = _expect([taps[:, :, t] for t in range(9)], cout, cin, p32, ident)
    for name, got in (("wp", wp), ("wp_only", wp_only)):
        assert np.array_equal(_bits(got.cpu().numpy()), _bits(want_wp.reshape(-1))), name
    assert np.array_equal(_bits(wp1.cpu().numpy()), _bits(_expect([w1], cout, cin, p32, ident).reshape(-1)))
    ss = np.zeros((cout, cin), np.float64)
    for t in range(9):  # ss = fmaf(v, v, ss): the exact v^2 + ss rounded once
        ss = (taps[:, :, t].astype(np.float64) ** 2 + ss).astype(_F).astype(np.float64)
    for name, got in (("wsq", wsq), ("wsq_only", wsq_only)):
        diff = np.abs(_bits(got.cpu().numpy()).astype(np.int64) - _bits(ss.astype(_F).reshape(-1)).astype(np.int64))
        assert diff.max() <= 1, (name, diff.max())  # (1 ulp: the nine-term fma chain, see the module docstring)
    assert np.array_equal(_bits(wsq1.cpu().numpy()), _bits((w1 * w1).reshape(-1)))

    def rows(fn):  # [cout, cin] arrays per (ky, xi), ky-major
        return [r for ky in range(3) for r in fn(g0[..., ky], g1[..., ky], g2[..., ky])]

    half, six, tf = _F(0.5), _F(1.0) / _F(6.0), _F(1.0) / _F(24.0)
    want2 = _expect(rows(lambda a, b, c: [a, half * ((a + b) + c), half * ((a - b) + c), c]), cout, cin, pw, wino_column)
    want3 = _expect(rows(lambda a, b, c: [a * _F(0.25), -((a + b) + c) * six, -((a - b) + c) * six, ((a + _F(2) * b) + _F(4) * c) * tf,
                                          ((a - _F(2) * b) + _F(4) * c) * tf, c]), cout, cin, pw, wino_column)
    want4 = _expect(rows(lambda a, b, c: [c, a + c, a, b]), cout, cin, p32, ident)
    for name, got, want in (("wino", wq2, want2), ("wino43", wq3, want3), ("upwino", wq4, want4)):
        assert want.dtype == _F
        gb, wb = _bits(got.cpu().numpy()), _bits(want.reshape(-1))
        # (+0.0 in the padding; a transformed value that cancels to -0.0 equals +0.0 numerically: compare such zeros by value)
        same = (gb == wb) | ((got.cpu().numpy() == 0) & (want.reshape(-1) == 0))
        assert same.all(), (name, int((~same).sum()))
        pad_cols = np.ones(want.shape[2], bool)
        pad_cols[[(wino_column if name != "upwino" else ident)(o, cout) for o in range(cout)]] = False
        assert (gb.reshape(want.shape)[:, :, pad_cols] == 0).all(), f"{name}: padded columns must be +0.0 bit for bit"
    assert (_bits(wp.cpu().numpy()).reshape(9, cin, p32)[:, :, cout:] == 0).all()


def test_simple_packers_refuse_bad_arguments(gpu):
    lib = _lib.load()
    g = Guard(gpu)
    w_in, out = g.inp(torch.ones(4, 4, 3, 3), "w"), g.out((18 * 4 * 32,), "out")
    st = _lib.stream_ptr(gpu)
    assert lib.maua_pack_weight_f32(None, out.data_ptr(), None, 4, 4, 9, st) == -22
    assert lib.maua_pack_weight_f32(w_in.data_ptr(), out.data_ptr(), None, 0, 4, 9, st) == -22
    for fn in (lib.maua_pack_weight_wino_f32, lib.maua_pack_weight_wino43_f32, lib.maua_pack_weight_upwino_f32):
        assert fn(w_in.data_ptr(), None, 4, 4, st) == -22 and fn(w_in.data_ptr(), out.data_ptr(), 4, 0, st) == -22
    assert g.untouched("out")
    g.check()


def _weight(rng, cout, cin):
    return torch.from_numpy(rng.standard_normal((1, cout, cin, 3, 3)).astype(np.float32))


TILE_PACKS = [  # (entry, size in bytes, accepted (cout, cin) shapes, refused ones)
    ("maua_pack_weight_wino2d_f32", lambda lib, co, ci: 4 * 24 * ci * co, [(32, 4), (64, 36), (128, 8)], [(32, 6), (48, 8), (96, 8), (40, 8)]),
    ("maua_pack_weight_up2d_f32", lambda lib, co, ci: 4 * lib.maua_pack_weight_up2d_floats(co, ci), [(32, 4), (96, 36)], [(32, 6), (40, 8)]),
    ("maua_pack_weight_sbf16_f32", lambda lib, co, ci: lib.maua_pack_weight_sbf16_bytes(co, ci), [(32, 16), (128, 48)], [(32, 8), (40, 16)]),
]


@pytest.mark.parametrize("entry,size,accepted,refused", TILE_PACKS, ids=[t[0] for t in TILE_PACKS])
def test_tile_image_packers_keep_their_buffer_contract(gpu, entry, size, accepted, refused):
    lib = _lib.load()
    fn = getattr(lib, entry)
    rng = np.random.default_rng(3)
    for cout, cin in accepted:
        g = Guard(gpu)
        n = size(lib, cout, cin)
        assert n > 0 and n % 4 == 0
        w_in, wq = g.inp(_weight(rng, cout, cin)[0], "w"), g.out((n // 4,), "wq")
        assert fn(w_in.data_ptr(), wq.data_ptr(), cout, cin, _lib.stream_ptr(gpu)) == 0
        # (the split-bf16 image holds bf16 pairs, no fp32 values: all-written and red zones only, its finiteness is not defined)
        g.check(written=("wq",), nonfinite_ok=("wq",) if "sbf16" in entry else ())
    for cout, cin in refused:
        g = Guard(gpu)
        w_in, wq = g.inp(_weight(rng, cout, cin)[0], "w"), g.out((24 * cin * cout,), "wq")
        assert fn(w_in.data_ptr(), wq.data_ptr(), cout, cin, _lib.stream_ptr(gpu)) == -22, (entry, cout, cin)
        assert g.untouched("wq")
        g.check()
    assert lib.maua_modconv_w2d_ok(8, 48, 16, 32) == 0 and lib.maua_pack_weight_sbf16_bytes(40, 16) == 0


def _ratio(mode, x, wt):
    """Rounding ratio of mode 5 (F(2x4, 3x3)) / mode 6 (F(2,2) on both axes) on the test's own operands (x [cin, h, w] already scaled by the
    styles, wt [cout, cin, 3, 3]; the amplification at an element depends on the data): the float32 emulations of tests/conv_ref.py
    (transforms, products and channel sums in float32, on the matrices and the index scheme tests/test_winograd_algebra.py proves) against
    fp64, on the CPU: max |emulation - fp64| / (u M).  Mode 6 includes the edge lines (row 2H, column 2W), plain polyphase sums."""
    cin, cout = x.shape[0], wt.shape[0]
    return conv_ref.ratio_of(mode, torch.from_numpy(x)[None], torch.ones(1, cin), torch.ones(1, cout), torch.from_numpy(wt)[None])


def _wino2d_ratio(x, wt):
    return _ratio(5, x, wt)


def _up2d_ratio(x, wt):
    return _ratio(6, x, wt)


# (mode, cin, cout, h, w, batch): the minimum each kernel accepts (modes 7 / 8: cin % 16, cout % 128 / % 32, h % 8, w % 32)
FROM_GUARDED_PACK = [(5, 4, 32, 16, 32, 1), (6, 4, 32, 8, 32, 1), (7, 16, 128, 8, 32, 1), (8, 16, 32, 8, 32, 1)]


@pytest.mark.parametrize("mode,cin,cout,h,w,batch", FROM_GUARDED_PACK)
def test_minimal_convolution_from_the_guarded_pack(gpu, mode, cin, cout, h, w, batch):
    """Modes 5 .. 8 read the packed image the library wrote into an exact-size window.  Bounds per element, M as in
    tests/test_conv_instances_gpu.py:
      mode 5: 4 R u M with R measured here on the CPU by the float32 emulation of F(2x4, 3x3) against fp64 (_wino2d_ratio);
      mode 6: max(4 R, 9 cin + 8) u M, R measured in the same way for F(2,2) on both axes (_up2d_ratio); the second term is the bound of
              modes 0 / 1 for the edge lines (output row 2H, column 2W), which are plain polyphase sums;
      modes 7, 8: the header's product error 2^-16 + 2^-17 relative in place of u for the products, plus the fp32 accumulation:
              ((2^-16 + 2^-17) + (9 cin + 8) u) M."""
    lib = _lib.load()
    up = mode in (6, 8)
    if mode == 7:
        assert lib.maua_modconv_sbf16_ok(cin, cout, h, w)
    if mode == 8:
        assert lib.maua_modconv_sbf16_up_ok(cin, cout, h, w)
    rng = np.random.default_rng(mode)
    f = lambda *shape: torch.from_numpy(rng.standard_normal(shape).astype(np.float32))  # noqa: E731
    stride = cin + 4
    x_, s_, wt = f(batch, cin, h, w), 1 + 0.3 * f(batch, stride), _weight(rng, cout, cin)
    d_ = torch.from_numpy((0.5 + rng.random((batch, cout))).astype(np.float32))
    g = Guard(gpu)
    x, s, d = g.inp(x_, "x"), g.inp(s_, "s"), g.inp(d_, "d")
    entry, size = {5: TILE_PACKS[0], 6: TILE_PACKS[1], 7: TILE_PACKS[2], 8: TILE_PACKS[2]}[mode][:2]
    w_in, wq = g.inp(wt[0], "w"), g.out((size(lib, cout, cin) // 4,), "wq")
    assert getattr(lib, entry)(w_in.data_ptr(), wq.data_ptr(), cout, cin, _lib.stream_ptr(gpu)) == 0
    oh, ow = (2 * h + 1, 2 * w + 1) if up else (h, w)
    y = g.out((batch, cout, oh, ow), "y")
    n_ws = lib.maua_modconv_ws_floats(batch, cin, cout, h, w, mode)
    ws = g.out((n_ws,), "ws") if n_ws else None
    rc = lib.maua_modconv3x3_f32(x.data_ptr(), wq.data_ptr(), s.data_ptr(), stride, d.data_ptr(), y.data_ptr(), batch, cin, cout, h, w, mode,
                                 float(1.0 / np.sqrt(cin * 9)), 0, None, 0, None, None, _lib.ptr(ws), None, 0, _lib.stream_ptr(gpu))
    assert rc == 0, rc
    g.check(written=("y", "wq") + (("ws",) if up else ()), nonfinite_ok=("wq",) if mode >= 7 else ())
    want, mag = conv_and_magnitude(x_, s_[:, :cin], d_, wt, up)
    assert batch == 1
    xs, wnp = (x_ * s_[:, :cin, None, None])[0].numpy(), wt[0].numpy()  # float32: the scaled input the transforms see
    if mode == 5:
        ratio = _wino2d_ratio(xs, wnp)
        assert 1.0 <= ratio <= 500.0, ratio
        bound = 4 * ratio * U32 * mag
    elif mode == 6:
        ratio = _up2d_ratio(xs, wnp)
        assert 1.0 <= ratio <= 500.0, ratio
        bound = max(4 * ratio, 9 * cin + 8) * U32 * mag
    else:
        bound = ((2.0 ** -16 + 2.0 ** -17) + (9 * cin + 8) * U32) * mag
    err = (y.double().cpu() - want).abs()
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"mode {mode}: max |err| {float(err.max()):.3e}, max |err| / bound {worst:.3f}")
    assert bool((err <= bound).all()), worst
