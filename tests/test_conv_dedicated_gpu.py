"""GPU: every kernel instance of csrc/modconv_w2d.hip (mode 5), csrc/modconv_up2d.hip (mode 6, the fused up-sampling layer, the 16-wide
split-K form) and csrc/modconv_sbf16.hip (modes 7 / 8), launched through the C ABI between red zones and compared per element with fp64.

The rows come from tests/golden/conv_dedicated_instances.json (tools/conv_instance_sweep.py --dedicated, on the CPU): shape, batch, the
pre-scaled flag, the instance name maua_modconv_last_instance must report, the workspace size and the rounding ratio R of modes 5 / 6,
measured by the float32 emulations of tests/conv_ref.py on the operands this file feeds (conv_ref.case_operands).

Every case: the weight is packed by the library's own pack entry into a window of exactly the documented size; x, s (s_stride = cin + 5; max(cin, cout) + 5 where post_s shares it),
d, y, ws (exactly the size the library reports), noise, noise_w, bias, post_s and the taps sit between red zones; rc == 0, the reported
name equals the table's, red zones intact, every output element written and finite.

Bounds, per element; u = 2^-24, M = the same convolution over absolute values in fp64 (none is taken from the kernel under test):
  mode 5: 4 R u M;   mode 6: max(4 R, 9 cin + 8) u M (the second term is the plain polyphase bound, which covers the edge lines);
  modes 7 / 8: ((2^-16 + 2^-17) + (9 cin + 8) u) M (tests/test_weight_pack_gpu.py derives it from the header);
  fused tail: sqrt(2) (bound + 4 u (|conv| + |noise_w noise| + |bias|)), as tests/test_conv_instances_gpu.py; post_s: one more rounding;
  through a blur with non-negative taps K (the blur is linear): blur_K(raw bound) + C u blur_K(|raw| + raw bound), then the tail.
    maua_upconv_blur_f32 (separable form, u2_blur_taps): C = 34 roundings on the path of a term —
      3 in a column sum kx[b] (four taps), 20 in a normalised row factor ky[a] = rs[a] * (1 / total) (3 in the row sum, 15 in the total
      of 16 taps, the reciprocal, the product), 4 in the horizontal 4-tap pass (product + three adds), 4 in the vertical one, 3 in the
      gain (wscale * d, * sqrt(2), its product with the blurred value).  With conv_ref.asymmetric_taps() the factors are exact; the
      count holds for any non-negative separable taps.
    maua_upconv_blur_lowres_f32 (general 4 x 4 taps, reduce_blur_tail_kernel): C = 17 — the 16-term fma chain and the product with d;
      split-K: one u M per slab summed."""
import json
import os

import numpy as np
import pytest
import torch

import conv_ref
from conv_ref import U32, case_operands, conv_and_magnitude, upconv_styled64
from maua_stylegan2_amd import _lib
from redzone import CANARY_BITS, Guard
from test_conv_instances_gpu import SQRT2, check_close

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

TABLE = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_dedicated_instances.json")))
ROWS = TABLE["instances"]
SBF16 = 2.0 ** -16 + 2.0 ** -17
C_FUSED, C_LOWRES = 34, 17
EINVAL, ENOSYS = -22, -38


def _id(r):
    return f"{r['entry']}-m{r['mode']}-{r['cin']}-{r['cout']}-{r['h']}x{r['w']}-b{r['batch']}{'-pre' if r['pre'] else ''}"


def row_of(entry, mode, cin, cout, h, w, batch, pre=False):
    got = [r for r in ROWS if (r["entry"], r["mode"], r["cin"], r["cout"], r["h"], r["w"], r["batch"], r["pre"]) == (entry, mode, cin, cout, h, w, batch, pre)]
    assert len(got) == 1, (entry, mode, cin, cout, h, w, batch, pre)
    return got[0]


def pack_dedicated(lib, g, weight, mode, dev):
    """weight [1, cout, cin, 3, 3] -> the packed operand of modes 5 .. 8 in a window of exactly the documented size, written by the library."""
    _, cout, cin = weight.shape[:3]
    if mode == 5:
        fn, n = lib.maua_pack_weight_wino2d_f32, 24 * cin * cout
    elif mode == 6:
        fn, n = lib.maua_pack_weight_up2d_f32, lib.maua_pack_weight_up2d_floats(cout, cin)
    else:
        nb = lib.maua_pack_weight_sbf16_bytes(cout, cin)
        assert nb > 0 and nb % 4 == 0
        fn, n = lib.maua_pack_weight_sbf16_f32, nb // 4
    w_in, wq = g.inp(weight[0], "w"), g.out((n,), "wq")
    assert fn(w_in.data_ptr(), wq.data_ptr(), cout, cin, _lib.stream_ptr(dev)) == 0
    return wq


def raw_bound(row, mag):
    mode, cin = row["mode"], row["cin"]
    if mode == 5:
        return 4.0 * row["R"] * U32 * mag
    if mode == 6:
        return max(4.0 * row["R"], 9 * cin + 8) * U32 * mag
    return (SBF16 + (9 * cin + 8) * U32) * mag


def blur_bound(row, taps, p, splits=0):
    """The bound of an up-sampling layer's activated map before post_s (module docstring), from the parts of conv_ref.upconv_styled64."""
    rb = raw_bound(row, p["mag"]) + splits * U32 * p["mag"]
    blur_abs = lambda a: conv_ref.upfirdn64(a, taps.abs(), up=1, pad=(1, 1))  # noqa: E731
    c = C_LOWRES if row["entry"] == "upconv_blur_lowres" else C_FUSED
    blurred = conv_ref.upfirdn64(p["raw"], taps, up=1, pad=(1, 1))
    return SQRT2 * (blur_abs(rb) + c * U32 * blur_abs(p["raw"].abs() + rb) + 4 * U32 * (blurred.abs() + p["tail"]))


class Noise:
    """The noise operand of a case: None, "image" (one map per image), "shared" (stride 0) or "source" (a frame source, frame0 = 2)."""

    def __init__(self, g, dev, rng, kind, batch, oh, ow):
        self.kind, self.ptr, self.stride, self.src, self.slot, self.keep = kind, None, 0, None, 0, None
        f0 = 2 if kind == "source" else 0
        n = 1 if kind == "shared" else batch + f0
        self.maps = torch.from_numpy(rng.standard_normal((n, 1, oh, ow)).astype(np.float32))
        self.used = self.maps[f0:] if kind else None
        if kind in ("image", "shared"):
            self.ptr, self.stride = g.inp(self.maps, "noise").data_ptr(), oh * ow if kind == "image" else 0
        elif kind == "source":
            src = _lib.FrameSource()
            src.frame0, self.slot = f0, 3
            src.noise[3], src.noise_stride[3] = g.inp(self.maps, "noise").data_ptr(), oh * ow
            self.keep = torch.frombuffer(bytearray(bytes(src)), dtype=torch.uint8).to(dev)
            self.src = self.keep.data_ptr()


def operands(row, d_null):
    rng, x_, s_, d_, wt = case_operands(row["mode"], row["cin"], row["cout"], row["h"], row["w"], row["batch"])
    cin = row["cin"]
    if row["pre"]:  # x is pre-multiplied on the host in fp32; the reference takes that product as its operand
        x_ref, s_ref = conv_ref.prescale(x_, s_[:, :cin].contiguous())
    else:
        x_ref, s_ref = x_, s_[:, :cin].contiguous()
    d_ref = torch.ones_like(d_) if d_null else d_
    return rng, x_ref, s_, s_ref, d_, d_ref, wt


def run_modconv(dev, row, fuse_act=False, noise=None, d_null=False):
    """One guarded maua_modconv3x3_f32 call of a table row compared with fp64."""
    lib = _lib.load()
    mode, cin, cout, h, w, batch = (row[k] for k in ("mode", "cin", "cout", "h", "w", "batch"))
    up = mode in (6, 8)
    rng, x_ref, s_, s_ref, d_, d_ref, wt = operands(row, d_null)
    f = lambda *shape: torch.from_numpy(rng.standard_normal(shape).astype(np.float32))  # noqa: E731
    oh, ow = (2 * h + 1, 2 * w + 1) if up else (h, w)
    bias_, nw_ = 0.3 * f(cout), 0.37
    g = Guard(dev)
    x, y = g.inp(x_ref, "x"), g.out((batch, cout, oh, ow), "y")
    s = None if row["pre"] else g.inp(s_, "s")
    d = None if d_null else g.inp(d_, "d")
    wq = pack_dedicated(lib, g, wt, mode, dev)
    n_ws = lib.maua_modconv_ws_floats(batch, cin, cout, h, w, mode)
    assert n_ws == row["ws_floats"] == (batch * cin * h if up else 0)
    ws = g.out((n_ws,), "ws") if n_ws else None
    nz = Noise(g, dev, rng, noise, batch, oh, ow)
    nw, bias = (g.inp(torch.tensor([nw_]), "noise_w"), g.inp(bias_, "bias")) if fuse_act else (None, None)
    rc = lib.maua_modconv3x3_f32(x.data_ptr(), wq.data_ptr(), _lib.ptr(s), s_.shape[1], _lib.ptr(d), y.data_ptr(), batch, cin, cout, h, w, mode,
                                 float(1.0 / np.sqrt(cin * 9)), int(fuse_act), nz.ptr, nz.stride, _lib.ptr(nw), _lib.ptr(bias), _lib.ptr(ws),
                                 nz.src, nz.slot, _lib.stream_ptr(dev))
    assert rc == 0, rc
    name = _lib.last_modconv_instance()
    assert name == row["name"], f"{_id(row)} now runs {name}, the table says {row['name']}"
    g.check(written=("y", "wq") + (("ws",) if up else ()), nonfinite_ok=("wq",) if mode >= 7 else ())
    if up:  # csrc/modconv_up2d.hip: xcol [B][Cin][H] = the last input column (of x as it is fed, before the style), bit for bit
        assert torch.equal(ws.cpu().view(batch, cin, h), x_ref[:, :, :, w - 1]), "the exported last input column"
    want, mag = conv_and_magnitude(x_ref, s_ref, d_ref, wt, up)  # (the edge lines — row 2H, column 2W, the corner — are part of the map)
    bound = raw_bound(row, mag)
    if fuse_act:
        nzt = (float(np.float32(nw_)) * nz.used.double()) if noise else torch.zeros(1, 1, oh, ow, dtype=torch.float64)
        bt = bias_.double()[None, :, None, None]
        bound = SQRT2 * (bound + 4 * U32 * (want.abs() + nzt.abs() + bt.abs()))
        t = want + nzt + bt
        want = torch.where(t > 0, t, 0.2 * t) * SQRT2
    check_close(y, want, bound, f"{name} {_id(row)} fuse_act {int(fuse_act)} noise {noise}")


def run_upconv_blur(dev, row, taps, noise="image", d_null=False, post=True, with_ws=True):
    """One guarded maua_upconv_blur_f32 / maua_upconv_blur_lowres_f32(up = 6) call of a table row compared with fp64."""
    lib = _lib.load()
    cin, cout, h, w, batch = (row[k] for k in ("cin", "cout", "h", "w", "batch"))
    lowres = row["entry"] == "upconv_blur_lowres"
    rng, x_ref, s_, s_ref, d_, d_ref, wt = operands(row, d_null)
    f = lambda *shape: torch.from_numpy(rng.standard_normal(shape).astype(np.float32))  # noqa: E731
    stride = max(cin, cout) + 5  # (post_s shares the stride of s and is indexed by the output channel)
    s_ = torch.cat([s_[:, :cin], 1 + 0.3 * f(batch, stride - cin)], 1)
    bias_, nw_, post_ = 0.3 * f(cout), 0.37, 1 + 0.3 * f(batch, stride)
    assert bool((taps >= 0).all())
    g = Guard(dev)
    x, y = g.inp(x_ref, "x"), g.out((batch, cout, 2 * h, 2 * w), "y")
    s = None if row["pre"] else g.inp(s_, "s")
    d = None if d_null else g.inp(d_, "d")
    k4, nw, bias = g.inp(taps, "k4"), g.inp(torch.tensor([nw_]), "noise_w"), g.inp(bias_, "bias")
    ps = g.inp(post_, "post_s") if post else None
    wq = pack_dedicated(lib, g, wt, 6, dev)
    nz = Noise(g, dev, rng, noise, batch, 2 * h, 2 * w)
    wscale = float(1.0 / np.sqrt(cin * 9))
    slab = batch * cout * (2 * h + 1) * (2 * w + 1)
    if lowres:
        assert lib.maua_lowres_ok(cin, cout, h, w, 6) == 1
        n_ws = lib.maua_lowres_ws_floats(batch, cin, cout, h, w, 6)
        splits, rem = divmod(n_ws - batch * cin * h, slab)  # slabs + the exported last input column
        assert rem == 0 and n_ws == row["ws_floats"]
        ws = g.out((n_ws,), "ws")
        rc = lib.maua_upconv_blur_lowres_f32(x.data_ptr(), wq.data_ptr(), s.data_ptr(), stride, _lib.ptr(d), y.data_ptr(), ws.data_ptr(), k4.data_ptr(),
                                             nz.ptr, nz.stride, nw.data_ptr(), bias.data_ptr(), nz.src, nz.slot, batch, cin, cout, h, w, 6, wscale,
                                             _lib.ptr(ps), _lib.stream_ptr(dev))
    else:
        assert lib.maua_upconv_blur_ok(cin, cout, h, w) == 1
        n_ws = lib.maua_upconv_blur_ws_floats(batch, cin, cout, h, w)
        n_seg, rem = divmod(n_ws - 4, batch * cout * 12 * w)
        n_seg += 1
        assert rem == 0 and n_ws == row["ws_floats"]
        splits = 0
        ws = g.out((n_ws,), "ws")
        rc = lib.maua_upconv_blur_f32(x.data_ptr(), wq.data_ptr(), _lib.ptr(s), stride, _lib.ptr(d), y.data_ptr(), ws.data_ptr() if with_ws else None,
                                      k4.data_ptr(), nz.ptr, nz.stride, nw.data_ptr(), bias.data_ptr(), nz.src, nz.slot, batch, cin, cout, h, w,
                                      wscale, _lib.ptr(ps), _lib.stream_ptr(dev))
        if not with_ws:
            assert n_seg > 1 and rc == EINVAL and g.untouched("y") and g.untouched("ws")
            g.check()
            return n_seg
    assert rc == 0, rc
    name = _lib.last_modconv_instance()
    assert name == row["name"], f"{_id(row)} now runs {name}, the table says {row['name']}"
    g.check(written=("y", "wq"))
    if lowres:
        # csrc/modconv_up2d.hip: `splits` slabs [B][Cout][2H+1][2W+1], the edge lines (row 2H, column 2W) in slab 0 only, then xcol
        stale = (ws.view(torch.int32)[:splits * slab].cpu() == CANARY_BITS).view(splits, batch, cout, 2 * h + 1, 2 * w + 1)
        assert not bool(stale[0].any()) and not bool(stale[:, :, :, :2 * h, :2 * w].any()), "slab elements never written"
        assert bool(stale[1:, :, :, 2 * h, :].all()) and bool(stale[1:, :, :, :, 2 * w].all()), "the edge lines belong to slab 0 alone"
        assert bool(torch.isfinite(ws[:slab]).all())
        assert torch.equal(ws[splits * slab:].cpu().view(batch, cin, h), x_ref[:, :, :, w - 1]), "the exported last input column"
    nzt = (float(np.float32(nw_)) * nz.used.double()) if noise else None
    pv = post_[:, :cout] if post else None
    want, p = upconv_styled64(x_ref, s_ref, d_ref, wt, taps, nzt, bias_, pv)
    bound = blur_bound(row, taps, p, splits)
    if post:
        bound = pv.double().abs()[:, :, None, None] * bound + U32 * want.abs()
    check_close(y, want, bound, f"{name} {_id(row)} noise {noise} post {int(post)} splits {splits}")
    return splits if lowres else n_seg


MODCONV_ROWS = [r for r in ROWS if r["entry"] == "modconv3x3"]
BLUR_ROWS = [r for r in ROWS if r["entry"] != "modconv3x3"]


@pytest.mark.parametrize("row", MODCONV_ROWS, ids=_id)
def test_every_dedicated_instance_against_fp64(gpu, row):
    """Modes 5 .. 8 through maua_modconv3x3_f32, raw map (mode 7's larger row: the fused tail with per-image noise, as the table says)."""
    fused = row["mode"] == 7 and row["batch"] > 1
    run_modconv(gpu, row, fuse_act=fused, noise="image" if fused else None)


@pytest.mark.parametrize("row", BLUR_ROWS, ids=_id)
def test_up_sampling_layers_with_asymmetric_taps_against_fp64(gpu, row):
    """The fused layer with exactly separable taps of two different non-palindromic factors, the low-resolution entry (which documents
    general 4 x 4 taps) with those taps plus a non-separable term; segment / split counts asserted from the reported workspace sizes."""
    taps = conv_ref.asymmetric_taps()
    if row["entry"] == "upconv_blur_lowres":
        taps = taps.clone()
        taps[0, 1] += 0.125
        taps[2, 3] += 0.0625
        splits = run_upconv_blur(gpu, row, taps)
        assert splits == {8: 1, 72: 2, 136: 4}[row["cin"]]
    else:
        n_seg = run_upconv_blur(gpu, row, taps)
        assert (n_seg > 1) == (row["h"] > 8), n_seg


def test_fused_layer_keeps_the_default_taps(gpu):
    from maua_stylegan2_amd import seeding

    run_upconv_blur(gpu, row_of("upconv_blur", 6, 8, 32, 8, 32, 1), torch.from_numpy(seeding.fir_kernel_2d((1, 3, 3, 1), 4.0)).float())


SMALL5 = [row_of("modconv3x3", 5, 4, 64, 8, 32, 1), row_of("modconv3x3", 5, 4, 32, 8, 32, 1), row_of("modconv3x3", 5, 4, 32, 16, 32, 1),
          row_of("modconv3x3", 5, 4, 32, 16, 32, 1, True), row_of("modconv3x3", 5, 12, 128, 16, 64, 3)]
SMALL6 = [row_of("modconv3x3", 6, 4, 32, 8, 32, 1), row_of("modconv3x3", 6, 8, 32, 8, 32, 1), row_of("modconv3x3", 6, 12, 64, 16, 64, 2)]
SMALL78 = [row_of("modconv3x3", 7, 16, 128, 8, 32, 1), row_of("modconv3x3", 8, 16, 32, 8, 32, 1)]


@pytest.mark.parametrize("noise", [None, "image", "shared", "source"])
@pytest.mark.parametrize("row", SMALL5 + SMALL78[:1], ids=_id)
def test_fused_tail_and_noise_sources_on_the_plain_kernels(gpu, row, noise):
    run_modconv(gpu, row, fuse_act=True, noise=noise)


@pytest.mark.parametrize("row", SMALL5[:3] + SMALL6 + SMALL78, ids=_id)
def test_without_demodulation(gpu, row):
    run_modconv(gpu, row, d_null=True)


@pytest.mark.parametrize("noise,d_null,post", [(None, False, False), ("shared", True, True), ("source", False, True)])
@pytest.mark.parametrize("row", [r for r in BLUR_ROWS if r["batch"] > 1 and r["cin"] <= 72], ids=_id)
def test_up_sampling_layer_variants(gpu, row, noise, d_null, post):
    run_upconv_blur(gpu, row, conv_ref.asymmetric_taps(), noise=noise, d_null=d_null, post=post)


def test_several_segments_need_their_workspace(gpu):
    run_upconv_blur(gpu, row_of("upconv_blur", 6, 8, 32, 32, 32, 3), conv_ref.asymmetric_taps(), with_ws=False)


# (mode, cin, cout, h, w, fuse_act): outside maua_modconv_w2d_ok / maua_modconv_up2d_ok, and fuse_act on the raw-output modes
REFUSED = [(5, 6, 64, 8, 32, 0), (5, 8, 48, 16, 32, 0), (5, 8, 96, 16, 32, 0), (5, 8, 64, 8, 48, 0), (5, 8, 64, 12, 32, 0), (6, 6, 32, 8, 32, 0),
           (6, 8, 48, 8, 32, 0), (6, 8, 32, 8, 48, 0), (6, 8, 32, 12, 32, 0), (6, 8, 32, 8, 32, 1), (8, 16, 32, 8, 32, 1)]


@pytest.mark.parametrize("mode,cin,cout,h,w,fuse_act", REFUSED)
def test_refused_shapes_launch_nothing(gpu, mode, cin, cout, h, w, fuse_act):
    lib = _lib.load()
    if not fuse_act:
        assert (lib.maua_modconv_w2d_ok if mode == 5 else lib.maua_modconv_up2d_ok)(cin, cout, h, w) == 0
    up = mode in (6, 8)
    g = Guard(gpu)
    x, s = g.inp(torch.ones(1, cin, h, w), "x"), g.inp(torch.ones(1, cin), "s")
    wq = g.inp(torch.ones(30 * cin * cout), "wq")
    y = g.out((1, cout, 2 * h + 1, 2 * w + 1) if up else (1, cout, h, w), "y")
    ws, nw, bias = g.out((cin * h,), "ws"), g.inp(torch.ones(1), "noise_w"), g.inp(torch.ones(cout), "bias")
    rc = lib.maua_modconv3x3_f32(x.data_ptr(), wq.data_ptr(), s.data_ptr(), cin, None, y.data_ptr(), 1, cin, cout, h, w, mode, 0.1, fuse_act, None, 0,
                                 nw.data_ptr(), bias.data_ptr(), ws.data_ptr(), None, 0, _lib.stream_ptr(gpu))
    assert rc == EINVAL, rc
    assert g.untouched("y") and g.untouched("ws")
    g.check()


@pytest.mark.parametrize("cin,cout,h,w", [(12, 32, 8, 32), (264, 32, 8, 32), (8, 48, 8, 32), (8, 32, 8, 48), (8, 32, 12, 32)])
def test_fused_layer_refuses_shapes_outside_its_predicate(gpu, cin, cout, h, w):
    lib = _lib.load()
    assert lib.maua_upconv_blur_ok(cin, cout, h, w) == 0 and lib.maua_upconv_blur_ws_floats(1, cin, cout, h, w) == 0
    g = Guard(gpu)
    x, s, k4 = g.inp(torch.ones(1, cin, h, w), "x"), g.inp(torch.ones(1, cin), "s"), g.inp(conv_ref.asymmetric_taps(), "k4")
    wq, y, ws = g.inp(torch.ones(21 * cin * cout), "wq"), g.out((1, cout, 2 * h, 2 * w), "y"), g.out((cout * 12 * w + 4,), "ws")
    rc = lib.maua_upconv_blur_f32(x.data_ptr(), wq.data_ptr(), s.data_ptr(), cin, None, y.data_ptr(), ws.data_ptr(), k4.data_ptr(), None, 0, None, None,
                                  None, 0, 1, cin, cout, h, w, 0.1, None, _lib.stream_ptr(gpu))
    assert rc == ENOSYS, rc
    assert g.untouched("y") and g.untouched("ws")
    g.check()


def _torgb_case(gpu, cin, cout, h, w, batch, partial=False, skip=False, u8=False, store=True, post=False):
    """maua_styledconv_torgb_f32 / _partial_f32 in mode 5.  Feature map: the bound of the fused tail (R measured here on the CPU for this
    shape's operands).  Image: the ToRGB of the fp64 feature map in fp64; bound = sum_o |w_o| bound_o + (cout + 12) u sum of the absolute
    terms, as tests/test_conv_instances_gpu.py states it.  The skip is up-sampled with general asymmetric 4 x 4 taps."""
    lib = _lib.load()
    rng, x_, s_cin, d_, wt = case_operands(5, cin, cout, h, w, batch)
    f = lambda *shape: torch.from_numpy(rng.standard_normal(shape).astype(np.float32))  # noqa: E731
    stride = max(cin, cout) + 3
    s_ = torch.cat([s_cin[:, :cin], 1 + 0.3 * f(batch, stride - cin)], 1)
    nz_, bias_, nw_, post_ = f(batch, 1, h, w), 0.3 * f(cout), 0.2, 1 + 0.3 * f(batch, stride)
    rgb_w_, rgb_s_, rgb_b_, skip_ = f(3, cout), 1 + 0.3 * f(batch, stride), 0.3 * f(3), f(batch, 3, h // 2, w // 2)
    taps = 4.0 * conv_ref.asymmetric_taps()
    taps[1, 2] += 0.25  # (general taps: not an outer product)
    mt = lib.maua_modconv_w2d_mtiles(cin, cout, h, w)
    g = Guard(gpu)
    x, s, d = g.inp(x_, "x"), g.inp(s_, "s"), g.inp(d_, "d")
    nz, nw, bias = g.inp(nz_, "noise"), g.inp(torch.tensor([nw_]), "noise_w"), g.inp(bias_, "bias")
    rgb_w, rgb_s, rgb_b = g.inp(rgb_w_, "rgb_w"), g.inp(rgb_s_, "rgb_s"), g.inp(rgb_b_, "rgb_bias")
    sk, k4 = (g.inp(skip_, "skip"), g.inp(taps, "k4")) if skip else (None, None)
    ps = g.inp(post_, "post_s") if post else None
    wq = pack_dedicated(lib, g, wt, 5, gpu)
    y, img = g.out((batch, cout, h, w), "y"), g.out((batch, 3 * mt if partial else 3, h, w), "rgb")
    frames = g.out((batch, h, w, 3), "frames", dtype=torch.uint8) if u8 else None
    wscale = float(1.0 / np.sqrt(cin * 9))
    if partial:
        rc = lib.maua_styledconv_torgb_partial_f32(x.data_ptr(), wq.data_ptr(), s.data_ptr(), stride, d.data_ptr(), y.data_ptr(), batch, cin, cout, h, w,
                                                   5, wscale, nz.data_ptr(), h * w, nw.data_ptr(), bias.data_ptr(), rgb_w.data_ptr(), rgb_s.data_ptr(),
                                                   0.1, img.data_ptr(), None, 0, _lib.ptr(ps), _lib.stream_ptr(gpu))
    else:
        rc = lib.maua_styledconv_torgb_f32(x.data_ptr(), wq.data_ptr(), s.data_ptr(), stride, d.data_ptr(), y.data_ptr(), batch, cin, cout, h, w, 5,
                                           wscale, nz.data_ptr(), h * w, nw.data_ptr(), bias.data_ptr(), rgb_w.data_ptr(), rgb_s.data_ptr(), 0.1,
                                           rgb_b.data_ptr(), _lib.ptr(sk), _lib.ptr(k4), img.data_ptr(), int(store), _lib.ptr(frames), None, 0,
                                           _lib.ptr(ps), _lib.stream_ptr(gpu))
    assert rc == 0, rc
    name = _lib.last_modconv_instance()
    g.check(written=("rgb", "wq") + (("y",) if store else ()) + (("frames",) if u8 else ()), nonfinite_ok=("frames",))
    if not store:
        assert g.untouched("y")
    conv, mag = conv_and_magnitude(x_, s_[:, :cin], d_, wt, False)
    ratio = conv_ref.rounding_ratio(5, cin, cout, h, w, batch)
    assert 1.0 <= ratio <= 500.0
    nzt, bt = float(np.float32(nw_)) * nz_.double(), bias_.double()[None, :, None, None]
    fbound = SQRT2 * (4 * ratio * U32 * mag + 4 * U32 * (conv.abs() + nzt.abs() + bt.abs()))
    t = conv + nzt + bt
    feat = torch.where(t > 0, t, 0.2 * t) * SQRT2
    what = f"{name} torgb {cin}->{cout} {h}x{w} partial {int(partial)} skip {int(skip)} u8 {int(u8)} store {int(store)} post {int(post)}"
    if store:
        pv = post_.double()[:, :cout, None, None] if post else torch.ones(1, 1, 1, 1, dtype=torch.float64)
        check_close(y, feat * pv, pv.abs() * fbound + (U32 * (feat * pv).abs() if post else 0.0), "feature map, " + what)
    mw = float(np.float32(0.1)) * rgb_w_.double()[None] * rgb_s_.double()[:, None, :cout]  # [B, 3, cout]
    want = torch.einsum("bco,bohw->bchw", mw, feat)
    absum = torch.einsum("bco,bohw->bchw", mw.abs(), feat.abs())
    if not partial:
        want, absum = want + rgb_b_.double()[None, :, None, None], absum + rgb_b_.double().abs()[None, :, None, None]
    if skip:
        want = want + conv_ref.upfirdn64(skip_, taps, up=2, pad=(2, 1))
        absum = absum + conv_ref.upfirdn64(skip_.abs(), taps.abs(), up=2, pad=(2, 1))
    ibound = torch.einsum("bco,bohw->bchw", mw.abs(), fbound) + (cout + 12) * U32 * absum
    got = img.view(batch, mt, 3, h, w).sum(1) if partial else img
    check_close(got, want, ibound, "image, " + what)
    if u8:
        q = ((img.clamp(-1, 1) + 1) * 127.5).to(torch.uint8).permute(0, 2, 3, 1)
        assert int((frames.int() - q.int()).abs().max()) <= 1  # (the kernel converts the same registers; a float tie may fall either way)
    return name


TORGB5 = {"general-32": (4, 32, 8, 32, "modconv_w2d_kernel<2, 2, 3, false>"), "wave-complete-32": (4, 32, 16, 32, "modconv_w2dw_kernel<false>"),
          "64": (4, 64, 8, 32, "modconv_w2d_kernel<4, 2, 2, false>")}


@pytest.mark.parametrize("skip,u8,store,post", [(False, False, True, False), (True, False, True, True), (True, True, False, False)])
@pytest.mark.parametrize("kernel", list(TORGB5))
def test_fused_torgb_on_every_single_m_tile_instance(gpu, kernel, skip, u8, store, post):
    cin, cout, h, w, name = TORGB5[kernel]
    assert _torgb_case(gpu, cin, cout, h, w, 2, skip=skip, u8=u8, store=store, post=post) == name


@pytest.mark.parametrize("cout,h,name", [(128, 8, "modconv_w2d_kernel<4, 2, 2, false>"), (192, 8, "modconv_w2d_kernel<4, 2, 2, false>"),
                                         (32, 16, "modconv_w2d_kernel<2, 2, 3, false>")])
def test_partial_torgb_sums(gpu, cout, h, name):
    """cout 32 at h = 16 must stay on the general kernel: the wave-complete one has no partial ToRGB mode."""
    assert _torgb_case(gpu, 4, cout, h, 32, 2, partial=True, post=cout == 128) == name


def test_torgb_refusals_launch_nothing(gpu):
    """Full ToRGB on more than one m-tile and a skip without taps: MAUA_ENOSYS, y and the image untouched."""
    lib = _lib.load()
    for cout, with_skip in ((128, False), (64, True)):
        cin, h, w = 4, 8, 32
        g = Guard(gpu)
        one = lambda *shape: g.inp(torch.ones(*shape), "in")  # noqa: E731
        x, s, d, wq, nw, bias = one(1, cin, h, w), one(1, cout), one(1, cout), one(24 * cin * cout), one(1), one(cout)
        rgb_w, rgb_s, rgb_b, sk = one(3, cout), one(1, cout), one(3), one(1, 3, h // 2, w // 2)
        y, img = g.out((1, cout, h, w), "y"), g.out((1, 3, h, w), "rgb")
        rc = lib.maua_styledconv_torgb_f32(x.data_ptr(), wq.data_ptr(), s.data_ptr(), cout, d.data_ptr(), y.data_ptr(), 1, cin, cout, h, w, 5, 0.1, None, 0,
                                           nw.data_ptr(), bias.data_ptr(), rgb_w.data_ptr(), rgb_s.data_ptr(), 0.1, rgb_b.data_ptr(),
                                           sk.data_ptr() if with_skip else None, None, img.data_ptr(), 1, None, None, 0, None, _lib.stream_ptr(gpu))
        assert rc == ENOSYS, rc
        assert g.untouched("y") and g.untouched("rgb")
        g.check()
