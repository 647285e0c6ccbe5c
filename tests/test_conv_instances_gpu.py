"""GPU: every instance of modconv_mfma_kernel<BM, BN, WM, MODE, MULTI, FAST, MAXP> (csrc/modconv_kernel.h, instantiated by csrc/modconv_m0.hip .. modconv_m4.hip) a call can reach, launched through
the C ABI at the smallest shape that reaches it, between red zones, against the fp64 direct convolution with a per-element bound.

The rows come from tests/golden/conv_instances.json, which tools/conv_instance_sweep.py writes on the CPU: it walks a grid of small shapes
through maua_modconv_plan_instance (the plan maua_modconv3x3_f32 dispatches through, without the launch) and keeps the cheapest shape per
name.  Every case asserts that the launch of its shape reports the recorded name (maua_modconv_last_instance), so the coverage claim
cannot rot silently; without a GPU, tests/test_conv_instances_host.py asserts the same names on the plan, that an enumeration of the plan
reaches no name outside the table, and tests/test_isa_checks.py that the library compiles exactly the table's instances.

Every case: the weight is packed by the library's own pack entry straight into a guarded window of exactly the documented size
(9 cin pad32(cout) floats for modes 0 and 1, 12 cin P for mode 2, 18 cin P for mode 3, 12 cin pad32(cout) for mode 4; P = cout padded to
32 up to 32 channels and to 64 above); x, s (s_stride > cin), d, y, ws (exactly maua_modconv_ws_floats), noise, noise_w and bias sit between
red zones (tests/redzone.py); rc == 0, red zones intact, every element of y written and finite.

Tolerance, per element.  u = 2^-24, M = the same convolution over absolute values in fp64, wscale |d| sum |x s| |w|.
  modes 0, 1: |got - want| <= (9 cin + 8) u M — the standard bound of an fp32 dot product of 9 cin terms plus the x s, wscale and d
      multiplies (any summation order, so split-K does not change it);
  modes 2, 3, 4: 4 R u M, R = "rounding_ratio" of the table: the largest |emulation - fp64| / (u M) of a float32 numpy emulation of the
      transforms exactly as written (tests/conv_ref.py emulate_f32), measured on the CPU against the fp64 reference over this file's
      shapes AND operands (conv_ref.case_operands: a transform's amplification at an element depends on the data) by
      tools/conv_instance_sweep.py --ratios — not taken from the kernel; the factor 4 covers the summation order of the matrix
      cores.  A wrong coefficient or a dropped term is orders of magnitude above it;
  through the fused tail: sqrt(2) (bound + 4 u (|conv| + |noise_w noise| + |bias|)) (the leaky ReLU is 1-Lipschitz)."""
import json
import os
import re

import numpy as np
import pytest
import torch

from conv_ref import U32, _layer, case_operands, conv_and_magnitude, upfirdn64
from maua_stylegan2_amd import _lib, seeding
from redzone import Guard

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

TABLE = json.load(open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_instances.json")))
ROWS = TABLE["instances"]
SQRT2 = 2.0 ** 0.5


def pad32(c):
    return (c + 31) // 32 * 32


def wino_pad(c):
    return (c + 63) // 64 * 64 if c > 32 else pad32(c)


PACKS = {0: ("maua_pack_weight_f32", 9, pad32), 1: ("maua_pack_weight_f32", 9, pad32), 2: ("maua_pack_weight_wino_f32", 12, wino_pad),
         3: ("maua_pack_weight_wino43_f32", 18, wino_pad), 4: ("maua_pack_weight_upwino_f32", 12, pad32)}


def pack_guarded(lib, g, weight, mode, dev, name="wp"):
    """weight [1, cout, cin, 3, 3] -> the packed operand of ``mode`` in a window of exactly the documented size, written by the library."""
    _, cout, cin = weight.shape[:3]
    fn, rows, padf = PACKS[mode]
    w_in = g.inp(weight.reshape(cout, cin, 3, 3), "w")
    wp = g.out((rows * cin * padf(cout),), name)
    if mode < 2:
        rc = lib.maua_pack_weight_f32(w_in.data_ptr(), wp.data_ptr(), None, cout, cin, 9, _lib.stream_ptr(dev))
    else:
        rc = getattr(lib, fn)(w_in.data_ptr(), wp.data_ptr(), cout, cin, _lib.stream_ptr(dev))
    assert rc == 0, rc
    return wp


def parse(name):
    m = re.fullmatch(r"modconv_mfma_kernel<(\d+), (\d+), (\d+), (\d+), (true|false), (true|false), (\d+)>", name)
    assert m, name
    return dict(bm=int(m[1]), bn=int(m[2]), wm=int(m[3]), mode=int(m[4]), multi=m[5] == "true", fast=m[6] == "true", maxp=int(m[7]))


def conv_bound(mode, cin, mag):
    k = 9 * cin + 8 if mode < 2 else 4.0 * TABLE["rounding_ratio"][str(mode)]
    return k * U32 * mag


def check_close(got, want, bound, what):
    err = (got.double().cpu() - want).abs()
    worst = float((err / bound.clamp_min(1e-300)).max())
    print(f"{what}: max |err| {float(err.max()):.3e}, max |err| / bound {worst:.3f}")
    assert bool((err <= bound).all()), f"{what}: |err| / bound up to {worst:.3f} at {int((err > bound).sum())} elements"


def run_case(dev, mode, cin, cout, h, w, batch, fuse_act=False, noise=None, d_null=False, seed=0):
    """One guarded maua_modconv3x3_f32 call compared with fp64.  noise: None, "image" (one map per image) or "shared" (stride 0).
    -> the instance name."""
    lib = _lib.load()
    up = mode in (1, 4)
    rng, x_, s_, d_, wt = case_operands(mode, cin, cout, h, w, batch, seed)
    f = lambda *shape: torch.from_numpy(rng.standard_normal(shape).astype(np.float32))  # noqa: E731
    stride = s_.shape[1]  # s_stride > cin: the styles of a layer are a slice of a wider table
    oh, ow = (2 * h + 1, 2 * w + 1) if up else (h, w)
    bias_, nw_ = 0.3 * f(cout), 0.37
    nz_ = f(batch if noise == "image" else 1, 1, oh, ow)
    g = Guard(dev)
    x, s, y = g.inp(x_, "x"), g.inp(s_, "s"), g.out((batch, cout, oh, ow), "y")
    d = None if d_null else g.inp(d_, "d")
    wp = pack_guarded(lib, g, wt, mode, dev)
    n_ws = lib.maua_modconv_ws_floats(batch, cin, cout, h, w, mode)
    ws = g.out((n_ws,), "ws") if n_ws else None
    nz = g.inp(nz_, "noise") if noise else None
    nw, bias = (g.inp(torch.tensor([nw_]), "noise_w"), g.inp(bias_, "bias")) if fuse_act else (None, None)
    rc = lib.maua_modconv3x3_f32(x.data_ptr(), wp.data_ptr(), s.data_ptr(), stride, _lib.ptr(d), y.data_ptr(), batch, cin, cout, h, w, mode,
                                 float(1.0 / np.sqrt(cin * 9)), int(fuse_act), _lib.ptr(nz), oh * ow if noise == "image" else 0, _lib.ptr(nw),
                                 _lib.ptr(bias), _lib.ptr(ws), None, 0, _lib.stream_ptr(dev))
    assert rc == 0, rc
    name = _lib.last_modconv_instance()
    g.check(written=("y", "wp"))
    want, mag = conv_and_magnitude(x_, s_[:, :cin], torch.ones_like(d_) if d_null else d_, wt, up)
    bound = conv_bound(mode, cin, mag)
    if fuse_act:
        nzt = (float(np.float32(nw_)) * nz_.double()) if noise else torch.zeros(1, 1, oh, ow, dtype=torch.float64)
        bt = bias_.double()[None, :, None, None]
        bound = SQRT2 * (bound + 4 * U32 * (want.abs() + nzt.abs() + bt.abs()))
        t = want + nzt + bt
        want = torch.where(t > 0, t, 0.2 * t) * SQRT2
    check_close(y, want, bound, f"{name} mode {mode} {cin}->{cout} {h}x{w} batch {batch}")
    return name


def _id(r):
    p = parse(r["name"])
    return f"m{r['mode']}-{p['bm']}x{p['bn']}x{p['wm']}-{'multi' if p['multi'] else 'single'}-{'fast' if p['fast'] else 'generic'}-p{p['maxp']}"


@pytest.mark.parametrize("row", ROWS, ids=_id)
def test_every_reachable_instance_against_fp64(gpu, row):
    """One case per row of the table: the recorded shape must still reach the recorded instance, inside its buffers, within the bound."""
    name = run_case(gpu, row["mode"], row["cin"], row["cout"], row["h"], row["w"], row["batch"])
    assert name == row["name"], f"the plan drifted: {row} now runs {name} (re-run tools/conv_instance_sweep.py)"
    assert parse(name)["mode"] == row["mode"]


def test_the_table_is_a_table_of_distinct_instances():
    names = [r["name"] for r in ROWS]
    assert len(set(names)) == len(names) and len(names) >= 58
    assert set(TABLE["rounding_ratio"]) == {"2", "3", "4"}


# ---- edge variants: at least once per applicable mode, on shapes chosen for the property (asserted from outside: the instance name, the
# workspace size).  Reasoning for the shapes is next to each list; the plan itself is not re-implemented here.
# fuse_act on the three plain modes, per-image and shared noise; the first of each pair is a tile that holds several images (1-row maps:
# the image index inside the tile drives the noise lookup), the second a single-image tile with ragged rows / columns
FUSED = [(0, 3, 40, 1, 3, 3, "image", True), (0, 12, 40, 9, 9, 2, "shared", False), (0, 12, 24, 9, 9, 2, "image", False),
         (2, 3, 40, 1, 4, 3, "image", True), (2, 12, 40, 5, 20, 2, "shared", False), (2, 12, 136, 9, 6, 2, "image", False),
         (3, 3, 40, 1, 8, 3, "image", True), (3, 10, 24, 5, 36, 2, "shared", False), (3, 10, 40, 5, 36, 2, "image", False)]
# images per tile (scratch evaluation of the tile shapes: an 8 x 8 map fills a quarter of a 256-pixel tile, ...): the batch is larger than
# the images of a tile and no multiple of it, so the last image group is ragged
RAGGED = [(0, 12, 40, 8, 8, 5), (0, 12, 136, 8, 8, 3), (1, 12, 40, 3, 3, 5), (1, 12, 24, 3, 3, 5), (2, 12, 40, 4, 8, 5), (2, 12, 136, 4, 16, 3),
          (3, 10, 24, 4, 16, 5), (3, 12, 40, 4, 16, 5)]
# split-K: 68 channels on an 8-channel chunk are 9 chunks, the last half full -> 4 splits of 3 chunks cover it in 3; 66 channels on a
# 4-channel chunk (mode 3; the 128-row tile of mode 2) are 17 chunks -> 6 splits of 3, the last one of 2 chunks, the last chunk half full
SPLITK = [(0, 68, 40, 8, 8, 1, 8), (1, 68, 40, 4, 4, 1, 8), (2, 68, 40, 8, 16, 1, 8), (2, 66, 136, 8, 16, 1, 4), (3, 66, 40, 8, 16, 1, 4),
          (4, 68, 40, 8, 16, 1, 8), (4, 68, 24, 16, 16, 1, 8)]  # (..., chunk channels)
# flat runs (transposed modes): the position grid (H + 1) x (W + 1) [mode 4: x (W / 2 + 1) pairs] has an odd width and is no multiple
# of the run length (128 positions up to 32 channels, 64 above)
FLAT = [(1, 12, 40, 8, 16, 2), (1, 12, 24, 8, 16, 2), (4, 12, 40, 8, 16, 2), (4, 12, 24, 16, 16, 1)]
D_NULL = [(0, 3, 40, 9, 9, 2), (1, 3, 40, 1, 8, 2), (2, 3, 40, 5, 20, 2), (3, 3, 40, 5, 36, 2), (4, 3, 40, 1, 66, 2)]
TORGB = [(m, 10, co, 16, 36, 2, skip, u8) for m in (0, 2, 3) for co, skip, u8 in ((24, True, False), (40, False, False), (40, True, m == 3))]


def extra_shapes():
    """(mode, cin, cout, h, w, batch) of every edge variant: tools/conv_instance_sweep.py --ratios measures the rounding ratios over them too."""
    out = [t[:6] for t in FUSED + RAGGED + SPLITK + FLAT + D_NULL + TORGB]
    return out + [(0, 12, 32, 4, 4, 3), (1, 12, 40, 4, 4, 3)]


@pytest.mark.parametrize("mode,cin,cout,h,w,batch,noise,multi", FUSED)
def test_fused_tail_on_the_generic_instances(gpu, mode, cin, cout, h, w, batch, noise, multi):
    p = parse(run_case(gpu, mode, cin, cout, h, w, batch, fuse_act=True, noise=noise))
    assert p["multi"] == multi and not p["fast"]


@pytest.mark.parametrize("mode,cin,cout,h,w,batch", RAGGED)
def test_ragged_last_image_group(gpu, mode, cin, cout, h, w, batch):
    p = parse(run_case(gpu, mode, cin, cout, h, w, batch, fuse_act=mode != 1, noise="image" if mode != 1 else None))
    assert p["multi"]


@pytest.mark.parametrize("mode,cin,cout,h,w,batch,cc", SPLITK)
def test_split_k_off_the_power_of_two_with_a_partial_last_chunk(gpu, mode, cin, cout, h, w, batch, cc):
    lib = _lib.load()
    oh, ow = (2 * h + 1, 2 * w + 1) if mode in (1, 4) else (h, w)
    n_ws = lib.maua_modconv_ws_floats(batch, cin, cout, h, w, mode)
    splits, rem = divmod(n_ws, batch * cout * oh * ow)
    assert rem == 0 and splits > 1 and splits & (splits - 1), splits  # more than one slab, not a power of two
    assert cin % cc, "the last chunk is partial"
    assert not parse(run_case(gpu, mode, cin, cout, h, w, batch))["fast"]


@pytest.mark.parametrize("mode,cin,cout,h,w,batch", FLAT)
def test_flat_runs_with_a_partial_last_run(gpu, mode, cin, cout, h, w, batch):
    p = parse(run_case(gpu, mode, cin, cout, h, w, batch))
    gw = w + 1 if mode == 1 else w // 2 + 1
    assert gw % 2 == 1 and ((h + 1) * gw) % p["bn"] and (h + 1) * gw > p["bn"] and not p["multi"]


@pytest.mark.parametrize("mode,cin,cout,h,w,batch", D_NULL)
def test_without_demodulation(gpu, mode, cin, cout, h, w, batch):
    run_case(gpu, mode, cin, cout, h, w, batch, d_null=True)


REFUSED = [(3, 8, 32, 16, 4, 1), (3, 8, 40, 4, 20, 1), (3, 8, 40, 2, 32, 2), (4, 8, 32, 4, 8, 1), (4, 8, 40, 4, 8, 1), (2, 8, 32, 4, 7, 1), (3, 8, 32, 4, 6, 1)]


@pytest.mark.parametrize("mode,cin,cout,h,w,batch", REFUSED)
def test_refused_shapes_return_einval_and_launch_nothing(gpu, mode, cin, cout, h, w, batch):
    """include/maua_hip.h: up == 3 with W == 4 or with H <= 4 and W >= 20, up == 4 on a grid of a single run, and the width rules."""
    lib = _lib.load()
    g = Guard(gpu)
    up = mode == 4
    x, s = g.inp(torch.ones(batch, cin, h, w), "x"), g.inp(torch.ones(batch, cin), "s")
    wp = g.inp(torch.ones(PACKS[mode][1] * cin * PACKS[mode][2](cout)), "wp")
    y = g.out((batch, cout, 2 * h + 1, 2 * w + 1) if up else (batch, cout, h, w), "y")
    ws = g.out((max(1, lib.maua_modconv_ws_floats(batch, cin, cout, h, w, mode)),), "ws")
    rc = lib.maua_modconv3x3_f32(x.data_ptr(), wp.data_ptr(), s.data_ptr(), cin, None, y.data_ptr(), batch, cin, cout, h, w, mode, 0.1, 0, None, 0,
                                 None, None, ws.data_ptr(), None, 0, _lib.stream_ptr(gpu))
    assert rc == -22, rc
    assert g.untouched("y") and g.untouched("ws")
    g.check()


@pytest.mark.parametrize("mode,cin,cout,h,w,batch,with_skip,u8", TORGB)
def test_torgb_epilogue_with_ragged_channels(gpu, mode, cin, cout, h, w, batch, with_skip, u8):
    """maua_styledconv_torgb_f32 on this kernel with 24 / 40 output channels (every other RGB shape of the suite has 32 or 64) and a
    channel count that is no multiple of the K chunk: the padded rows of the weight tile must contribute nothing, and rgb_w [3, cout]
    sits between red zones, so a read past it is a NaN in the image.  Feature map: the bound of the fused tail.  Image: the ToRGB of
    the fp64 feature map in fp64; bound = sum_o |w_o| bound_o (the feature map's error through the 1x1 conv) + (cout + 12) u sum of the
    absolute terms (a cout-term fp32 dot product, its modulated weights (wscale w) s, the bias and the four skip taps)."""
    from maua_stylegan2_amd.models.stylegan2 import Upsample

    lib = _lib.load()
    rng, x_, s_cin, d_, wt = case_operands(mode, cin, cout, h, w, batch)
    f = lambda *shape: torch.from_numpy(rng.standard_normal(shape).astype(np.float32))  # noqa: E731
    stride = max(cin, cout) + 3  # (rgb_s shares the stride of s and is indexed by the output channel)
    s_ = torch.cat([s_cin[:, :cin], 1 + 0.3 * f(batch, stride - cin)], 1)
    nz_, bias_, nw_ = f(batch, 1, h, w), 0.3 * f(cout), 0.2
    rgb_w_, rgb_s_, rgb_b_, skip_ = f(3, cout), 1 + 0.3 * f(batch, stride), 0.3 * f(3), f(batch, 3, h // 2, w // 2)
    g = Guard(gpu)
    x, s, d = g.inp(x_, "x"), g.inp(s_, "s"), g.inp(d_, "d")
    nz, nw, bias = g.inp(nz_, "noise"), g.inp(torch.tensor([nw_]), "noise_w"), g.inp(bias_, "bias")
    rgb_w, rgb_s, rgb_b = g.inp(rgb_w_, "rgb_w"), g.inp(rgb_s_, "rgb_s"), g.inp(rgb_b_, "rgb_bias")
    skip = g.inp(skip_, "skip") if with_skip else None
    k4 = g.inp(torch.from_numpy(seeding.fir_kernel_2d((1, 3, 3, 1), 4.0)), "k4")
    wp = pack_guarded(lib, g, wt, mode, gpu)
    y, img = g.out((batch, cout, h, w), "y"), g.out((batch, 3, h, w), "rgb")
    frames = g.out((batch, h, w, 3), "frames", dtype=torch.uint8) if u8 else None
    assert lib.maua_modconv_ws_floats(batch, cin, cout, h, w, mode) == 0
    rc = lib.maua_styledconv_torgb_f32(x.data_ptr(), wp.data_ptr(), s.data_ptr(), stride, d.data_ptr(), y.data_ptr(), batch, cin, cout, h, w, mode,
                                       float(1.0 / np.sqrt(cin * 9)), nz.data_ptr(), h * w, nw.data_ptr(), bias.data_ptr(), rgb_w.data_ptr(),
                                       rgb_s.data_ptr(), 0.1, rgb_b.data_ptr(), _lib.ptr(skip), k4.data_ptr() if with_skip else None,
                                       img.data_ptr(), 1, _lib.ptr(frames), None, 0, None, _lib.stream_ptr(gpu))
    assert rc == 0, rc
    p = parse(_lib.last_modconv_instance())
    assert p["mode"] == mode and not p["fast"] and not p["multi"]
    g.check(written=("y", "rgb", "wp") + (("frames",) if u8 else ()), nonfinite_ok=("frames",))  # (bytes, not floats)
    conv, mag = conv_and_magnitude(x_, s_[:, :cin], d_, wt, False)
    nzt, bt = float(np.float32(nw_)) * nz_.double(), bias_.double()[None, :, None, None]
    fbound = SQRT2 * (conv_bound(mode, cin, mag) + 4 * U32 * (conv.abs() + nzt.abs() + bt.abs()))
    t = conv + nzt + bt
    feat = torch.where(t > 0, t, 0.2 * t) * SQRT2
    check_close(y, feat, fbound, f"feature map mode {mode} cout {cout}")
    mw = float(np.float32(0.1)) * rgb_w_.double()[None] * rgb_s_.double()[:, None, :cout]  # [B, 3, cout]
    want = torch.einsum("bco,bohw->bchw", mw, feat) + rgb_b_.double()[None, :, None, None]
    absum = torch.einsum("bco,bohw->bchw", mw.abs(), feat.abs()) + rgb_b_.double().abs()[None, :, None, None]
    if with_skip:
        up = Upsample([1, 3, 3, 1])
        want = want + upfirdn64(skip_, up.kernel, up=2, pad=up.pad)
        absum = absum + upfirdn64(skip_.abs(), up.kernel.abs(), up=2, pad=up.pad)
    ibound = torch.einsum("bco,bohw->bchw", mw.abs(), fbound) + (cout + 12) * U32 * absum
    check_close(img, want, ibound, f"image mode {mode} cout {cout}")
    if u8:
        q = ((img.clamp(-1, 1) + 1) * 127.5).to(torch.uint8).permute(0, 2, 3, 1)
        assert int((frames.int() - q.int()).abs().max()) <= 1  # (the kernel converts the same registers; a float tie may fall either way)


def test_lowres_plain_entry_on_generic_loads(gpu):
    """maua_styledconv_rgbpart_lowres_f32 with a channel count that is no multiple of the K chunk: K is not split, so the single slab
    left in `ws` (force_ws) is written by the generic-load instance; slab sum + tail against fp64 with the fused-tail bound."""
    lib = _lib.load()
    mode, cin, cout, h, w, batch = 0, 12, 32, 4, 4, 3
    assert lib.maua_lowres_ok(cin, cout, h, w, mode) == 1
    rng = np.random.default_rng(5)
    f = lambda *shape: torch.from_numpy(rng.standard_normal(shape).astype(np.float32))  # noqa: E731
    stride = 40
    x_, s_, wt = f(batch, cin, h, w), 1 + 0.3 * f(batch, stride), f(1, cout, cin, 3, 3)
    d_, bias_, nz_ = 0.5 + torch.rand(batch, cout), 0.3 * f(cout), f(batch, 1, h, w)
    rgb_w_, rgb_s_ = f(3, cout), 1 + 0.3 * f(batch, stride)
    g = Guard(gpu)
    x, s, d = g.inp(x_, "x"), g.inp(s_, "s"), g.inp(d_, "d")
    nz, nw, bias = g.inp(nz_, "noise"), g.inp(torch.tensor([0.2]), "noise_w"), g.inp(bias_, "bias")
    rgb_w, rgb_s = g.inp(rgb_w_, "rgb_w"), g.inp(rgb_s_, "rgb_s")
    wp = pack_guarded(lib, g, wt, mode, gpu)
    y, part = g.out((batch, cout, h, w), "y"), g.out((batch, 3 * (cout // 32), h, w), "rgb_partial")
    n_ws = lib.maua_lowres_ws_floats(batch, cin, cout, h, w, mode)
    assert n_ws == batch * cout * h * w  # one slab
    ws = g.out((n_ws,), "ws")
    rc = lib.maua_styledconv_rgbpart_lowres_f32(x.data_ptr(), wp.data_ptr(), s.data_ptr(), stride, d.data_ptr(), y.data_ptr(), ws.data_ptr(),
                                                nz.data_ptr(), h * w, nw.data_ptr(), bias.data_ptr(), rgb_w.data_ptr(), rgb_s.data_ptr(), 0.1,
                                                part.data_ptr(), None, 0, batch, cin, cout, h, w, mode, float(1.0 / np.sqrt(cin * 9)),
                                                _lib.stream_ptr(gpu))
    assert rc == 0, rc
    assert not parse(_lib.last_modconv_instance())["fast"]
    g.check(written=("y", "rgb_partial", "ws", "wp"))
    conv, mag = conv_and_magnitude(x_, s_[:, :cin], d_, wt, False)
    nzt, bt = float(np.float32(0.2)) * nz_.double(), bias_.double()[None, :, None, None]
    fbound = SQRT2 * (conv_bound(mode, cin, mag) + 4 * U32 * (conv.abs() + nzt.abs() + bt.abs()))
    t = conv + nzt + bt
    feat = torch.where(t > 0, t, 0.2 * t) * SQRT2
    check_close(y, feat, fbound, "lowres plain entry, feature map")
    mw = float(np.float32(0.1)) * rgb_w_.double()[None] * rgb_s_.double()[:, None, :cout]
    want = torch.einsum("bco,bohw->bchw", mw, feat)
    ibound = torch.einsum("bco,bohw->bchw", mw.abs(), fbound) + (cout + 12) * U32 * torch.einsum("bco,bohw->bchw", mw.abs(), feat.abs())
    check_close(part.view(batch, cout // 32, 3, h, w).sum(1), want, ibound, "lowres plain entry, partial ToRGB planes")


def test_lowres_upsampling_entry_on_generic_loads(gpu):
    """maua_upconv_blur_lowres_f32 (up = 1) with a channel count that is no multiple of the K chunk: one slab from the generic-load
    polyphase instance, then slab sum + blur + tail.  Bound: the blur is linear with non-negative taps, so the raw values' bounds
    (9 cin + 8) u M pass through it; plus 20 u of the blurred magnitudes for the 16 fmas, d and the tail's roundings, through sqrt(2) and
    the post scale."""
    lib = _lib.load()
    cin, cout, h, w, batch = 12, 40, 4, 4, 3
    assert lib.maua_lowres_ok(cin, cout, h, w, 1) == 1
    m, rng = _layer(cin, cout, True, 77, gpu)
    f = lambda *shape: torch.from_numpy(rng.standard_normal(shape).astype(np.float32))  # noqa: E731
    stride = 48
    x_, s_, post_ = f(batch, cin, h, w), 1 + 0.3 * f(batch, stride), 1 + 0.3 * f(batch, stride)
    d_, bias_, nz_ = 0.5 + torch.rand(batch, cout), 0.3 * f(cout), f(1, 1, 2 * h, 2 * w)
    wt = m.weight.cpu()
    g = Guard(gpu)
    x, s, d, post, bias = g.inp(x_, "x"), g.inp(s_, "s"), g.inp(d_, "d"), g.inp(post_, "post_s"), g.inp(bias_, "bias")
    k4, nw, nz = g.inp(m.blur.kernel, "k4"), g.inp(torch.tensor([0.37]), "noise_w"), g.inp(nz_, "noise")
    wp = pack_guarded(lib, g, wt, 1, gpu)
    y = g.out((batch, cout, 2 * h, 2 * w), "y")
    n_ws = lib.maua_lowres_ws_floats(batch, cin, cout, h, w, 1)
    assert n_ws == batch * cout * (2 * h + 1) * (2 * w + 1)  # one slab
    ws = g.out((n_ws,), "ws")
    rc = lib.maua_upconv_blur_lowres_f32(x.data_ptr(), wp.data_ptr(), s.data_ptr(), stride, d.data_ptr(), y.data_ptr(), ws.data_ptr(), k4.data_ptr(),
                                         nz.data_ptr(), 0, nw.data_ptr(), bias.data_ptr(), None, 0, batch, cin, cout, h, w, 1, float(m.scale),
                                         post.data_ptr(), _lib.stream_ptr(gpu))
    assert rc == 0, rc
    assert not parse(_lib.last_modconv_instance())["fast"]
    g.check(written=("y", "ws", "wp"))
    raw, mag = conv_and_magnitude(x_, s_[:, :cin], d_, wt, True)
    kern = m.blur.kernel.cpu()
    assert bool((kern >= 0).all())
    blur = lambda a: upfirdn64(a, kern, up=1, pad=(1, 1))  # noqa: E731
    nzt, bt = float(np.float32(0.37)) * nz_.double(), bias_.double()[None, :, None, None]
    t = blur(raw) + nzt + bt
    ps = post_.double()[:, :cout, None, None]
    want = torch.where(t > 0, t, 0.2 * t) * SQRT2 * ps
    bound = SQRT2 * ps.abs() * (blur((9 * cin + 8) * U32 * mag) + 20 * U32 * blur(raw.abs()) + 4 * U32 * (nzt.abs() + bt.abs()))
    check_close(y, want, bound, "lowres up-sampling entry")
