"""GPU: the frame-source read path of the layer entries, through the C ABI.

Eight entries take (src, noise_slot) and read their noise through src->noise[slot] + src->frame0 * src->noise_stride[slot] — the path of
every captured render — and every kernel file carries its own copy of that address computation.  maua_upconv_blur_f32 has its entry-level
test (test_layers_gpu.py, test_upconv_blur_fused_c_abi_contract); here are the other seven, each at a small shape of its own kernel family:
the run through a device maua_frame_source_t (7-frame sequence, frame0 = 3, slots 5 and 31, the entry's own noise arguments pointing at
NaNs) must give the bits of the run with the noise slice as arguments.  No tolerances: every comparison is bit for bit.  Operands, the
frame source, outputs and workspaces sit between red zones (tests/redzone.py)."""
import numpy as np
import pytest
import torch

from maua_stylegan2_amd import _lib, seeding
from redzone import Guard
from test_canary_gpu import _layer, _packed

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

EINVAL = -22
FRAMES, FRAME0 = 7, 3


class _Case:
    """Operands of one entry in a Guard; ``call(tag, noise, nstride, src, slot, nw)`` launches it on fresh outputs named ``<name>:<tag>``."""

    def __init__(self, gpu, batch, cin, cout, h, w, up, pack_mode, seed, oh=None, ow=None):
        self.gpu, self.lib, self.g = gpu, _lib.load(), Guard(gpu)
        self.batch, self.cin, self.cout, self.h, self.w = batch, cin, cout, h, w
        self.oh, self.ow = oh or h, ow or w
        self.m, self.r = _layer(cin, cout, up, seed, gpu)
        self.stride = max(cin, cout)
        g = self.g
        self.x, self.s, self.d = g.inp(self.f(batch, cin, h, w), "x"), g.inp(1 + 0.3 * self.f(batch, self.stride), "s"), g.inp(0.5 + self.u(batch, cout), "d")
        self.bias, self.nw = g.inp(0.3 * self.f(cout), "bias"), g.inp(torch.tensor([0.37]), "noise_w")
        self.wp = _packed(self.m, pack_mode, g) if pack_mode is not None else None
        self.st = _lib.stream_ptr(gpu)
        self.outs = []   # (name, shape) of what a call must write
        self.ws_floats = 0

    def f(self, *shape):
        return torch.from_numpy(self.r.standard_normal(shape).astype(np.float32))

    def u(self, *shape):
        return torch.from_numpy(self.r.random(shape).astype(np.float32))

    def rgb_operands(self, with_bias=True):
        g = self.g
        self.rgb_w, self.rgb_s = g.inp(self.f(3, self.cout), "rgb_w"), g.inp(1 + 0.3 * self.f(self.batch, self.stride), "rgb_s")
        self.rgb_b = g.inp(0.3 * self.f(3), "rgb_bias") if with_bias else None

    def call(self, tag, noise=None, nstride=0, src=None, slot=0, nw=True):
        bufs = {name: self.g.out(shape, f"{name}:{tag}") for name, shape in self.outs}
        ws = self.g.out((self.ws_floats,), f"ws:{tag}") if self.ws_floats else None
        rc = self.launch(bufs, ws, _lib.ptr(noise), nstride, self.nw.data_ptr() if nw else None, src, slot)
        return rc, bufs

    def names(self, tag):
        return tuple(f"{name}:{tag}" for name, _ in self.outs)


def _blur_tail(gpu):
    c = _Case(gpu, 3, 5, 5, 9, 11, False, None, 1, oh=8, ow=10)
    k = c.g.inp(torch.from_numpy(seeding.fir_kernel_2d((1, 3, 3, 1), 4.0)), "k")
    c.outs = [("y", (3, 5, 8, 10))]
    c.launch = lambda o, ws, nz, nst, nw, src, slot: c.lib.maua_blur_noise_act_f32(
        c.x.data_ptr(), k.data_ptr(), o["y"].data_ptr(), 3, 5, 9, 11, 4, 4, 1, 1, c.d.data_ptr(), nz, nst, nw, c.bias.data_ptr(), src, slot, None, 0, c.st)
    return c


def _modconv(mode, cin, cout, h, w, batch, split_k):
    def build(gpu):
        c = _Case(gpu, batch, cin, cout, h, w, False, mode, 10 + mode + cin)
        c.outs = [("y", (batch, cout, h, w))]
        c.ws_floats = c.lib.maua_modconv_ws_floats(batch, cin, cout, h, w, mode)
        assert (c.ws_floats > 0) == split_k  # (split K: the tail, noise included, runs in reduce_tail_kernel instead of the conv's epilogue)
        c.launch = lambda o, ws, nz, nst, nw, src, slot: c.lib.maua_modconv3x3_f32(
            c.x.data_ptr(), c.wp.data_ptr(), c.s.data_ptr(), c.stride, c.d.data_ptr(), o["y"].data_ptr(), batch, cin, cout, h, w, mode, float(c.m.scale), 1,
            nz, nst, nw, c.bias.data_ptr(), _lib.ptr(ws), src, slot, c.st)
        return c
    return build


def _torgb(mode, cin, cout, h, w, batch):
    def build(gpu):
        c = _Case(gpu, batch, cin, cout, h, w, False, mode, 20 + mode)
        c.rgb_operands()
        c.outs = [("y", (batch, cout, h, w)), ("rgb", (batch, 3, h, w))]
        c.launch = lambda o, ws, nz, nst, nw, src, slot: c.lib.maua_styledconv_torgb_f32(
            c.x.data_ptr(), c.wp.data_ptr(), c.s.data_ptr(), c.stride, c.d.data_ptr(), o["y"].data_ptr(), batch, cin, cout, h, w, mode, float(c.m.scale),
            nz, nst, nw, c.bias.data_ptr(), c.rgb_w.data_ptr(), c.rgb_s.data_ptr(), 0.1, c.rgb_b.data_ptr(), None, None, o["rgb"].data_ptr(), 1, None,
            src, slot, None, c.st)
        return c
    return build


def _torgb_partial(gpu):
    batch, cin, cout, h, w = 2, 128, 256, 16, 32
    c = _Case(gpu, batch, cin, cout, h, w, False, 5, 30)
    c.rgb_operands(with_bias=False)
    mt = c.lib.maua_modconv_w2d_mtiles(cin, cout, h, w)
    c.outs = [("y", (batch, cout, h, w)), ("rgb_partial", (batch, 3 * mt, h, w))]
    c.launch = lambda o, ws, nz, nst, nw, src, slot: c.lib.maua_styledconv_torgb_partial_f32(
        c.x.data_ptr(), c.wp.data_ptr(), c.s.data_ptr(), c.stride, c.d.data_ptr(), o["y"].data_ptr(), batch, cin, cout, h, w, 5, float(c.m.scale), nz, nst,
        nw, c.bias.data_ptr(), c.rgb_w.data_ptr(), c.rgb_s.data_ptr(), 0.1, o["rgb_partial"].data_ptr(), src, slot, None, c.st)
    return c


def _lowres_up(up, cin, cout, h, w, batch):
    def build(gpu):
        c = _Case(gpu, batch, cin, cout, h, w, True, 6 if up == 6 else 0, 40 + up, oh=2 * h, ow=2 * w)
        assert c.lib.maua_lowres_ok(cin, cout, h, w, up) == 1
        k4 = c.g.inp(c.m.blur.kernel, "k4")
        c.outs = [("y", (batch, cout, 2 * h, 2 * w))]
        c.ws_floats = c.lib.maua_lowres_ws_floats(batch, cin, cout, h, w, up)
        c.launch = lambda o, ws, nz, nst, nw, src, slot: c.lib.maua_upconv_blur_lowres_f32(
            c.x.data_ptr(), c.wp.data_ptr(), c.s.data_ptr(), c.stride, c.d.data_ptr(), o["y"].data_ptr(), ws.data_ptr(), k4.data_ptr(), nz, nst, nw,
            c.bias.data_ptr(), src, slot, batch, cin, cout, h, w, up, float(c.m.scale), None, c.st)
        return c
    return build


def _lowres_plain(gpu):
    batch, cin, cout, h, w = 3, 64, 32, 8, 8
    c = _Case(gpu, batch, cin, cout, h, w, False, 0, 50)
    assert c.lib.maua_lowres_ok(cin, cout, h, w, 0) == 1
    c.rgb_operands(with_bias=False)
    c.outs = [("y", (batch, cout, h, w)), ("rgb_partial", (batch, 3 * (cout // 32), h, w))]
    c.ws_floats = c.lib.maua_lowres_ws_floats(batch, cin, cout, h, w, 0)
    c.launch = lambda o, ws, nz, nst, nw, src, slot: c.lib.maua_styledconv_rgbpart_lowres_f32(
        c.x.data_ptr(), c.wp.data_ptr(), c.s.data_ptr(), c.stride, c.d.data_ptr(), o["y"].data_ptr(), ws.data_ptr(), nz, nst, nw, c.bias.data_ptr(),
        c.rgb_w.data_ptr(), c.rgb_s.data_ptr(), 0.1, o["rgb_partial"].data_ptr(), src, slot, batch, cin, cout, h, w, 0, float(c.m.scale), c.st)
    return c


def _const_conv(gpu):
    batch, cin, cout = 3, 8, 32
    c = _Case(gpu, batch, cin, cout, 4, 4, False, None, 60)
    assert c.lib.maua_const_conv_ok(cin, cout, 4, 4) == 1
    c.rgb_operands(with_bias=False)
    w_in, const = c.g.inp(c.m.weight.reshape(cout, cin, 3, 3), "w"), c.g.inp(c.f(cin, 4, 4), "const")
    T = c.g.out((cout * 16 * cin,), "T")
    assert c.lib.maua_pack_const_conv_f32(w_in.data_ptr(), const.data_ptr(), T.data_ptr(), cout, cin, 4, 4, c.st) == 0
    c.outs = [("y", (batch, cout, 4, 4)), ("rgb_partial", (batch, 3 * (cout // 32), 4, 4))]
    c.launch = lambda o, ws, nz, nst, nw, src, slot: c.lib.maua_const_styledconv_f32(
        T.data_ptr(), c.s.data_ptr(), c.stride, c.d.data_ptr(), o["y"].data_ptr(), nz, nst, nw, c.bias.data_ptr(), c.rgb_w.data_ptr(), c.rgb_s.data_ptr(),
        0.1, o["rgb_partial"].data_ptr(), src, slot, batch, cin, cout, 4, 4, float(c.m.scale), c.st)
    return c


CASES = {  # small shapes of each kernel family (those of tests/test_canary_gpu.py where they are the smallest), at most 4 frames per launch;
    # modes 0, 2 and 3 once with the tail in the convolution's own epilogue and once behind a split K (reduce_tail_kernel)
    "blur_noise_act": _blur_tail,
    "modconv3x3-mode0": _modconv(0, 24, 40, 5, 7, 3, False),
    "modconv3x3-mode0-splitk": _modconv(0, 512, 512, 4, 4, 2, True),
    "modconv3x3-mode2": _modconv(2, 8, 32, 32, 36, 2, False),
    "modconv3x3-mode2-splitk": _modconv(2, 64, 64, 16, 34, 2, True),
    "modconv3x3-mode3": _modconv(3, 8, 32, 32, 36, 2, False),
    "modconv3x3-mode3-splitk": _modconv(3, 64, 96, 8, 36, 2, True),
    "modconv3x3-mode5": _modconv(5, 4, 32, 16, 32, 2, False),
    "styledconv_torgb-mode0": _torgb(0, 32, 32, 256, 256, 4),
    "styledconv_torgb-mode5": _torgb(5, 32, 32, 16, 32, 2),
    "styledconv_torgb_partial": _torgb_partial,
    "upconv_blur_lowres-up1": _lowres_up(1, 24, 40, 5, 7, 3),
    "upconv_blur_lowres-up6": _lowres_up(6, 8, 32, 16, 16, 2),
    "styledconv_rgbpart_lowres": _lowres_plain,
    "const_styledconv": _const_conv,
}


def _frame_source(g, name, slots):
    """A device maua_frame_source_t at frame FRAME0 with ``slots`` = {slot: (map sequence or None, floats between frames)}."""
    src = _lib.FrameSource()
    src.frame0 = FRAME0
    for slot, (t, stride) in slots.items():
        src.noise[slot], src.noise_stride[slot] = _lib.ptr(t), stride
    return g.inp(torch.frombuffer(bytearray(bytes(src)), dtype=torch.uint8), name, dtype=torch.uint8)


def _same_bits(c, a, b):
    for name, _ in c.outs:
        assert torch.equal(a[name].view(torch.int32), b[name].view(torch.int32)), name


@pytest.mark.parametrize("entry", list(CASES))
def test_noise_through_a_frame_source_equals_noise_through_the_arguments(gpu, entry):
    c = CASES[entry](gpu)
    g, batch, hw = c.g, c.batch, c.oh * c.ow
    assert FRAME0 + batch <= FRAMES
    seq_ = c.f(FRAMES, 1, c.oh, c.ow)
    seq = g.inp(seq_, "noise_sequence")
    nan = g.inp(torch.full((batch, hw), float("nan")), "ignored_noise")

    # the slice [frame0, frame0 + batch) as arguments / the whole sequence behind src, the arguments pointing at NaNs
    rc, direct = c.call("direct", g.inp(seq_[FRAME0: FRAME0 + batch], "noise_slice"), hw)
    assert rc == 0, rc
    g.check(written=c.names("direct"))
    for slot in (5, 31):
        src = _frame_source(g, f"src{slot}", {slot: (seq, hw)})
        rc, via = c.call(f"slot{slot}", nan, hw, src.data_ptr(), slot)
        assert rc == 0, rc
        g.check(written=c.names(f"slot{slot}"))  # (finite as well: the NaNs were not read)
        _same_bits(c, direct, via)

    # stride 0: one map shared by every frame, whatever frame0 is
    one = g.inp(seq_[1], "shared_map")
    rc, shared = c.call("shared", one, 0)
    assert rc == 0, rc
    rc, via = c.call("src_shared", nan, hw, _frame_source(g, "src_shared", {5: (one, 0)}).data_ptr(), 5)
    assert rc == 0, rc
    g.check(written=c.names("shared") + c.names("src_shared"))
    _same_bits(c, shared, via)
    assert not torch.equal(shared["y"], direct["y"])  # (the noise does reach the output)

    # an empty slot: no noise
    rc, none = c.call("none")
    assert rc == 0, rc
    rc, via = c.call("src_none", nan, hw, _frame_source(g, "src_none", {6: (seq, hw)}).data_ptr(), 5)
    assert rc == 0, rc
    g.check(written=c.names("none") + c.names("src_none"))
    _same_bits(c, none, via)

    # refusals: a slot outside 0 .. 31, a frame source without noise_w
    src = _frame_source(g, "src_refused", {5: (seq, hw)})
    for tag, slot, nw in (("below", -1, True), ("above", 32, True), ("no_noise_w", 5, False)):
        rc, _ = c.call(tag, None, 0, src.data_ptr(), slot, nw=nw)
        assert rc == EINVAL, (tag, rc)
        assert all(g.untouched(n) for n in c.names(tag)), tag
    g.check()
