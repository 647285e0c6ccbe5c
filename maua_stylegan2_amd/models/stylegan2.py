"""StyleGAN2 generator (inference) for MI355X — host-side mirror of /root/reference/models/stylegan2.py:1-576.

Same class names, constructor arguments, ``forward`` signatures and state-dict keys as the reference (so
``th.load(ckpt)["g_ema"]`` drops in, models/stylegan2.py:458-459), but the forward is a different program:

  reference (per StyledConv)                          here
  ------------------------------------------------    ---------------------------------------------------------
  F.linear, mul, pow/sum/rsqrt, mul  (per layer)      2 launches for ALL layers: maua_style_affine_f32, maua_demod_f32
  grouped conv with per-sample weights (cuDNN)        shared-weight implicit GEMM on fp32 MFMA, input-scale/output-demod
  add noise, fused_bias_act                           fused into the conv epilogue (plain) / the blur kernel (upsample)
  conv_transpose2d + upfirdn2d (Blur)                 polyphase MFMA transposed conv + fir_tile_kernel with fused tail
  ToRGB: linear, mul, conv, add, upfirdn2d, add       1 launch (maua_torgb_f32)

All activations live in a per-batch-size cache of static device buffers, so a forward performs no allocation after
its first call and can be captured into a hipGraph (``capture_graph``).  There is no CPU path: CPU tensors raise.
"""
import ctypes
import math
from types import SimpleNamespace

import torch as th
from torch import nn
from torch.nn import functional as F

from .. import _lib
from ..op import FusedLeakyReLU, fused_leaky_relu, upfirdn2d


class PixelNorm(nn.Module):
    def forward(self, inputs):
        return inputs * th.rsqrt(th.mean(inputs ** 2, dim=1, keepdim=True) + 1e-8)


def make_kernel(k):
    k = th.tensor(k, dtype=th.float32)
    if k.ndim == 1:
        k = k[None, :] * k[:, None]
    k /= k.sum()
    return k


class Upsample(nn.Module):
    """reference :34-52 — upfirdn2d(up=factor, pad=(pad0, pad1)) with kernel * factor**2."""

    def __init__(self, kernel, factor=2):
        super().__init__()
        self.factor = factor
        self.register_buffer("kernel", make_kernel(kernel) * (factor ** 2))
        p = self.kernel.shape[0] - factor
        self.pad = ((p + 1) // 2 + factor - 1, p // 2)

    def forward(self, inputs):
        return upfirdn2d(inputs, self.kernel, up=self.factor, down=1, pad=self.pad)


class Blur(nn.Module):
    """reference :76-92."""

    def __init__(self, kernel, pad, upsample_factor=1):
        super().__init__()
        kernel = make_kernel(kernel)
        if upsample_factor > 1:
            kernel = kernel * (upsample_factor ** 2)
        self.register_buffer("kernel", kernel)
        self.pad = pad

    def forward(self, inputs):
        return upfirdn2d(inputs, self.kernel, pad=self.pad)


import threading  # noqa: E402

_SKIP_INIT = threading.local()  # .on: set only on the thread that is building a Generator from a checkpoint


def _randn(*shape):
    """``th.randn`` for a parameter / buffer of a module under construction.  While a ``Generator`` that was given a checkpoint builds
    itself, every such tensor is about to be overwritten by the strict ``load_state_dict`` of its constructor: it is then left
    uninitialised (the 30 M normal draws of a 1024^2 generator cost 0.4 s of host time, a quarter of a warm generate() of 900 frames;
    the reference draws them and throws them away, models/stylegan2.py:455-459 — the only observable difference is that the CPU
    generator's state is not advanced by the construction)."""
    return th.empty(*shape) if getattr(_SKIP_INIT, "on", False) else th.randn(*shape)


class EqualLinear(nn.Module):
    """reference :123-146 (mapping network / standalone use; the per-layer modulations inside the generator forward
    go through the table-driven style kernel instead)."""

    def __init__(self, in_dim, out_dim, bias=True, bias_init=0, lr_mul=1, activation=None):
        super().__init__()
        self.weight = nn.Parameter(_randn(out_dim, in_dim).div_(lr_mul))
        self.bias = nn.Parameter(th.zeros(out_dim).fill_(bias_init)) if bias else None
        self.activation = activation
        self.scale = (1 / math.sqrt(in_dim)) * lr_mul
        self.lr_mul = lr_mul

    def forward(self, inputs):
        if self.activation:
            out = F.linear(inputs, self.weight * self.scale)
            return fused_leaky_relu(out, self.bias * self.lr_mul)
        return F.linear(inputs, self.weight * self.scale, bias=self.bias * self.lr_mul)


DEMOD_MAX_CIN = 1024  # maua_demod_f32 (include/maua_hip.h): [16][cin] squared styles in 64 KB of LDS, 16 values per lane


def _check_demod_cin(cin):
    """maua_demod_f32 cannot see its table (it lives in device memory), so the limit of a demodulated entry is enforced where the table is
    built: wider, demod_kernel would write past its LDS and drop terms without any error."""
    if cin > DEMOD_MAX_CIN:
        raise NotImplementedError(f"demodulation is built for at most {DEMOD_MAX_CIN} input channels (got {cin}): maua_demod_f32 keeps "
                                  "the squared styles of 16 frames in 64 KB of LDS")


def _style_table(entries, device):
    """entries: list of dict(mod_w, mod_b, wsq|None, cin, cout, lat_idx, s_off, d_off, wscale) -> device byte tensor.  Raises for a
    demodulated entry (wsq given) wider than DEMOD_MAX_CIN, before anything is uploaded."""
    for e in entries:
        if e["wsq"] is not None:
            _check_demod_cin(e["cin"])
    arr = (_lib.StyleLayer * len(entries))()
    for i, e in enumerate(entries):
        arr[i].mod_w = e["mod_w"].data_ptr()
        arr[i].mod_b = e["mod_b"].data_ptr()
        arr[i].wsq = e["wsq"].data_ptr() if e["wsq"] is not None else None
        arr[i].cin, arr[i].cout, arr[i].lat_idx = e["cin"], e["cout"], e["lat_idx"]
        arr[i].s_off, arr[i].d_off, arr[i].wscale = e["s_off"], e["d_off"], e["wscale"]
    raw = th.frombuffer(bytearray(bytes(arr)), dtype=th.uint8).clone()
    return raw.to(device)


def _round_up(n, multiple):
    return (n + multiple - 1) // multiple * multiple


def _noise_stride(noise):
    """Batch stride (floats) of a [B or 1, 1, oh, ow] noise map as the kernels take it: 0 = one map shared by the batch (or no map)."""
    return 0 if noise is None or noise.shape[0] == 1 else noise.shape[-1] * noise.shape[-2]


def _checked_noise(noise, batch, oh, ow, src):
    """(noise map or None, its batch stride) for a layer that stores [batch, *, oh, ow]; ``noise`` is ignored with a frame source ``src``."""
    if src is not None or noise is None:
        return None, 0
    noise = _lib.require_cuda(noise, "noise")
    # the kernels read oh*ow floats per sample (batch samples unless the map is shared): a wrongly sized map would be
    # a silent out-of-bounds read where the reference raises a broadcast error (models/stylegan2.py:266)
    if noise.dim() != 4 or noise.shape[1] != 1 or tuple(noise.shape[-2:]) != (oh, ow) or noise.shape[0] not in (1, batch):
        raise RuntimeError(f"noise {tuple(noise.shape)} does not match feature map [{batch}, 1, {oh}, {ow}] (batch must be 1 or {batch})")
    return noise, _noise_stride(noise)  # (require_cuda made it contiguous)


class ModulatedConv2d(nn.Module):
    """reference :164-254.  ``forward(inputs, style)`` keeps the reference contract; the generator calls
    ``run(...)`` with styles / demod factors already computed for all layers."""

    def __init__(self, in_channel, out_channel, kernel_size, style_dim, demodulate=True, upsample=False,
                 downsample=False, blur_kernel=[1, 3, 3, 1]):
        super().__init__()
        if downsample:
            raise NotImplementedError("downsample=True is discriminator-only (SURVEY.md §2 row 4: out of scope)")
        if kernel_size not in (1, 3):
            raise NotImplementedError("the generator only uses 3x3 and 1x1 modulated convolutions")
        self.eps = 1e-8
        self.kernel_size = kernel_size
        self.in_channel = in_channel
        self.out_channel = out_channel
        self.upsample = upsample
        self.downsample = downsample
        if upsample:
            factor = 2
            p = (len(blur_kernel) - factor) - (kernel_size - 1)
            self.blur = Blur(blur_kernel, pad=((p + 1) // 2 + factor - 1, p // 2 + 1), upsample_factor=factor)
        self.scale = 1 / math.sqrt(in_channel * kernel_size ** 2)
        self.padding = kernel_size // 2
        self.weight = nn.Parameter(_randn(1, out_channel, in_channel, kernel_size, kernel_size))
        self.modulation = EqualLinear(style_dim, in_channel, bias_init=1)
        self.demodulate = demodulate
        self._packed = None  # (key, wp, wsq)
        self._packed_wino = None

    def __repr__(self):
        return (f"{self.__class__.__name__}({self.in_channel}, {self.out_channel}, {self.kernel_size}, "
                f"upsample={self.upsample}, downsample={self.downsample})")

    def packed(self):
        """Tap-major repack + per-(o,i) squared-tap sums of the shared weight; rebuilt when the parameter changes
        (model rewriting, render.py:160-167, swaps the Parameter object)."""
        w = self.weight
        key = (w.data_ptr(), w._version, str(w.device))
        if self._packed is None or self._packed[0] != key:
            wd = _lib.require_cuda(w.detach(), "weight")
            k2 = self.kernel_size ** 2
            cpad = _round_up(self.out_channel, 32)
            wp = th.empty((k2, self.in_channel, cpad), dtype=th.float32, device=w.device) if k2 == 9 else None
            wsq = th.empty((self.out_channel, self.in_channel), dtype=th.float32, device=w.device)
            with th.cuda.device(w.device):
                rc = _lib.load().maua_pack_weight_f32(wd.data_ptr(), _lib.ptr(wp), wsq.data_ptr(), self.out_channel,
                                                      self.in_channel, k2, _lib.stream_ptr(w.device))
            _lib.check(rc, "maua_pack_weight_f32")
            self._packed = (key, wp, wsq)
            self._packed_wino = None
        return self._packed[1], self._packed[2]

    # plain 3x3 layers with at least this many output channels run through Winograd F(2,3) (MFMA-bound layers);
    # a huge value turns it off
    winograd_min_cout = 32
    # ... on the maps below 32 x 32 from this many output channels (a huge value turns it off there)
    winograd_small_min_cout = 128
    # ... and from this many output channels, on maps at least this wide, through F(4,3) (6 products per 4 outputs)
    winograd43_min_cout = 32
    winograd43_min_width = 32
    # transposed layers: F(2,2) on the even x-phase (mode 4) where the launch is large enough, see conv_mode
    upconv_winograd = True
    # plain layers whose shape the 2-D Winograd kernel accepts (csrc/modconv_w2d.hip, mode 5: F(2,3) along y on top of
    # F(4,3) along x, 3 instead of 4.5 MFMA products per output) with at least this many output channels.  Measured inside
    # bench.py (profiles/r02_w2d.md): -11..24 % per launch on the 128..512-channel layers; -14 % on the 64-channel and -1 % on
    # the 32-channel layer with the fused ToRGB epilogue (since the skip-image taps of that epilogue are unconditional loads),
    # +1.8 % frames/s for the whole generator.
    winograd2d_min_cout = 32
    # transposed layers whose shape csrc/modconv_up2d.hip accepts (mode 6: F(2,2) on both axes of the polyphase form, 25 instead of
    # 30 (mode 4) / 36 (mode 1) products per 2x2 positions) with at least this many output channels; a huge value turns it off
    upwino2d_min_cout = 32
    # SIDE MEASUREMENT, off by default (a huge value): plain layers with at least this many output channels whose shape
    # csrc/modconv_sbf16.hip accepts run the direct 9-tap form with split-bf16 products on the bf16 matrix cores (mode 7) instead of the
    # fp32 2-D Winograd kernel.  bench.py lowers it for its `split_bf16` side figure; the headline path computes in fp32.
    split_bf16_min_cout = 1 << 30
    # ... and the same for the transposed layers (mode 8: the four polyphase output phases as four launches of the same kernel + the
    # fp32 edge lines)
    split_bf16_up_min_cout = 1 << 30

    def conv_mode(self, h, w):
        """Kernel mode of maua_modconv3x3_f32 for an [*, Cin, h, w] input: 1 / 4 / 6 transposed, 2 Winograd F(2,3), 3 Winograd
        F(4,3), 5 2-D Winograd F(2x4,3x3), 0 direct; 7 / 8 = the split-bf16 side measurement (plain / transposed), off by default."""
        if self.upsample and self.out_channel >= self.split_bf16_up_min_cout and _lib.load().maua_modconv_sbf16_up_ok(
                self.in_channel, self.out_channel, h, w):
            return 8
        if self.upsample and self.out_channel >= self.upwino2d_min_cout and _lib.load().maua_modconv_up2d_ok(
                self.in_channel, self.out_channel, h, w):
            return 6
        if self.upsample:
            # F(2,2) on the even x-phase of the polyphase transposed conv (mode 4: -17 % MFMA work, but 2 instead of 3-4
            # workgroups per CU) once a batch of 8 frames yields at least ~4 rounds of workgroups; smaller grids lose more
            # to the partially filled last round than they gain and keep the plain polyphase kernel (mode 1)
            pairs_per_tile, rows_per_tile = (128, 32) if self.out_channel <= 32 else (64, 64)
            tiles = -(-((h + 1) * (w // 2 + 1)) // pairs_per_tile) * -(-self.out_channel // rows_per_tile)
            if self.upconv_winograd and w % 2 == 0 and tiles >= 256:
                return 4
            return 1
        if self.out_channel >= self.split_bf16_min_cout and _lib.load().maua_modconv_sbf16_ok(self.in_channel, self.out_channel, h, w):
            return 7
        # (the Winograd kernels want at least one full 128-position tile per image; shorter maps would pack several images
        # into a tile, which only the direct mode implements)
        if (self.out_channel >= self.winograd2d_min_cout
                and _lib.load().maua_modconv_w2d_ok(self.in_channel, self.out_channel, h, w)):
            return 5
        if (self.out_channel >= self.winograd43_min_cout and w % 4 == 0 and w >= self.winograd43_min_width
                and h * (w // 4) >= 128):
            return 3
        if self.out_channel >= self.winograd_min_cout and w % 2 == 0 and w >= 32 and h * (w // 2) >= 128:
            return 2
        # the 8^2 / 16^2 layers of a generator (128 and more channels: the 128 x 64 Winograd tile, several images per tile at 8^2): F(2,3) as well —
        # 50 -> 41 us at 8^2, 103 -> 75 us at 16^2 for 512 channels at batch 8 (tools/plain_mode_probe.py, round 6)
        if self.out_channel >= self.winograd_small_min_cout and w % 2 == 0 and 8 <= w < 32 and h >= 8:
            return 2
        return 0

    def blur_is_separable(self):
        """True when the Blur's tap matrix is 4 x 4 and an outer product (make_kernel of 1-D taps always is; a checkpoint could carry
        anything): what maua_upconv_blur_f32 requires.  One host read per (buffer, version), made by the eager warm-up forward — never
        inside a capture."""
        k = self.blur.kernel
        key = (k.data_ptr(), k._version, str(k.device))
        cached = self.__dict__.get("_blur_sep")
        if cached is None or cached[0] != key:
            kk = k.detach().double().cpu()
            ok = tuple(kk.shape) == (4, 4) and float(kk.sum()) != 0.0
            if ok:
                outer = kk.sum(1)[:, None] * kk.sum(0)[None, :] / kk.sum()
                ok = bool((outer - kk).abs().max() <= 1e-6 * kk.abs().max())
            self.__dict__["_blur_sep"] = cached = (key, ok)
        return cached[1]

    # packed_wino: mode -> (pack entry, shape of the packed buffer for a layer ``m``, dtype).  Modes 2 / 3 above 32 channels: columns
    # padded to 64 and interleaved [lane][m-tile] (see pack_weight_wino_kernel), else padded to 32.
    _WINO_PACKS = {
        2: ("maua_pack_weight_wino_f32", lambda m: (12, m.in_channel, _round_up(m.out_channel, 64 if m.out_channel > 32 else 32)), th.float32),
        3: ("maua_pack_weight_wino43_f32", lambda m: (18, m.in_channel, _round_up(m.out_channel, 64 if m.out_channel > 32 else 32)), th.float32),
        4: ("maua_pack_weight_upwino_f32", lambda m: (12, m.in_channel, _round_up(m.out_channel, 32)), th.float32),
        5: ("maua_pack_weight_wino2d_f32", lambda m: (24 * m.in_channel * m.out_channel,), th.float32),
        6: ("maua_pack_weight_up2d_f32", lambda m: (_lib.load().maua_pack_weight_up2d_floats(m.out_channel, m.in_channel),), th.float32),
        7: ("maua_pack_weight_sbf16_f32", lambda m: (_lib.load().maua_pack_weight_sbf16_bytes(m.out_channel, m.in_channel),), th.uint8),
    }

    def packed_wino(self, mode=2):
        """Weight in the form the kernel of ``mode`` reads (``_WINO_PACKS``): Winograd-domain [(ky*F+xi), Cin, Cout_pad] with F = 4 for
        modes 2 and 4, 6 for mode 3; the layouts of csrc/modconv_w2d.hip (5), modconv_up2d.hip (6), modconv_sbf16.hip (7 / 8).  Cached like
        ``packed()``."""
        self.packed()  # refreshes / invalidates on weight change
        if self._packed_wino is None:
            self._packed_wino = {}
        if mode == 8:
            mode = 7  # (one packed weight serves the plain and the transposed form)
        if mode not in self._packed_wino:
            fn, shape, dtype = self._WINO_PACKS[mode]
            w = self.weight
            wd = _lib.require_cuda(w.detach(), "weight")
            wq = th.empty(shape(self), dtype=dtype, device=w.device)
            with th.cuda.device(w.device):
                rc = getattr(_lib.load(), fn)(wd.data_ptr(), wq.data_ptr(), self.out_channel, self.in_channel, _lib.stream_ptr(w.device))
            _lib.check(rc, fn)
            self._packed_wino[mode] = wq
        return self._packed_wino[mode]

    def weight_for(self, mode):
        """The packed weight the kernel of ``mode`` reads: tap-major for the direct and polyphase kernels (0, 1), ``packed_wino`` above."""
        return self.packed_wino(mode) if mode >= 2 else self.packed()[0]

    def table_entry(self, lat_idx, s_off, d_off):
        wp, wsq = self.packed()
        return dict(mod_w=self.modulation.weight, mod_b=self.modulation.bias, wsq=wsq if self.demodulate else None,
                    cin=self.in_channel, cout=self.out_channel, lat_idx=lat_idx, s_off=s_off, d_off=d_off,
                    wscale=self.scale)

    def run(self, x, s, s_off, d, out, ws, fuse_act=False, noise=None, noise_w=None, bias=None, src=None, slot=0, prescaled=False, mode=None):
        """3x3 only. x [B,Cin,H,W]; s [B,S] (this layer's slice at s_off); d [B,Cout] or None.
        Writes ``out`` ([B,Cout,H,W] or [B,Cout,2H+1,2W+1] when upsample).  ``src`` (device pointer of a frame source,
        include/maua_hip.h): the noise map comes from its slot ``slot`` instead of ``noise``.  ``prescaled``: x arrives multiplied by
        this layer's styles (the style fold, include/maua_hip.h; modes 5 and 6 only).  ``mode``: ``conv_mode(H, W)``, if the caller has it."""
        lib = _lib.load()
        b, cin, h, w = x.shape
        if mode is None:
            mode = self.conv_mode(h, w)
        rc = lib.maua_modconv3x3_f32(
            x.data_ptr(), self.weight_for(mode).data_ptr(), None if prescaled else s.data_ptr() + 4 * s_off, s.shape[1], _lib.ptr(d),
            out.data_ptr(), b, cin, self.out_channel, h, w, mode, float(self.scale), int(fuse_act), _lib.ptr(noise), _noise_stride(noise),
            _lib.ptr(noise_w), _lib.ptr(bias), _lib.ptr(ws), src if fuse_act else None, slot, _lib.stream_ptr(x.device),
        )
        _lib.check(rc, "maua_modconv3x3_f32")
        return out

    def forward(self, inputs, style):
        x, s, d = _layer_styles(self, inputs, style)
        b, cin, h, w = x.shape
        dev = x.device
        lib = _lib.load()
        with th.cuda.device(dev):
            if self.kernel_size == 1:
                if self.out_channel != 3 or self.demodulate:
                    raise NotImplementedError("1x1 modulated conv is only built for ToRGB (3 channels, no demodulation)")
                out = th.empty((b, 3, h, w), dtype=th.float32, device=dev)
                _lib.check(lib.maua_torgb_f32(x.data_ptr(), self.weight.data_ptr(), s.data_ptr(), cin, None, None, None,
                                              out.data_ptr(), b, cin, h, w, float(self.scale), _lib.stream_ptr(dev)), "maua_torgb_f32")
                return out
            oh, ow = (2 * h + 1, 2 * w + 1) if self.upsample else (h, w)
            out = th.empty((b, self.out_channel, oh, ow), dtype=th.float32, device=dev)
            n_ws = lib.maua_modconv_ws_floats(b, cin, self.out_channel, h, w, self.conv_mode(h, w))
            ws = th.empty(n_ws, dtype=th.float32, device=dev) if n_ws else None
            self.run(x, s, 0, d, out, ws)
            if self.upsample:
                out = self.blur(out)
        return out


def _layer_styles(conv, inputs, style):
    """(checked inputs, s [batch, Cin], d [batch, Cout] or None when ``conv`` does not demodulate) of ONE ModulatedConv2d for ``style``
    [batch, style_dim]: the one-entry form of the generator's style table, for the standalone ``forward`` of the layer classes."""
    cin, cout = conv.in_channel, conv.out_channel
    if conv.demodulate:
        _check_demod_cin(cin)  # (before the weight pack and every other launch)
    lib = _lib.load()
    x, style = _lib.require_cuda(inputs, "inputs"), _lib.require_cuda(style, "style")
    batch, dev = x.shape[0], x.device
    s = th.empty((batch, cin), dtype=th.float32, device=dev)
    d = th.empty((batch, cout), dtype=th.float32, device=dev) if conv.demodulate else None
    with th.cuda.device(dev):
        table = _style_table([conv.table_entry(0, 0, 0)], dev)
        lat = style.reshape(batch, 1, -1)
        st = _lib.stream_ptr(dev)
        _lib.check(lib.maua_style_affine_f32(lat.data_ptr(), batch, 1, lat.shape[-1], None, None, table.data_ptr(), 1, cin, s.data_ptr(), cin,
                                             None, st), "maua_style_affine_f32")
        if d is not None:
            _lib.check(lib.maua_demod_f32(table.data_ptr(), 1, cout, s.data_ptr(), cin, d.data_ptr(), batch, st), "maua_demod_f32")
    return x, s, d


class NoiseInjection(nn.Module):
    """reference :257-266 (standalone; inside StyledConv the add is fused into the conv / blur epilogue)."""

    def __init__(self):
        super().__init__()
        self.weight = nn.Parameter(th.zeros(1))

    def forward(self, image, noise=None):
        if noise is None:
            batch, _, height, width = image.shape
            noise = image.new_empty(batch, 1, height, width).normal_()
        return image + self.weight * noise.to(image.device)


class ConstantInput(nn.Module):
    def __init__(self, channel, size=4):
        super().__init__()
        self.input = nn.Parameter(_randn(1, channel, size, size))

    def forward(self, inputs):
        return self.input.repeat(inputs.shape[0], 1, 1, 1)


class LatentInput(nn.Module):
    """reference :281-294 (``--noconst`` checkpoints): the 4x4 input is an affine function of the first latent row,
    ``activate(fused_lrelu(EqualLinear(latent[:, 0])))`` reshaped to [B, C, 4, 4].  State-dict keys as the reference:
    input.linear.{weight,bias}, input.activate.bias, input.input (an unused scalar Parameter that only carries the device)."""

    def __init__(self, latent_dim, channel, size=4):
        super().__init__()
        self.channel = channel
        self.size = size
        self.linear = EqualLinear(latent_dim, channel * size * size, activation="fused_lrelu")
        self.activate = FusedLeakyReLU(channel * size * size)
        self.input = nn.Parameter(th.randn(1))

    def forward(self, inputs):
        out = self.activate(self.linear(inputs[:, 0]))
        return out.reshape((inputs.shape[0], self.channel, self.size, self.size))

    def run(self, latent, trunc, tl, out, src=None, n_latent=None, style_dim=None):
        """Device path on static buffers (capturable): the table-driven affine kernel (truncation lerp included) writes
        W x / sqrt(dim) + b into ``out`` [B, C*16]; two in-place bias-act launches apply lrelu*sqrt2 and the second
        bias + lrelu*sqrt2.  ``src``: the latents / truncation come from the frame source instead of ``latent`` / ``trunc``."""
        lib = _lib.load()
        dev = out.device
        n_out = self.channel * self.size * self.size
        batch = out.shape[0]
        if latent is not None:
            n_latent, style_dim = latent.shape[1], latent.shape[2]
        key = (self.linear.weight.data_ptr(), self.linear.bias.data_ptr(), str(dev))
        if getattr(self, "_table", None) is None or self._table[0] != key:
            entry = dict(mod_w=self.linear.weight, mod_b=self.linear.bias, wsq=None, cin=n_out, cout=0, lat_idx=0, s_off=0,
                         d_off=0, wscale=1.0)
            self._table = (key, _style_table([entry], dev))
        st = _lib.stream_ptr(dev)
        flat = out.view(batch, n_out)
        _lib.check(lib.maua_style_affine_f32(_lib.ptr(latent), batch, n_latent, style_dim, _lib.ptr(trunc),
                                             _lib.ptr(tl), self._table[1].data_ptr(), 1, n_out, flat.data_ptr(), n_out, src, st),
                   "maua_style_affine_f32")
        _lib.check(lib.maua_fused_bias_act_f32(flat.data_ptr(), None, None, flat.data_ptr(), flat.numel(), 0, 1, 3, 0, 0.2,
                                               2 ** 0.5, st), "maua_fused_bias_act_f32")
        _lib.check(lib.maua_fused_bias_act_f32(flat.data_ptr(), self.activate.bias.data_ptr(), None, flat.data_ptr(),
                                               flat.numel(), n_out, 1, 3, 0, self.activate.negative_slope,
                                               self.activate.scale, st), "maua_fused_bias_act_f32")
        return out


class ManipulationLayer(nn.Module):
    """reference :297-307 — applies every transform whose "layer" id matches."""

    def __init__(self, layer):
        super().__init__()
        self.layer = layer

    def forward(self, input, tranforms_dict_list):
        out = input
        for transform_dict in tranforms_dict_list:
            if transform_dict["layer"] == self.layer:
                out = transform_dict["transform"].to(out.device)(out)
        return out

    def run(self, x, bends, bufs, tag, src=None):
        """Device path.  Eager (``src`` None): as ``forward``.  Inside a captured forward every bend is a module with the
        ``run_static(x, out, src)`` protocol (audioreactive/bend.py): it writes into a static buffer and reads its per-frame
        parameters through the frame source, so one captured graph serves every batch of the render.  A bend that changes the map's
        shape (audioreactive/bend.py: Pad) gives the shape of its output through ``static_shape``."""
        if src is None:
            return self.forward(x, bends)
        for i, bd in enumerate(bends):
            if bd["layer"] == self.layer:
                transform = bd["transform"]
                shape = transform.static_shape(tuple(x.shape)) if hasattr(transform, "static_shape") else tuple(x.shape)
                x = transform.run_static(x, bufs(f"{tag}.bend{i}", shape), src)
        return x


class StyledConv(nn.Module):
    """reference :310-343: ModulatedConv2d -> NoiseInjection -> FusedLeakyReLU -> ManipulationLayer."""

    def __init__(self, in_channel, out_channel, kernel_size, style_dim, upsample=False, blur_kernel=[1, 3, 3, 1],
                 demodulate=True, layerID=-1):
        super().__init__()
        self.conv = ModulatedConv2d(in_channel, out_channel, kernel_size, style_dim, upsample=upsample,
                                    blur_kernel=blur_kernel, demodulate=demodulate)
        self.noise = NoiseInjection()
        self.activate = FusedLeakyReLU(out_channel)
        self.manipulation = ManipulationLayer(layerID)

    # layers wider than one weight tile on the 2-D Winograd kernel leave per-tile partial ToRGB sums (A/B switch)
    partial_rgb_fusion = True
    # up-sampling layers whose INPUT is at least this wide run transposed convolution + blur + noise + bias + activation as one kernel
    # (maua_upconv_blur_f32, round 5): convs.14 (0.82 ms against the pair's 1.01) and convs.12 (level alone, +0.8 % frames/s inside the
    # overlapped pipeline, where the raw map's round trip competes for HBM); below, the extra tiles of its overlapped tiling cost more than
    # that round trip saves (convs.10: 0.70 against 0.56 ms; profiles/r05_fused_upconv_blur.md).  A huge value = always the two-launch path.
    fused_blur_min_width = 256
    # the 4^2 .. 32^2 layers (split-K direct / polyphase kernels): the convolution leaves its split-K slabs and ONE more launch reduces them
    # together with what follows — blur + noise + bias + activation of an up-sampling layer (maua_upconv_blur_lowres_f32), tail + per-group
    # partial ToRGB sums of a plain one (maua_styledconv_rgbpart_lowres_f32) — instead of reduce, then blur / ToRGB (A/B switch)
    lowres_fusion = True
    # ... and the 16-wide up-sampling layer among them on the F(2,2)^2 kernel (16 x 16-position tiles, K split) instead of the polyphase one (A/B switch)
    lowres_up2d = True

    def accepts_prescaled(self, h, w):
        """True when this layer's convolution has a kernel instance without the style multiplies for an [*, Cin, h, w] input (the style
        fold, include/maua_hip.h: the 2-D Winograd kernels, mode 5, and the F(2,2)^2 transposed kernel, mode 6, fused with its blur or not)."""
        return self.conv.conv_mode(h, w) in (5, 6)

    # what the last call of ``run`` did: its path ("torgb", "rgb_partial", "lowres", "plain" on a plain layer, "fused", "lowres", "pair" on an
    # up-sampling one, "const" for conv1 through Generator._run_const_conv) and whether the map it stored carries the consumer's styles
    last_path = None
    posted = False

    def _took(self, path, out, posted=False, rgb=None, u8_done=True):
        """The one place where a call reports what it did: every exit of ``run`` (and of Generator._run_const_conv) returns through here.
        ``rgb``: the offer that was taken; ``u8_done`` False: its image is in rgb["out"] as fp32 planes (a last layer still needs the frame epilogue)."""
        self.last_path, self.posted = path, posted
        if rgb is not None:
            rgb["done"] = True
            if not u8_done:
                rgb["u8_done"] = False
        return out

    @staticmethod
    def _rgb_operands(rgb, s):
        """(ToRGB weight, its styles inside ``s``, its weight scale) as the ToRGB-fused kernels take them; NULLs without an offer."""
        if rgb is None:
            return None, None, 0.0
        t = rgb["module"]
        return t.conv.weight.data_ptr(), s.data_ptr() + 4 * rgb["s_off"], float(t.conv.scale)

    def run(self, x, s, s_off, d, noise, bufs, tag, rgb=None, src=None, slot=0, prescaled=False, post_off=None):
        """Fused forward on precomputed styles. ``bufs(name, shape)`` hands out static device buffers.
        The style fold (include/maua_hip.h): ``prescaled`` = x arrives multiplied by this layer's styles (the producer applied them);
        ``post_off`` = offset inside ``s`` of the styles of the layer that consumes this layer's output: where this layer's path can, it
        stores its map multiplied by them and sets ``self.posted`` (the consumer is then run with ``prescaled``).
        ``src`` / ``slot``: the noise map is read through the frame source (``noise`` is then ignored and may be None).
        ``rgb`` (plain layers only) offers the following ToRGB for folding into this layer's launches.  Keys in: ``module`` (the ToRGB),
        ``s_off`` (its styles inside ``s``), ``skip`` (the image of the resolution below, or None), ``out`` ([B, 3, H, W] image buffer),
        ``store`` (False: the feature map itself is not needed — single-launch path only), ``u8`` ([B, H, W, 3] uint8 frames that the
        single-launch path writes instead of ``out``) and ``tap`` (write ``out`` as well as ``u8``).  Keys out: ``done`` = the image was
        produced here (the caller runs no ToRGB pass), ``u8_done`` = False when it is in ``out`` as fp32 planes although ``u8`` was offered.
        The call reports its path in ``self.last_path``; the paths are tried in the order below, each launches or declines."""
        lib = _lib.load()
        conv = self.conv
        b, cin, h, w = x.shape
        up = 2 if conv.upsample else 1
        mode = conv.conv_mode(h, w)
        noise, nstride = _checked_noise(noise, b, up * h, up * w, src)
        c = SimpleNamespace(x=x, s=s, s_off=s_off, d=d, bufs=bufs, tag=tag, rgb=rgb, src=src, slot=slot, prescaled=prescaled, noise=noise,
                            dims=(b, cin, conv.out_channel, h, w), mode=mode, st=_lib.stream_ptr(x.device))
        # one split-K workspace PER LAYER (tag + ".ws", for the paths that run the convolution on its own): a shared name would be
        # re-allocated whenever the size changes, and a captured hipGraph keeps writing through the pointer of the buffer that was freed
        c.n_ws = lib.maua_modconv_ws_floats(*c.dims, mode)
        c.low = (self.lowres_fusion and not prescaled and mode in ((1,) if conv.upsample else (0, 2, 3))
                 and lib.maua_lowres_ok(*c.dims[1:], mode))
        # (input, packed weight of ``mode``, styles or NULL when the input carries them, their row stride, demodulation) as every fused entry
        # takes them; a function, so that the path that launches packs the weight (the one-time pack launch keeps its place in the stream)
        c.head = lambda mode=mode: (x.data_ptr(), conv.weight_for(mode).data_ptr(), None if prescaled else s.data_ptr() + 4 * s_off,  # noqa: E731
                                    s.shape[1], _lib.ptr(d))
        c.post_ptr = None if post_off is None else s.data_ptr() + 4 * post_off
        c.tail = (_lib.ptr(noise), nstride, self.noise.weight.data_ptr(), self.activate.bias.data_ptr())  # noise + bias + activation
        if conv.upsample:
            paths = (self._up_fused, self._up_lowres, self._up_pair)
        else:
            c.out = bufs(tag, (b, conv.out_channel, h, w))
            c.rgb_ok = rgb is not None and rgb["module"].skip_fusable(rgb["skip"], h, w)  # the offer can be taken in-launch
            c.rgb_w = self._rgb_operands(rgb, s)
            paths = (self._torgb, self._rgb_partial, self._lowres_rgb, self._plain)
        for path in paths:
            out = path(c)
            if out is not None:
                return out

    def _torgb(self, c):
        """Layers of at most 64 channels: ToRGB (+ on the last layer the uint8 frame epilogue) in the convolution's epilogue, one launch."""
        conv, rgb = self.conv, c.rgb
        if not (c.rgb_ok and conv.out_channel <= 64 and c.n_ws == 0):
            return None
        t = rgb["module"]
        post = c.post_ptr if c.mode == 5 else None
        rc = _lib.load().maua_styledconv_torgb_f32(
            *c.head(), c.out.data_ptr(), *c.dims, c.mode, float(conv.scale), *c.tail, *c.rgb_w, t.bias.data_ptr(), *t.skip_operands(rgb["skip"]),
            rgb["out"].data_ptr() if (rgb.get("u8") is None or rgb.get("tap")) else None,
            int(rgb.get("store", True)), _lib.ptr(rgb.get("u8")), c.src, c.slot, post, c.st)
        if rc == -38:  # MAUA_ENOSYS = layer shape not fusable (the library's tile plan decides) -> the paths below
            return None
        _lib.check(rc, "maua_styledconv_torgb_f32")
        return self._took("torgb", c.out, post is not None, rgb)

    def _rgb_partial(self, c):
        """Wider layers on the 2-D Winograd kernel: every output-channel tile leaves its share of the ToRGB sum (3 planes); the ToRGB pass
        then adds 3 * m_tiles planes (+ bias, + up-sampled skip) instead of reading all ``cout`` feature planes."""
        conv, rgb = self.conv, c.rgb
        # (up to 64 channels the single-launch path above is the only ToRGB fusion that is tried)
        b, cin, cout, h, w = c.dims
        if not (c.rgb_ok and cout > 64 and self.partial_rgb_fusion and c.n_ws == 0 and c.mode == 5):
            return None
        m_tiles = _lib.load().maua_modconv_w2d_mtiles(cin, cout, h, w)
        if m_tiles <= 1:
            return None
        part = c.bufs(c.tag + ".rgb_partial", (b, 3 * m_tiles, h, w))
        _lib.check(_lib.load().maua_styledconv_torgb_partial_f32(
            *c.head(), c.out.data_ptr(), *c.dims, 5, float(conv.scale), *c.tail, *c.rgb_w, part.data_ptr(), c.src, c.slot, c.post_ptr, c.st),
            "maua_styledconv_torgb_partial_f32")
        rgb["module"].run(part, None, 0, rgb["skip"], rgb["out"])
        return self._took("rgb_partial", c.out, c.post_ptr is not None, rgb, u8_done=False)

    def _lowres_rgb(self, c):
        """Low-resolution entry of a plain layer: convolution -> split-K slabs, ONE launch for slab sum + tail + per-group partial ToRGB
        sums (maua_styledconv_rgbpart_lowres_f32), then the plane sum."""
        conv, rgb = self.conv, c.rgb
        b, cin, cout, h, w = c.dims
        if not (c.low and c.rgb_ok and self.partial_rgb_fusion and w % 4 == 0 and c.post_ptr is None):
            return None
        lib = _lib.load()
        lws = c.bufs(c.tag + ".lws", (lib.maua_lowres_ws_floats(*c.dims, c.mode),))
        part = c.bufs(c.tag + ".rgb_partial", (b, 3 * (cout // 32), h, w))
        _lib.check(lib.maua_styledconv_rgbpart_lowres_f32(
            *c.head(), c.out.data_ptr(), lws.data_ptr(), *c.tail, *c.rgb_w, part.data_ptr(), c.src, c.slot, *c.dims, c.mode, float(conv.scale),
            c.st), "maua_styledconv_rgbpart_lowres_f32")
        rgb["module"].run(part, None, 0, rgb["skip"], rgb["out"])
        return self._took("lowres", c.out, rgb=rgb, u8_done=False)

    def _plain(self, c):
        """Convolution with noise + bias + activation in its epilogue; an offered ToRGB is left to the caller."""
        ws = c.bufs(c.tag + ".ws", (c.n_ws,)) if c.n_ws else None
        self.conv.run(c.x, c.s, c.s_off, c.d, c.out, ws, fuse_act=True, noise=c.noise, noise_w=self.noise.weight,
                      bias=self.activate.bias, src=c.src, slot=c.slot, prescaled=c.prescaled, mode=c.mode)
        return self._took("plain", c.out)

    def _up_fused(self, c):
        """The whole layer in one pass over the transposed convolution's accumulators: no raw (2H+1) x (2W+1) map (csrc/modconv_up2d.hip)."""
        conv, lib = self.conv, _lib.load()
        b, cin, cout, h, w = c.dims
        if not (self.fused_blur_min_width <= w and c.mode == 6 and tuple(conv.blur.pad) == (1, 1) and conv.blur_is_separable()
                and lib.maua_upconv_blur_ok(cin, cout, h, w)):
            return None
        out = c.bufs(c.tag, (b, cout, 2 * h, 2 * w))
        n_seam = lib.maua_upconv_blur_ws_floats(*c.dims)
        seam = c.bufs(c.tag + ".seam", (n_seam,)) if n_seam else None
        _lib.check(lib.maua_upconv_blur_f32(
            *c.head(), out.data_ptr(), _lib.ptr(seam), conv.blur.kernel.data_ptr(), *c.tail, c.src, c.slot, *c.dims, float(conv.scale),
            c.post_ptr, c.st), "maua_upconv_blur_f32")
        return self._took("fused", out, c.post_ptr is not None)

    def _up_lowres(self, c):
        """Low-resolution entry of an up-sampling layer: transposed convolution -> split-K slabs, then ONE launch: slab sum, demodulation,
        blur, noise, bias, leaky ReLU (+ the style fold's scale)."""
        conv, lib = self.conv, _lib.load()
        b, cin, cout, h, w = c.dims
        k = conv.blur.kernel
        if not (c.low and tuple(k.shape) == (4, 4) and tuple(conv.blur.pad) == (1, 1)):
            return None
        # (6 = the F(2,2)^2 kernel on 16-wide inputs where the shape allows it, else 1 = the polyphase kernel, which is ``c.mode`` here)
        low_up = 6 if (self.lowres_up2d and lib.maua_lowres_ok(cin, cout, h, w, 6)) else 1
        out = c.bufs(c.tag, (b, cout, 2 * h, 2 * w))
        lws = c.bufs(c.tag + ".lws", (lib.maua_lowres_ws_floats(*c.dims, low_up),))
        _lib.check(lib.maua_upconv_blur_lowres_f32(
            *c.head(low_up), out.data_ptr(), lws.data_ptr(), k.data_ptr(), *c.tail, c.src, c.slot, *c.dims, low_up,
            float(conv.scale), c.post_ptr, c.st), "maua_upconv_blur_lowres_f32")
        return self._took("lowres", out, c.post_ptr is not None)

    def _up_pair(self, c):
        """Transposed convolution into a raw (2H+1) x (2W+1) map, then blur + noise + bias + activation (+ the style fold's scale)."""
        conv = self.conv
        b, cin, cout, h, w = c.dims
        k = conv.blur.kernel
        pad0, pad1 = conv.blur.pad
        ws = c.bufs(c.tag + ".ws", (c.n_ws,)) if c.n_ws else None
        raw = c.bufs(c.tag + ".raw", (b, cout, 2 * h + 1, 2 * w + 1))
        conv.run(c.x, c.s, c.s_off, c.d, raw, ws, prescaled=c.prescaled, mode=c.mode)
        oh, ow = raw.shape[2] + pad0 + pad1 - k.shape[0] + 1, raw.shape[3] + pad0 + pad1 - k.shape[1] + 1
        out = c.bufs(c.tag, (b, cout, oh, ow))
        rc = _lib.load().maua_blur_noise_act_f32(raw.data_ptr(), k.data_ptr(), out.data_ptr(), b, cout, raw.shape[2], raw.shape[3],
                                                 k.shape[0], k.shape[1], pad0, pad1, None, *c.tail, c.src, c.slot, c.post_ptr,
                                                 c.s.shape[1], c.st)
        _lib.check(rc, "maua_blur_noise_act_f32")
        return self._took("pair", out, c.post_ptr is not None)

    def forward(self, inputs, style, noise=None, transform_dict_list=[]):
        x, s, d = _layer_styles(self.conv, inputs, style)
        b, dev = x.shape[0], x.device
        with th.cuda.device(dev):
            if noise is None:
                up = 2 if self.conv.upsample else 1
                noise = th.randn(b, 1, x.shape[2] * up, x.shape[3] * up, device=dev)
            out = self.run(x, s, 0, d, noise, lambda name, shape: th.empty(shape, dtype=th.float32, device=dev), "out")
        return self.manipulation(out, transform_dict_list)


class ToRGB(nn.Module):
    """reference :346-365."""

    def __init__(self, in_channel, style_dim, upsample=True, blur_kernel=[1, 3, 3, 1]):
        super().__init__()
        if upsample:
            self.upsample = Upsample(blur_kernel)
        self.conv = ModulatedConv2d(in_channel, 3, 1, style_dim, demodulate=False)
        self.bias = nn.Parameter(th.zeros(1, 3, 1, 1))

    def _upsample_is_4tap(self):
        return tuple(self.upsample.kernel.shape) == (4, 4) and self.upsample.factor == 2

    def skip_fusable(self, skip, h, w):
        """True when the kernels can up-sample ``skip`` inside the launch that adds it to an h x w image: no skip at all, or the 4-tap /
        factor-2 Upsample on an image of half the size."""
        return skip is None or (self._upsample_is_4tap() and skip.shape[2] * 2 == h and skip.shape[3] * 2 == w)

    def skip_operands(self, skip):
        """(skip image, taps of its Upsample) as the kernels take them: NULLs without a skip image."""
        return (None, None) if skip is None else (skip.data_ptr(), self.upsample.kernel.data_ptr())

    def run(self, x, s, s_off, skip, out):
        """``s`` None: the plane-sum form of maua_torgb_f32 (w = s = NULL) — ``x`` [B, 3 n, H, W] holds partial ToRGB sums that a convolution
        left, ``out`` = the sum of its 3-plane groups + bias + up-sampled ``skip``."""
        b, cin, h, w = x.shape
        if not self.skip_fusable(skip, h, w):
            if not self._upsample_is_4tap():
                raise NotImplementedError("fused ToRGB skip path is built for the 4-tap / factor-2 Upsample")
            raise RuntimeError(f"skip {tuple(skip.shape)} is not half of {h}x{w}")
        weight = (None, None, 0) if s is None else (self.conv.weight.data_ptr(), s.data_ptr() + 4 * s_off, s.shape[1])
        rc = _lib.load().maua_torgb_f32(x.data_ptr(), *weight, self.bias.data_ptr(), *self.skip_operands(skip), out.data_ptr(), b, cin, h, w,
                                        1.0 if s is None else float(self.conv.scale), _lib.stream_ptr(x.device))
        _lib.check(rc, "maua_torgb_f32")
        return out

    def forward(self, inputs, style, skip=None):
        x, s, _ = _layer_styles(self.conv, inputs, style)
        (b, _, h, w), dev = x.shape, x.device
        with th.cuda.device(dev):
            out = th.empty((b, 3, h, w), dtype=th.float32, device=dev)
            if skip is not None:
                skip = _lib.require_cuda(skip, "skip")
            return self.run(x, s, 0, skip, out)


class Generator(nn.Module):
    """reference :368-576.  ``constant_input=True`` is what load_generator passes by default
    (generate_audiovisual.py:49); ``--noconst`` checkpoints use LatentInput (:281-294,409-412)."""

    def __init__(self, size, style_dim, n_mlp, channel_multiplier=2, blur_kernel=[1, 3, 3, 1], lr_mlp=0.01,
                 constant_input=False, checkpoint=None, output_size=None, min_rgb_size=4, base_res_factor=1):
        super().__init__()
        _SKIP_INIT.on = checkpoint is not None  # (see _randn; thread-local; reset below, also when construction fails)
        try:
            self._build(size, style_dim, n_mlp, channel_multiplier, blur_kernel, lr_mlp, constant_input, min_rgb_size)
        finally:
            _SKIP_INIT.on = False
        self.truncation_latent = None
        if checkpoint is not None:
            try:  # zip-format checkpoints are mapped instead of read (0.1 s for the 120 MB of a 1024^2 generator)
                state = th.load(checkpoint, map_location="cpu", mmap=True)
            except (RuntimeError, ValueError, TypeError):
                state = th.load(checkpoint)
            # the tensors above were left uninitialised: EVERY parameter and buffer must come from the checkpoint (strict load,
            # and the key sets are compared explicitly so that a later relaxation to strict=False cannot leave garbage weights)
            missing = set(self.state_dict().keys()) - set(state["g_ema"].keys())
            if missing:
                raise RuntimeError(f"checkpoint {checkpoint!r} lacks {sorted(missing)[:5]} ... ({len(missing)} tensors): the generator "
                                   "was built without initial values and cannot be completed from it")
            self.load_state_dict(state["g_ema"], strict=True)
        self._random_noise_buffers = size != output_size or base_res_factor != 1
        if self._random_noise_buffers:  # reference :461-470 (resizes only the noise buffers)
            for layer_idx in range(self.num_layers):
                res = (layer_idx + 5) // 2
                shape = [1, 1, int(base_res_factor * 2 ** res * (2 if output_size == 1080 else 1)),
                         int(base_res_factor * 2 ** res * (2 if output_size == 1920 else 1))]
                setattr(self.noises, f"noise_{layer_idx}", th.randn(*shape))
        self._bufs = {}
        self._arena = {}  # (lane, device) -> (current chunk, bytes used): see _arena_tensor
        self._retired = []  # replaced static buffers, kept alive for graphs that still reference them
        self._captured = False
        self._lane = 0  # static-buffer namespace: concurrent hipGraphs of one generator each own a lane
        self._tables = {}

    # parity-test tap: a forward that writes uint8 frames from the last layer's epilogue ALSO leaves the fp32 image of the last
    # resolution (``GraphLane.image``) — the same kernel instance writes both, so the float comparison sees exactly what became the frame
    tap_float_image = False
    # the style fold (include/maua_hip.h THE STYLE FOLD; A/B switch): producers store their map multiplied by the consumer's styles
    style_fold = True
    # every ToRGB as a pass of its own instead of folded into the preceding layer's launches (A/B switch)
    disable_rgb_fusion = False
    # seed of the counter-based noise of a randomised render (render.synthesize, ``random_noise``); None: one draw from torch's CPU
    # generator per render.  ``noise_frame_offset``: absolute index of frame 0 of the sequences a render is given (a rank that holds one
    # shard of a job's frames: render.render_shard sets it), so that frame n of the job gets the same maps on whichever rank.
    noise_seed = None
    noise_frame_offset = 0

    def _build(self, size, style_dim, n_mlp, channel_multiplier, blur_kernel, lr_mlp, constant_input, min_rgb_size):
        self.size = size
        self.style_dim = style_dim
        layers = [PixelNorm()]
        for _ in range(n_mlp):
            layers.append(EqualLinear(style_dim, style_dim, lr_mul=lr_mlp, activation="fused_lrelu"))
        self.style = nn.Sequential(*layers)
        self.channels = {4: 512, 8: 512, 16: 512, 32: 512, 64: 256 * channel_multiplier, 128: 128 * channel_multiplier,
                         256: 64 * channel_multiplier, 512: 32 * channel_multiplier, 1024: 16 * channel_multiplier}
        self.log_size = int(math.log(size, 2))
        self.num_layers = (self.log_size - 2) * 2 + 1
        self.n_latent = self.log_size * 2 - 2
        self.min_rgb_size = min_rgb_size
        self.input = ConstantInput(self.channels[4]) if constant_input else LatentInput(style_dim, self.channels[4])
        self.const_manipulation = ManipulationLayer(0)
        layerID = 1
        self.conv1 = StyledConv(self.channels[4], self.channels[4], 3, style_dim, blur_kernel=blur_kernel, layerID=layerID)
        self.to_rgb1 = ToRGB(self.channels[4], style_dim, upsample=False)
        self.convs = nn.ModuleList()
        self.upsamples = nn.ModuleList()
        self.to_rgbs = nn.ModuleList()
        self.noises = nn.Module()
        in_channel = self.channels[4]
        for layer_idx in range(self.num_layers):
            res = (layer_idx + 5) // 2
            self.noises.register_buffer(f"noise_{layer_idx}", _randn(1, 1, 2 ** res, 2 ** res))
        for i in range(3, self.log_size + 1):
            out_channel = self.channels[2 ** i]
            layerID += 1
            self.convs.append(StyledConv(in_channel, out_channel, 3, style_dim, upsample=True, blur_kernel=blur_kernel,
                                         layerID=layerID))
            layerID += 1
            self.convs.append(StyledConv(out_channel, out_channel, 3, style_dim, blur_kernel=blur_kernel, layerID=layerID))
            self.to_rgbs.append(ToRGB(out_channel, style_dim))
            in_channel = out_channel

    # ------------------------------------------------------------------ helpers shared with the reference API
    def make_noise(self):
        device = self.input.input.device
        noises = [th.randn(1, 1, 4, 4, device=device)]
        for i in range(3, self.log_size + 1):
            for _ in range(2):
                noises.append(th.randn(1, 1, 2 ** i, 2 ** i, device=device))
        return noises

    def mean_latent(self, n_latent):
        latent_in = th.randn(n_latent, self.style_dim, device=self.input.input.device)
        return self.style(latent_in).mean(0, keepdim=True)

    def get_latent(self, inputs):
        return self.style(inputs)

    # ------------------------------------------------------------------ static buffers / tables
    def _buf(self, batch, name, shape, dtype=th.float32):
        """Static device buffer keyed by (batch, name, lane).  A buffer that has to change shape is RETIRED, not freed:
        hipGraphs captured earlier still launch kernels on its address."""
        key = (batch, name, self._lane)
        t = self._bufs.get(key)
        shape = tuple(int(v) for v in shape)
        if t is None or tuple(t.shape) != shape or t.device != self.input.input.device:
            if t is not None and self._captured:
                self._retired.append(t)
            t = self._arena_tensor(shape, dtype)
            self._bufs[key] = t
        return t

    _ARENA_CHUNK = 256 << 20

    def _arena_tensor(self, shape, dtype):
        """Static buffers are carved out of a few large device allocations per lane instead of one allocation each: a 1024^2
        generator owns ~240 buffers per lane, and 720 hipMalloc calls were 0.3-0.4 s of every generate() (the reference's
        `empty_cache()` before the render hands the cached blocks of the previous run back to the driver, so they are real
        allocations each time).  Buffers of half a chunk and more get an allocation of their own; nothing is ever returned to
        an arena (a retired buffer keeps its bytes, hipGraphs captured earlier still write there)."""
        dev = self.input.input.device
        n = 1
        for v in shape:
            n *= v
        nbytes = n * th.empty((), dtype=dtype).element_size()
        aligned = max(256, (nbytes + 255) & ~255)
        if aligned >= self._ARENA_CHUNK // 2:
            raw = th.empty(aligned, dtype=th.uint8, device=dev)
        else:
            key = (self._lane, str(dev))
            chunk, used = self._arena.get(key, (None, 0))
            if chunk is None or used + aligned > chunk.numel():
                chunk, used = th.empty(self._ARENA_CHUNK, dtype=th.uint8, device=dev), 0
            raw = chunk[used: used + aligned]
            self._arena[key] = (chunk, used + aligned)
        return raw[:nbytes].view(dtype).view(shape)

    def _const_conv_operand(self):
        """T [Cout / 32, 16, Cin / 8, 32, 8] = conv1's weight applied to the learned constant (csrc/constconv.hip): a function of the checkpoint,
        rebuilt when either parameter changes."""
        w, c = self.conv1.conv.weight, self.input.input
        key = (w.data_ptr(), w._version, c.data_ptr(), c._version, str(w.device))
        cached = self.__dict__.get("_const_T")
        if cached is None or cached[0] != key:
            cout, cin = self.conv1.conv.out_channel, self.conv1.conv.in_channel
            T = th.empty(cout * 16 * cin, dtype=th.float32, device=w.device)
            with th.cuda.device(w.device):
                _lib.check(_lib.load().maua_pack_const_conv_f32(_lib.require_cuda(w.detach(), "weight").data_ptr(),
                                                                _lib.require_cuda(c.detach(), "input").data_ptr(), T.data_ptr(), cout, cin, 4, 4,
                                                                _lib.stream_ptr(w.device)), "maua_pack_const_conv_f32")
            self.__dict__["_const_T"] = cached = (key, T)
        return cached[1]

    def _style_layers(self):
        """(module ModulatedConv2d, latent index) in forward order: conv1, to_rgb1, then per resolution
        conv_up, conv, to_rgb with latent indices i, i+1, i+2 (reference :549-569)."""
        seq = [(self.conv1.conv, 0), (self.to_rgb1.conv, 1)]
        i = 1
        for n in range(self.log_size - 2):
            seq += [(self.convs[2 * n].conv, i), (self.convs[2 * n + 1].conv, i + 1), (self.to_rgbs[n].conv, i + 2)]
            i += 2
        return seq

    def _table(self, batch):
        seq = self._style_layers()
        key = (batch,) + tuple((m.weight.data_ptr(), m.weight._version, m.modulation.weight.data_ptr()) for m, _ in seq)
        cached = self._tables.get(batch)
        if cached is not None and cached["key"] == key:
            return cached
        entries, s_off, d_off = [], 0, 0
        for m, lat_idx in seq:
            entries.append(m.table_entry(lat_idx, s_off, d_off))
            s_off += m.in_channel
            d_off += batch * m.out_channel if m.demodulate else 0
        info = dict(key=key, table=_style_table(entries, self.input.input.device), entries=entries, s_total=s_off,
                    d_total=max(d_off, 1), max_cin=max(e["cin"] for e in entries),
                    max_cout=max(e["cout"] for e in entries))
        self._tables[batch] = info
        return info

    # ------------------------------------------------------------------ forward
    def forward(self, styles, return_latents=False, return_activation_maps=False, inject_index=None, truncation=1.0,
                truncation_latent=None, input_is_latent=False, noise=None, randomize_noise=True, transform_dict_list=[],
                map_latents=False):
        dev = self.input.input.device
        if dev.type != "cuda":
            raise RuntimeError("Generator must live on a HIP device (.cuda()); the MI355X path has no CPU fallback")
        if map_latents:
            # evident intent of the reference branch (:506-509), whose literal code normalises over a singleton dim
            # (SURVEY.md §8a quirks): map z [N,512] through the mapping network and repeat to n_latent.
            return self.style(styles)[:, None, :].repeat(1, self.n_latent, 1)
        if not input_is_latent:
            styles = [self.style(s) for s in styles]
            if len(styles) < 2:
                inject_index = self.n_latent
                latent = styles[0].unsqueeze(1).repeat(1, inject_index, 1) if styles[0].ndim < 3 else styles[0]
            else:
                if inject_index is None:
                    import random
                    inject_index = random.randint(1, self.n_latent - 1)
                latent = th.cat([styles[0].unsqueeze(1).repeat(1, inject_index, 1),
                                 styles[1].unsqueeze(1).repeat(1, self.n_latent - inject_index, 1)], 1)
        else:
            latent = styles
            if latent.dim() == 2:
                latent = latent[:, None, :].repeat(1, self.n_latent, 1)
        latent = _lib.require_cuda(latent.to(dev), "styles")
        batch = latent.shape[0]
        # the reference only indexes latent[:, i] for i < n_latent (:549-569): surplus rows — an 18-layer latent file fed to a
        # 256-px generator — are legal and ignored; the kernels take the row count as a stride
        if latent.dim() != 3 or latent.shape[1] < self.n_latent or latent.shape[2] != self.style_dim:
            raise RuntimeError(f"styles {tuple(latent.shape)} do not match [batch, >= {self.n_latent}, {self.style_dim}]")
        latent = latent.contiguous()

        noise = list(noise) if noise is not None else [None] * self.num_layers
        for ns in range(self.num_layers):
            if noise[ns] is None and not randomize_noise:
                noise[ns] = getattr(self.noises, f"noise_{ns}")
        # truncation (:537-543).  A float 1.0 is an exact identity and skips the lazy random mean_latent.
        trunc = None
        if not (isinstance(truncation, float) and truncation == 1.0 and truncation_latent is None
                and self.truncation_latent is None):
            if isinstance(truncation, float):
                truncation = th.full((1,), truncation, device=dev)
            if self.truncation_latent is None:
                self.truncation_latent = truncation_latent if truncation_latent is not None else self.mean_latent(2 ** 14)
            trunc = _lib.require_cuda(truncation.to(dev).float().reshape(-1), "truncation")
            if trunc.numel() == 1 and batch > 1:
                trunc = trunc.expand(batch).contiguous()
            if trunc.numel() != batch:
                raise RuntimeError(f"truncation has {trunc.numel()} entries for a batch of {batch}")
        tl = _lib.require_cuda(self.truncation_latent.to(dev).reshape(-1), "truncation_latent") if trunc is not None else None

        with th.cuda.device(dev):
            image, acts, lat_out = self._forward_device(latent, noise, trunc, tl, transform_dict_list,
                                                        return_activation_maps, return_latents)
        # the device forward writes into static per-(batch, layer, lane) buffers that the next call overwrites; the public
        # call hands out private copies, like the reference's freshly allocated outputs (render / hipGraph replay read the
        # static buffers directly and never pass through here)
        image = image.clone() if image is not None else None  # None: min_rgb_size above the output size (reference :553-568)
        if return_activation_maps:
            return image, [a.clone() for a in acts]
        if return_latents:
            return image, lat_out
        return image, None

    def _forward_device(self, latent, noise, trunc, tl, bends, want_acts=False, want_latents=False, frames_u8=None, src=None,
                        batch=None):
        """``frames_u8`` ([B, H, W, 3] uint8): the frame epilogue of render.py:40-43 (clamp, scale, NHWC, uint8) is folded into
        the last layer's fused ToRGB epilogue — the fp32 image of the last resolution is then never written (``image`` returned
        is None) — or, when that layer cannot take the fused path, applied by maua_frames_to_u8 right behind it.
        ``src`` (device pointer of a maua_frame_source_t) + ``batch``: latents, truncation and every noise map are read through
        the frame source (``latent`` / ``noise`` / ``trunc`` are ignored); this is the form ``capture_graph`` records."""
        lib = _lib.load()
        dev = self.input.input.device
        if src is None:
            batch = latent.shape[0]
        st = _lib.stream_ptr(dev)
        info = self._table(batch)
        bufs = lambda name, shape: self._buf(batch, name, shape)  # noqa: E731
        s = bufs("styles", (batch, info["s_total"]))
        d = bufs("demod", (info["d_total"],))
        lat_rows = self.n_latent if latent is None else latent.shape[1]  # row stride of the latents (surplus rows are skipped)
        _lib.check(lib.maua_style_affine_f32(_lib.ptr(latent), batch, lat_rows, self.style_dim, _lib.ptr(trunc),
                                             _lib.ptr(tl), info["table"].data_ptr(), len(info["entries"]),
                                             info["max_cin"], s.data_ptr(), info["s_total"], src, st), "maua_style_affine_f32")
        _lib.check(lib.maua_demod_f32(info["table"].data_ptr(), len(info["entries"]), info["max_cout"], s.data_ptr(),
                                      info["s_total"], d.data_ptr(), batch, st), "maua_demod_f32")
        ent = info["entries"]

        def demod_of(e):
            if e["wsq"] is None:
                return None
            return d[e["d_off"]: e["d_off"] + batch * e["cout"]].view(batch, e["cout"])

        def noise_for(i, h, w):
            if src is not None:
                # slot i of the frame source.  It is bound to maps of the shape of the generator's noise buffer (FrameSource.bind) and no
                # kernel looks at that shape again: a bend that reshapes the maps of a generator built for another output size would read
                # the slots, and write the frames, out of bounds where the eager path raises (_checked_noise)
                hw = tuple(getattr(self.noises, f"noise_{i}").shape[-2:])
                if hw != (int(h), int(w)):
                    raise RuntimeError(f"noise slot {i} holds {hw[0]} x {hw[1]} maps (the generator's noise buffers), the layer's map is "
                                       f"{int(h)} x {int(w)}: build the generator with the output_size its bends produce")
                return None
            nz = noise[i]
            if nz is None:  # randomize_noise=True: fresh N(0,1) per call (:262-265)
                nz = bufs(f"rand_noise_{i}", (batch, 1, h, w)).normal_()
            return nz.to(dev)

        # the style fold (include/maua_hip.h): a layer's epilogue multiplies the map it stores by the NEXT convolution's styles, which then
        # runs without the multiplies in its K loop.  Only where nothing else reads the map: no bend on the producer's layer id, no
        # activation maps handed out (the ToRGB of a plain layer is computed in its own epilogue from the un-scaled value).
        fold = self.style_fold and not want_acts

        def bent(layer_id):
            return any(bd["layer"] == layer_id for bd in bends)

        def post_for(layer_id, consumer, h, w, consumer_entry):
            """s offset of ``consumer``'s styles if the producer with ``layer_id`` may store its map pre-multiplied by them, else None."""
            if not fold or bent(layer_id) or not consumer.accepts_prescaled(h, w):
                return None
            return consumer_entry["s_off"]

        acts = []
        # conv1 on a ConstantInput nobody bends: y = T s with T = W * const precomputed (csrc/constconv.hip) — no [B, C, 4, 4] copy of the
        # constant, no convolution
        c1 = self.conv1.conv
        const_conv = (isinstance(self.input, ConstantInput) and self.conv1.lowres_fusion and not bent(0)
                      and tuple(self.input.input.shape[2:]) == (4, 4) and c1.kernel_size == 3 and not c1.upsample
                      and lib.maua_const_conv_ok(c1.in_channel, c1.out_channel, 4, 4))
        x = None
        if isinstance(self.input, LatentInput):
            x = self.input.run(latent, trunc, tl, bufs("const", (batch, self.input.channel, self.input.size, self.input.size)),
                               src=src, n_latent=self.n_latent, style_dim=self.style_dim)
        elif not const_conv:
            x = bufs("const", (batch,) + tuple(self.input.input.shape[1:]))
            x.copy_(self.input.input.expand(batch, -1, -1, -1))
        if x is not None:
            x = self.const_manipulation.run(x, bends, bufs, "const", src)
        # min_rgb_size (reference :553,567): resolutions below it contribute no ToRGB, the skip chain starts later
        current_size = 4
        image = None
        posted = False  # whether `out` carries the next convolution's styles already
        u8_written = False  # whether the last layer's epilogue wrote ``frames_u8``

        def plain_layer(conv, tag, slot, layer_id, x, e, to_rgb, e_rgb, rgb_name, is_last=False, post_off=None):
            """conv1 (``x`` None: on the constant input) or the plain layer of a resolution, its bends, and the resolution's ToRGB onto
            ``image``: offered to the layer's own launches, else a pass of its own.  Returns the layer's map."""
            nonlocal image, posted, u8_written
            h, w = (4, 4) if x is None else x.shape[2:]
            if is_last and frames_u8 is not None and tuple(frames_u8.shape) != (batch, h, w, 3):
                raise RuntimeError(f"frames buffer {tuple(frames_u8.shape)} for frames [{batch}, {h}, {w}, 3]")
            rgb_buf = bufs(rgb_name, (batch, 3, h, w))
            wants_rgb = self.min_rgb_size <= current_size
            # fold ToRGB into the conv epilogue where the layer qualifies (<= 64 channels) and nothing needs the feature
            # map in between (a bend on this layer id would); the last layer then never writes its feature map at all
            fuse = None
            if wants_rgb and not bent(layer_id) and not self.disable_rgb_fusion:
                fuse = dict(module=to_rgb, s_off=e_rgb["s_off"], skip=image, out=rgb_buf,
                            store=(not is_last) or want_acts, u8=frames_u8 if is_last else None, tap=self.tap_float_image)
            if x is None:
                out = self._run_const_conv(s, e["s_off"], demod_of(e), noise_for(slot, h, w), bufs, fuse, src, batch)
            else:
                out = conv.run(x, s, e["s_off"], demod_of(e), noise_for(slot, h, w), bufs, tag, rgb=fuse, src=src, slot=slot,
                               prescaled=posted, post_off=post_off)
            posted = conv.posted
            out = conv.manipulation.run(out, bends, bufs, tag, src)
            acts.append(out)
            if fuse is not None and fuse.get("done"):
                image = rgb_buf
                if is_last and frames_u8 is not None and fuse.get("u8_done", True):
                    u8_written = True  # left the device path as uint8 frames
                    if not self.tap_float_image:
                        image = None
            elif wants_rgb:
                assert not posted  # (a separate ToRGB pass reads the un-scaled map: plain.run only posts from the ToRGB-fused paths)
                image = to_rgb.run(out, s, e_rgb["s_off"], image, rgb_buf)
            return out

        # (conv1 never posts: its consumer is a polyphase layer without a pre-scaled instance)
        out = plain_layer(self.conv1, "conv1", 0, 1, x, ent[0], self.to_rgb1, ent[1], "rgb1")
        for n in range(self.log_size - 2):
            up, plain = self.convs[2 * n], self.convs[2 * n + 1]
            is_last = n == self.log_size - 3
            # this resolution's entries of the style table (conv1 and to_rgb1 come first); e_next: the next resolution's up-sampling layer
            e_up, e_plain, e_rgb = ent[3 * n + 2: 3 * n + 5]
            e_next = None if is_last else ent[3 * n + 5]
            h, w = out.shape[2] * 2, out.shape[3] * 2
            out = up.run(out, s, e_up["s_off"], demod_of(e_up), noise_for(2 * n + 1, h, w), bufs, f"convs.{2 * n}", src=src,
                         slot=2 * n + 1, prescaled=posted, post_off=post_for(2 * n + 2, plain, h, w, e_plain))
            posted = up.posted
            out = up.manipulation.run(out, bends, bufs, f"convs.{2 * n}", src)
            acts.append(out)
            current_size *= 2
            post_off = None if is_last else post_for(2 * n + 3, self.convs[2 * n + 2], h, w, e_next)
            out = plain_layer(plain, f"convs.{2 * n + 1}", 2 * n + 2, 2 * n + 3, out, e_plain, self.to_rgbs[n], e_rgb, f"rgbs.{n}",
                              is_last, post_off)
        # last layer not fusable (bend on it, > 64 channels, ...).  (Not behind an epilogue that wrote the frames: with tap_float_image the
        # fp32 image exists as well, and converting it here would replace the frames the parity tests mean to look at.)
        if frames_u8 is not None and image is not None and not u8_written:
            _lib.check(lib.maua_frames_to_u8(image.data_ptr(), frames_u8.data_ptr(), batch, image.shape[2], image.shape[3], st),
                       "maua_frames_to_u8")
        lat_out = None
        if want_latents:
            lat_out = latent if trunc is None else tl[None, None, :] + trunc[:, None, None] * (latent - tl[None, None, :])
        return image, acts, lat_out

    def _run_const_conv(self, s, s_off, d, noise, bufs, rgb, src, batch):
        """conv1 + noise + bias + activation (+ the partial ToRGB sums of to_rgb1 and their plane sum) on the constant input: one launch of
        maua_const_styledconv_f32 (+ one of maua_torgb_f32's plane-sum form).  One more path of ``StyledConv.run``, reported on conv1."""
        m, c1 = self.conv1, self.conv1.conv
        cin, cout = c1.in_channel, c1.out_channel
        out = bufs("conv1", (batch, cout, 4, 4))
        noise, nstride = _checked_noise(noise, batch, 4, 4, src)
        part = None if rgb is None else bufs("conv1.rgb_partial", (batch, 3 * (cout // 32), 4, 4))
        _lib.check(_lib.load().maua_const_styledconv_f32(
            self._const_conv_operand().data_ptr(), s.data_ptr() + 4 * s_off, s.shape[1], _lib.ptr(d), out.data_ptr(), _lib.ptr(noise), nstride,
            m.noise.weight.data_ptr(), m.activate.bias.data_ptr(), *m._rgb_operands(rgb, s), _lib.ptr(part), src, 0, batch,
            cin, cout, 4, 4, float(c1.scale), _lib.stream_ptr(self.input.input.device)), "maua_const_styledconv_f32")
        if rgb is not None:
            rgb["module"].run(part, None, 0, None, rgb["out"])
        return m._took("const", out, rgb=rgb)

    # ------------------------------------------------------------------ counter-based noise
    def _randn_table(self, slots, maps):
        """Device table of maua_randn_slot_t (include/maua_hip.h) for ``maps[k]`` = the [batch, 1, h, w] destination of slot ``slots[k]``."""
        host = (_lib.RandnSlot * len(slots))()
        for entry, i, t in zip(host, slots, maps):
            entry.dst, entry.hw, entry.slot = t.data_ptr(), int(t.shape[-2]) * int(t.shape[-1]), int(i)
        return th.frombuffer(bytearray(bytes(host)), dtype=th.uint8).to(self.input.input.device)

    def _noise_slots(self, slots):
        slots = list(range(self.num_layers)) if slots is None else [int(i) for i in slots]
        if not slots or len(set(slots)) != len(slots) or min(slots) < 0 or max(slots) >= min(self.num_layers, _lib.MAX_NOISE_SLOTS):
            raise RuntimeError(f"noise slots {slots} are not distinct indices below {min(self.num_layers, _lib.MAX_NOISE_SLOTS)}")
        return slots

    def random_noise(self, frame0, batch, seed, slots=None):
        """Seeded N(0,1) noise maps of frames [frame0, frame0 + batch) for ``slots`` (default: every noise layer): a list of
        [batch, 1, h, w] device tensors, one launch of maua_randn_frames_f32.  The map of (seed, frame, slot) is a pure function
        (Philox4x32-10 + Box-Muller, include/maua_hip.h): the same whatever batch it is produced in, and the same a captured forward
        with ``random_slots`` generates for itself."""
        dev = self.input.input.device
        if dev.type != "cuda":
            raise RuntimeError("Generator must live on a HIP device (.cuda()); the MI355X path has no CPU fallback")
        slots = self._noise_slots(slots)
        frame0, batch, seed = int(frame0), int(batch), int(seed)
        if frame0 < 0 or batch < 1 or frame0 + batch > 2 ** 31 or not 0 <= seed < 2 ** 64:
            raise RuntimeError(f"random_noise: frames [{frame0}, {frame0 + batch}) / seed {seed} out of range")
        with th.cuda.device(dev):
            maps = [th.empty((batch, 1) + tuple(getattr(self.noises, f"noise_{i}").shape[-2:]), dtype=th.float32, device=dev) for i in slots]
            table = self._randn_table(slots, maps)
            _lib.check(_lib.load().maua_randn_frames_f32(table.data_ptr(), len(slots), batch, seed, frame0, None, _lib.stream_ptr(dev)),
                       "maua_randn_frames_f32")
            table.record_stream(th.cuda.current_stream(dev))
        return maps

    # ------------------------------------------------------------------ hipGraph
    def weights_key(self):
        """Identity of everything a captured graph has baked in as pointers: parameters and buffers (a swapped or in-place
        modified tensor invalidates the packed weights, style tables and therefore the graph)."""
        return tuple((t.data_ptr(), t._version) for t in list(self.parameters()) + list(self.buffers()))

    def capture_graph(self, batch, lane=0, frames_u8=False, bends=(), random_slots=(), noise_seed=0, noise_frame_offset=0, synth_slots=(),
                      synth_frame_offset=0):
        """Capture one forward of ``batch`` frames into a hipGraph and return its ``GraphLane``.  The captured kernels read
        their per-frame inputs (latents, truncation, noise maps, bend parameters) THROUGH a frame source in device memory
        (include/maua_hip.h): ``lane.bind(latents, noise, truncation)`` points it at sequences resident in HBM — any render,
        any mix of per-frame maps and checkpoint noise buffers — and ``lane.replay(frame0)`` moves only the frame index, so a
        graph is captured once per (batch, lane, bend set) and outlives the render (the reference re-uploads every slice per
        batch, render.py:140-149).  ``bends``: [{"layer", "transform"}] whose transforms implement ``run_static`` (audioreactive
        /bend.py).  Lanes share the weights but no activation buffer: they may be replayed concurrently on different streams.
        ``random_slots``: noise slots whose maps the captured forward GENERATES per replay (``randomize_noise``): it then starts with one
        maua_randn_frames_f32 launch that fills lane-private [batch, 1, h, w] buffers with the maps of (``noise_seed``, frame
        ``noise_frame_offset`` + frame0 + b, slot) — what ``random_noise`` returns for those frames — and points the frame source at them;
        ``bind`` takes None for these slots.  Seed and offset are kernel arguments: part of the graph.
        ``synth_slots``: noise slots whose maps the captured forward SYNTHESISES per replay from a recipe (audioreactive/noise.py NoiseSynth):
        one maua_noise_synth_f32 launch, behind the maua_randn_frames_f32 one, fills lane-private [batch, 1, h, w] buffers from a lane-private
        table in device memory and points the frame source at them; ``bind`` takes a NoiseSynth for exactly these slots and writes the table,
        so another render's recipes need no new capture.  Only ``synth_frame_offset`` (the recipes' frame offset: 0, or a shard's first frame)
        is a kernel argument.  The two slot sets are disjoint."""
        dev = self.input.input.device
        if th.cuda.current_stream(dev).cuda_stream == 0:
            raise RuntimeError("capture_graph must run on a non-default stream (with torch.cuda.stream(s): ...): HIP cannot "
                               "capture the legacy default stream")
        bends = list(bends)
        for bd in bends:
            if not hasattr(bd["transform"], "run_static"):
                raise RuntimeError(f"bend on layer {bd['layer']} is not capturable: {type(bd['transform']).__name__} has no run_static")
        self._lane = lane
        self._captured = True
        try:
            with th.cuda.device(dev):
                random_slots = tuple(self._noise_slots(random_slots)) if len(random_slots) else ()
                generated = {i: self._buf(batch, f"g.randn_{i}", (batch, 1) + tuple(getattr(self.noises, f"noise_{i}").shape[-2:]))
                             for i in random_slots}
                synth_slots = tuple(self._noise_slots(synth_slots)) if len(synth_slots) else ()
                if set(synth_slots) & set(random_slots):
                    raise RuntimeError(f"noise slots {sorted(set(synth_slots) & set(random_slots))} are both random_slots and synth_slots")
                if not 0 <= int(synth_frame_offset) < 2 ** 31:
                    raise RuntimeError(f"synth_frame_offset {synth_frame_offset} out of range")
                synthesised = {i: self._buf(batch, f"g.synth_{i}", (batch, 1) + tuple(getattr(self.noises, f"noise_{i}").shape[-2:]))
                               for i in synth_slots}
                synth_table = None
                if synth_slots:  # all zero = every entry empty: the launch is a no-op until ``bind`` has written the recipes
                    synth_table = self._buf(batch, "g.synth_table", (len(synth_slots) * ctypes.sizeof(_lib.NoiseSynthSlot),), dtype=th.uint8)
                    synth_table.zero_()
                source = FrameSource(self, batch, lane, generated, synthesised, synth_table, int(synth_frame_offset))
                randn_table = self._randn_table(random_slots, [generated[i] for i in random_slots]) if random_slots else None
                u8 = None
                if frames_u8:
                    hw = getattr(self.noises, f"noise_{self.num_layers - 1}").shape[-2:]
                    u8 = self._buf(batch, "g.frames_u8", (batch, int(hw[0]), int(hw[1]), 3), dtype=th.uint8)
                tl = self._buf(0, "g.trunc_latent", (self.style_dim,))

                def run():
                    if randn_table is not None:  # first launch of the forward: the layers below read the maps through the frame source
                        _lib.check(_lib.load().maua_randn_frames_f32(randn_table.data_ptr(), len(random_slots), batch, int(noise_seed),
                                                                     int(noise_frame_offset), source.ptr, _lib.stream_ptr(dev)),
                                   "maua_randn_frames_f32")
                    if synth_table is not None:  # the table is read on every replay: whatever ``bind`` wrote last
                        _lib.check(_lib.load().maua_noise_synth_f32(synth_table.data_ptr(), len(synth_slots), batch, int(synth_frame_offset),
                                                                    source.ptr, _lib.stream_ptr(dev)), "maua_noise_synth_f32")
                    return self._forward_device(None, None, None, tl, bends, frames_u8=u8, src=source.ptr, batch=batch)

                run()  # warm-up: allocates every static buffer, packs the weights
                th.cuda.synchronize(dev)
                graph = _lib.HipGraph()
                with graph:
                    image, _, _ = run()
            lane_ = GraphLane(self, graph, source, image, u8, tl, batch, lane, self.weights_key())
            lane_.random_slots, lane_.noise_seed, lane_.noise_frame_offset = random_slots, int(noise_seed), int(noise_frame_offset)
            lane_._randn_table = randn_table  # the captured launch reads it on every replay
            lane_.synth_slots, lane_.synth_frame_offset = synth_slots, int(synth_frame_offset)
            return lane_
        finally:
            self._lane = 0


class FrameSource:
    """Host handle of a maua_frame_source_t in device memory (include/maua_hip.h): the pointers of the HBM-resident per-frame
    sequences a captured forward reads, plus the frame it starts at."""

    def __init__(self, generator, batch, lane, generated=None, synthesised=None, synth_table=None, synth_frame_offset=0):
        self.generator = generator
        self.batch = batch
        # slot -> lane-private [batch, 1, h, w] buffer the captured forward fills itself (capture_graph's random_slots); its first launch
        # rewrites the slot's pointer / stride on every replay, so what ``bind`` leaves there is never read: one valid map, stride 0
        self.generated = dict(generated or {})
        # slot -> lane-private buffer the captured forward synthesises from the recipe ``bind`` wrote into ``synth_table`` (capture_graph's
        # synth_slots; one maua_noise_synth_slot_t per slot, in slot order); the launch rewrites pointer and stride like the random one
        self.synthesised = dict(synthesised or {})
        self.synth_table, self.synth_frame_offset = synth_table, int(synth_frame_offset)
        self.dev = generator._buf(batch, "g.frame_source", (ctypes.sizeof(_lib.FrameSource),), dtype=th.uint8)
        self.ptr = self.dev.data_ptr()
        self._keep = None
        # until bound: zero latents of one batch, the checkpoint's noise buffers (stride 0), no truncation
        zeros = generator._buf(batch, "g.latents0", (batch, generator.n_latent, generator.style_dim))
        zeros.zero_()
        self.noise_hw = [tuple(getattr(generator.noises, f"noise_{i}").shape[-2:]) for i in range(generator.num_layers)]
        self.bind(zeros, [None] * generator.num_layers, None, _n_frames=batch)

    def bind(self, latents, noise, trunc, _n_frames=None):
        """latents [n_frames, n_latent, style_dim]; noise: per slot None (the checkpoint's buffer for every frame), a
        [n_frames, 1, h, w] sequence or one shared [1, 1, h, w] map — or, for exactly the lane's synth slots, a NoiseSynth recipe;
        trunc [n_frames] or None — all fp32, on the device, contiguous; they are kept alive by this handle until ``release``."""
        from ..audioreactive.noise import NoiseSynth

        g = self.generator
        dev = g.input.input.device
        n_frames = latents.shape[0] if _n_frames is None else _n_frames
        host = _lib.FrameSource()
        latents = _lib.require_cuda(latents, "latents")
        if latents.dim() != 3 or latents.shape[1] < g.n_latent or latents.shape[2] != g.style_dim:
            raise RuntimeError(f"latents {tuple(latents.shape)} do not match [n_frames, >= {g.n_latent}, {g.style_dim}]")
        if latents.shape[1] != g.n_latent or not latents.is_contiguous():
            # surplus rows (the reference only indexes latent[:, i], i < n_latent): the captured kernels have the row stride
            # n_latent baked in, so the sequence is cut once per render
            latents = latents[:, :g.n_latent].contiguous()
        host.latents = latents.data_ptr()
        keep = [latents]
        if trunc is not None:
            trunc = _lib.require_cuda(trunc, "truncation").reshape(-1)
            if trunc.numel() != n_frames:
                raise RuntimeError(f"truncation has {trunc.numel()} entries for {n_frames} frames")
            host.trunc = trunc.data_ptr()
            keep.append(trunc)
        if len(noise) != g.num_layers or g.num_layers > _lib.MAX_NOISE_SLOTS:
            raise RuntimeError(f"{len(noise)} noise entries for {g.num_layers} layers")
        synth_host = (_lib.NoiseSynthSlot * max(len(self.synthesised), 1))()  # zero = empty entries (the unbound lane)
        for i, nz in enumerate(noise):
            if i in self.synthesised:
                if isinstance(nz, NoiseSynth):
                    if (nz.height, nz.width) != self.noise_hw[i]:
                        raise RuntimeError(f"noise[{i}]: the recipe makes {nz.height} x {nz.width} maps, the layer takes "
                                           f"{self.noise_hw[i][0]} x {self.noise_hw[i][1]}")
                    if nz.n_frames is not None and nz.n_frames != n_frames:
                        raise RuntimeError(f"noise[{i}]: the recipe's envelopes cover {nz.n_frames} frames, the render has {n_frames}")
                    if nz.offset != self.synth_frame_offset:
                        raise RuntimeError(f"noise[{i}]: the recipe starts at frame {nz.offset}, this lane was captured for frame offset "
                                           f"{self.synth_frame_offset}")
                    if nz.device != dev:
                        raise RuntimeError(f"noise[{i}]: the recipe lives on {nz.device}, the generator on {dev}")
                    synth_host[sorted(self.synthesised).index(i)] = nz.table_entry(self.synthesised[i].data_ptr(), i)
                    keep.append(nz)
                elif nz is not None or _n_frames is None:
                    raise RuntimeError(f"noise[{i}] is synthesised by this lane (synth_slots): bind a NoiseSynth, not "
                                       f"{'None' if nz is None else 'a tensor'}")
                host.noise[i] = self.synthesised[i].data_ptr()
                host.noise_stride[i] = 0
                continue
            if isinstance(nz, NoiseSynth):
                raise RuntimeError(f"noise[{i}] is a NoiseSynth, but this lane was not captured with slot {i} among its synth_slots")
            if i in self.generated:
                if nz is not None:
                    raise RuntimeError(f"noise[{i}] is generated by this lane (random_slots): bind it as None")
                host.noise[i] = self.generated[i].data_ptr()
                host.noise_stride[i] = 0
                continue
            if nz is None:
                nz = getattr(g.noises, f"noise_{i}")
            nz = _lib.require_cuda(nz.to(dev), f"noise[{i}]")
            if nz.dim() != 4 or nz.shape[1] != 1 or tuple(nz.shape[-2:]) != self.noise_hw[i] or nz.shape[0] not in (1, n_frames):
                raise RuntimeError(f"noise[{i}] {tuple(nz.shape)} does not match [{n_frames} or 1, 1, {self.noise_hw[i][0]}, "
                                   f"{self.noise_hw[i][1]}]")
            host.noise[i] = nz.data_ptr()
            host.noise_stride[i] = _noise_stride(nz)
            keep.append(nz)
        self.n_frames = n_frames
        self._keep = keep
        raw = th.frombuffer(bytearray(bytes(host)), dtype=th.uint8)
        th.cuda.synchronize(dev)  # no replay of this lane may still be reading the previous pointers (bind is once per render)
        self.dev.copy_(raw.to(dev), non_blocking=False)
        if self.synth_table is not None:  # the recipes of this render, under the same two synchronisations as the pointers
            self.synth_table.copy_(th.frombuffer(bytearray(bytes(synth_host)), dtype=th.uint8).to(dev), non_blocking=False)
        th.cuda.synchronize(dev)

    def release(self):
        """Drop the references to the bound sequences (the end of a render): a replay before the next ``bind`` raises instead of
        reading memory the allocator may have handed out again."""
        self._keep = None
        self.n_frames = 0

    def seek(self, frame0, stream=None):
        if frame0 < 0 or frame0 + self.batch > self.n_frames:
            raise RuntimeError(f"frames [{frame0}, {frame0 + self.batch}) are outside the bound sequences ({self.n_frames} frames)")
        _lib.check(_lib.load().maua_frame_source_seek(self.ptr, int(frame0), stream if stream is not None else _lib.stream_ptr()),
                   "maua_frame_source_seek")


class GraphLane:
    """One captured forward of a Generator: hipGraph + the frame source it reads + its output buffers."""

    def __init__(self, generator, graph, source, image, u8, trunc_latent, batch, lane, weights_key):
        self.generator, self.graph, self.source = generator, graph, source
        self.image, self.u8, self.batch, self.lane = image, u8, batch, lane
        self._trunc_latent = trunc_latent
        self.weights_key = weights_key
        self.random_slots, self.noise_seed, self.noise_frame_offset = (), 0, 0
        self.synth_slots, self.synth_frame_offset = (), 0

    def bind(self, latents, noise, truncation=None):
        """Point the lane at the sequences of a render (see FrameSource.bind).  ``truncation`` [n_frames] switches the
        truncation lerp on; its centre is the generator's truncation latent (drawn lazily as in the reference :539-540)."""
        g = self.generator
        if truncation is not None:
            if g.truncation_latent is None:
                g.truncation_latent = g.mean_latent(2 ** 14)
            self._trunc_latent.copy_(g.truncation_latent.to(self._trunc_latent.device).reshape(-1))
        self.source.bind(latents, noise, truncation)

    def release(self):
        self.source.release()

    def replay(self, frame0, stream=None):
        """Frames [frame0, frame0 + batch) of the bound sequences: one 4-byte device write + the graph launch."""
        self.source.seek(frame0, stream)
        self.graph.replay(stream)
