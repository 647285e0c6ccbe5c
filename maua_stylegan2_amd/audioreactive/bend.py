"""Network bending with the reference's ``audioreactive.bend`` surface, on one HIP warp kernel instead of kornia.

Mirrors /root/reference/audioreactive/bend.py: NetworkBend :12-26 · AddNoise :29-41 · Print :44-49 · Translate :52-72 ·
Zoom :75-87 · Rotate :90-102 (and, without a counterpart there, the point / morphological bends, the
padding bend and the coordinate-remap bends Mirror, Kaleidoscope, Swirl, Ripple, Displace).  The reference composes ReflectionPad2d -> kornia Translate/Scale/Rotate -> kornia
CenterCrop (three full-size intermediates); here the composition is evaluated per OUTPUT pixel by
maua_affine_reflect_warp_f32: inverse affine map into the padded canvas, bilinear taps, reflection folded into the
index.  kornia is an un-pinned, un-vendored dependency (requirements.txt:8) -> "parity unpinned" (DESIGN.md); the
conventions implemented are kornia's documented ones: pixel-unit translation, transforms about the canvas centre
((W-1)/2, (H-1)/2), bilinear, zeros outside the canvas, anticlockwise-positive angles in degrees.
"""
import math

import torch as th

from .. import _lib


class NetworkBend(th.nn.Module):
    """reference :12-26.  ``modulation`` is the batch slice in the reference's render loop (render.py:151-158); the MI355X
    render loop hands over the modulation of the WHOLE sequence once and a captured forward picks the frame's row on the
    device (``run_static``), which is what makes bends hipGraph-capturable."""

    def __init__(self, sequential_fn, modulation):
        super().__init__()
        self.sequential = sequential_fn(modulation)

    def forward(self, x):
        return self.sequential(x)

    def run_static(self, x, out, src):
        if not hasattr(self.sequential, "run_static"):
            raise RuntimeError(f"{type(self.sequential).__name__} cannot run inside a captured forward")
        return self.sequential.run_static(x, out, src)

    @property
    def capturable(self):
        return hasattr(self.sequential, "run_static")

    @property
    def sequence_rows(self):
        """Rows of per-frame parameters the captured form indexes with frame0 + b (None: nothing per-frame); the render loop
        requires 1 or the number of frames of the sequence before it captures (a shorter table would be read out of bounds)."""
        return getattr(self.sequential, "sequence_rows", None)


class AddNoise(th.nn.Module):
    def __init__(self, noise):
        super().__init__()
        self.noise = noise

    def forward(self, x):
        return x + self.noise.to(x.device)

    def run_static(self, x, out, src):
        """Capturable form: writes into the static buffer ``out`` (no allocation; the noise is static for the whole render)."""
        if self.noise.device != x.device or self.noise.dtype != x.dtype:
            self.noise = self.noise.to(x.device, x.dtype)
        return th.add(x, self.noise, out=out)


class Print(th.nn.Module):
    def forward(self, x):
        print(x.shape, [x.min().item(), x.mean().item(), x.max().item()], th.std(x).item())
        return x


def reflection_chain_index(n, pad_pairs):
    """Source index of every element of an axis of length ``n`` after a CHAIN of reflection pads [(before, after), ...]
    applied one after the other, as stacked ``ReflectionPad2d`` modules do: each pad mirrors the canvas built so far, so
    the composition is in general not one triangular fold of the source (reference bend.py:60-64 stacks three)."""
    idx = list(range(n))
    for before, after in pad_pairs:
        if before >= len(idx) or after >= len(idx):
            raise ValueError(f"reflection pad ({before}, {after}) must be smaller than the axis ({len(idx)})")
        idx = idx[before:0:-1] + idx + idx[-2:-2 - after:-1] if before or after else idx
    return idx


class AffineReflectWarp(th.nn.Module):
    """y = CenterCrop(h, w)( Affine( ReflectionPad(x) [+ noise] ) ) with a per-sample inverse map ``m`` [B, 6].
    ``pads`` is one (left, right, top, bottom) tuple or a list of them (pads stacked in that order)."""

    def __init__(self, inv_maps, pads, noise=None):
        super().__init__()
        self.inv_maps = inv_maps
        chain = [tuple(pads)] if isinstance(pads[0], int) else [tuple(p) for p in pads]
        self.chain = chain
        self.pads = tuple(sum(p[i] for p in chain) for i in range(4))  # total (left, right, top, bottom)
        self.noise = noise
        self._maps = None  # (h, w, device) -> int32 index tables, only for a real chain
        self._dev = None   # (device, batch) -> device-resident operands of the launch

    @property
    def sequence_rows(self):
        return int(self.inv_maps.shape[0])

    def _operands(self, x, per_frame):
        """Device-resident operands, built on the first call for a (device, batch) and reused (so that a captured forward
        performs no allocation): inverse maps (the whole sequence when ``per_frame``, else expanded to the batch), the canvas
        noise plane, the reflection-chain index tables."""
        b, c, h, w = x.shape
        key = (str(x.device), b, per_frame, h, w)
        if self._dev is None or self._dev[0] != key:
            m = self.inv_maps.to(x.device, th.float32).contiguous()
            if not per_frame:
                if m.shape[0] == 1 and b > 1:
                    m = m.expand(b, 6).contiguous()
                if m.shape != (b, 6):
                    raise RuntimeError(f"expected {b} inverse affine maps, got {tuple(m.shape)}")
            nz = None
            if self.noise is not None:
                nz = _lib.require_cuda(self.noise.to(x.device).float(), "noise")
                pl, pr, pt, pb = self.pads
                if nz.numel() != (h + pt + pb) * (w + pl + pr):
                    raise RuntimeError("bend noise must have the size of one padded canvas plane")
            xmap = ymap = None
            if len(self.chain) > 1:
                xs = reflection_chain_index(w, [(p[0], p[1]) for p in self.chain])
                ys = reflection_chain_index(h, [(p[2], p[3]) for p in self.chain])
                xmap, ymap = th.tensor(xs, dtype=th.int32, device=x.device), th.tensor(ys, dtype=th.int32, device=x.device)
            self._dev = (key, m, nz, xmap, ymap)
        return self._dev[1:]

    def _launch(self, x, y, m, nz, xmap, ymap, src):
        b, c, h, w = x.shape
        _lib.call("maua_affine_reflect_warp_mapped_f32", x, m, y, b, c, h, w, *self.pads, nz, xmap, ymap, src)
        return y

    def forward(self, x):
        x = _lib.require_cuda(x, "x")
        m, nz, xmap, ymap = self._operands(x, per_frame=False)
        return self._launch(x, th.empty_like(x), m, nz, xmap, ymap, None)

    def run_static(self, x, out, src):
        """Inside a captured forward: ``inv_maps`` holds one row per frame of the render (or a single static row) and sample b
        uses row frame0 + b, read on the device through the frame source ``src`` — nothing is rebuilt per batch."""
        per_frame = self.inv_maps.shape[0] != 1
        m, nz, xmap, ymap = self._operands(x, per_frame=per_frame)
        return self._launch(x, out, m, nz, xmap, ymap, src if per_frame else None)


_POINT_OPS = {"ablate": 0, "invert": 1, "multiply": 2, "threshold": 3}  # `op` of maua_bend_point_f32
_MORPH_OPS = {"erode": 0, "dilate": 1}                                   # `op` of maua_bend_morph_f32
_MAX_RADIUS = 16                                                         # MAUA_BEND_MAX_RADIUS


class _ChannelBend(th.nn.Module):
    """What the point and the morphological bends share: a per-frame parameter table of ``rows`` entries (``table`` [rows], or None
    for an op without parameter) and a channel subset, uploaded once per (device, channel count) and reused, so that a captured
    forward allocates nothing."""

    def __init__(self, table, channels, n_channels=None):
        super().__init__()
        self.table = table
        self.channels = None if channels is None else th.as_tensor(channels, dtype=th.int64).reshape(-1).cpu()
        self._dev = {}  # (device, channels of the map) -> table and channel mask on the device; entries are never evicted: a captured
                        # graph keeps reading them, also when one static instance sits on layers of different widths
        if n_channels is not None:
            self._channel_mask(int(n_channels))

    @property
    def sequence_rows(self):
        return 1 if self.table is None else int(self.table.shape[0])

    def _channel_mask(self, c):
        if self.channels is None:
            return None
        if self.channels.numel() and (int(self.channels.min()) < 0 or int(self.channels.max()) >= c):
            raise RuntimeError(f"bend channels must lie in 0 .. {c - 1} (the feature map has {c} channels)")
        mask = th.zeros(c, dtype=th.uint8)
        mask[self.channels] = 1
        return mask

    def _operands(self, x, per_frame):
        """(table, mask) on x's device.  ``per_frame``: the table is the sequence of the whole render, indexed through the frame
        source; otherwise it holds one row, or one row per sample of ``x``."""
        b, c = x.shape[:2]
        if b > 64:
            raise RuntimeError(f"bends serve batches of up to 64 frames (got {b})")
        if not per_frame and self.sequence_rows not in (1, b):
            raise RuntimeError(f"expected 1 or {b} bend parameter rows, got {self.sequence_rows}")
        if c > 65535:
            raise RuntimeError(f"bends serve feature maps of up to 65535 channels (got {c})")
        key = (str(x.device), c)
        if key not in self._dev:
            table = None if self.table is None else self.table.to(x.device).contiguous()
            mask = self._channel_mask(c)
            self._dev[key] = (table, None if mask is None else mask.to(x.device))
        return self._dev[key]

    def forward(self, x):
        x = _lib.require_cuda(x, "x")
        return self._launch(x, th.empty_like(x), *self._operands(x, per_frame=False), None)

    def run_static(self, x, out, src):
        """Inside a captured forward: the table holds one row per frame of the render (or a single static row) and sample b uses
        row frame0 + b, read on the device through the frame source ``src``."""
        per_frame = self.sequence_rows != 1
        return self._launch(x, out, *self._operands(x, per_frame=per_frame), src if per_frame else None)


class PointBend(_ChannelBend):
    """y = op(x, p) on the channels ``channels`` (index list / LongTensor, None = all), the others copied through; ``op`` one of
    _POINT_OPS, ``params`` [rows] (None for ablate / invert).  ``n_channels`` validates the channel list at construction instead of
    at first use."""

    def __init__(self, op, params, channels, n_channels=None):
        if op not in _POINT_OPS:
            raise ValueError(f"unknown point bend {op!r} ({' | '.join(_POINT_OPS)})")
        if params is None and _POINT_OPS[op] >= 2:
            raise ValueError(f"point bend {op!r} needs a parameter")
        if params is not None:
            params = th.as_tensor(params)
            if params.dim() != 1 or params.shape[0] < 1:
                raise ValueError(f"bend modulation must be a [n_frames] sequence (got shape {tuple(params.shape)})")
            params = params.float()
        super().__init__(params, channels, n_channels)
        self.op = _POINT_OPS[op]

    def _launch(self, x, y, params, mask, src):
        b, c = x.shape[:2]
        _lib.call("maua_bend_point_f32", x, y, b, c, x[0, 0].numel(), self.op, params, self.sequence_rows, mask, src)
        return y


class MorphBend(_ChannelBend):
    """Erosion / dilation (``op`` one of _MORPH_OPS) with a (2r + 1)^2 window, r = ``radii`` [rows] (integers in 0 .. _MAX_RADIUS,
    checked here on the host), on the channels ``channels``."""

    def __init__(self, op, radii, channels, n_channels=None):
        if op not in _MORPH_OPS:
            raise ValueError(f"unknown morphological bend {op!r} ({' | '.join(_MORPH_OPS)})")
        radii = th.as_tensor(radii).float()
        if radii.dim() != 1 or radii.shape[0] < 1:
            raise ValueError(f"bend modulation must be a [n_frames] sequence (got shape {tuple(radii.shape)})")
        lo, hi = float(radii.min()), float(radii.max())
        if not (lo >= 0 and hi <= _MAX_RADIUS):  # (also refuses a NaN)
            raise ValueError(f"morphological bend radii must lie in 0 .. {_MAX_RADIUS} (got {lo:g} .. {hi:g})")
        if not bool((radii == th.round(radii)).all()):
            raise ValueError("morphological bend radii must be whole numbers (Erode / Dilate round their modulation)")
        super().__init__(radii.to(th.int32), channels, n_channels)
        self.op = _MORPH_OPS[op]

    def _launch(self, x, y, radii, mask, src):
        b, c, h, w = x.shape
        _lib.call("maua_bend_morph_f32", x, y, b, c, h, w, self.op, radii, self.sequence_rows, mask, src)
        return y


_PAD_MODES = {"constant": 0, "replicate": 1, "reflect": 2, "circular": 3}  # `mode` of maua_bend_pad_f32


class Pad(th.nn.Module):
    """y = torch.nn.functional.pad(x, padding, mode, value) (+ noise) in one launch of maua_bend_pad_f32: the capturable form of the
    examples' layer-0 transform ``Sequential(ReplicationPad2d((2, 2, 0, 0)), AddNoise(noise))`` that widens the 4 x 4 constant for a
    2:1 render.  ``padding`` = (left, right, top, bottom), each >= 0; ``noise``: a static plane of the PADDED size, [H, W], [1 or C, H, W]
    or [1, 1 or C, H, W].  Nothing is per frame.  A static bend that changes the map's shape says so through ``static_shape``: the
    captured forward sizes the output buffer with it (ManipulationLayer.run)."""

    capturable = True
    sequence_rows = None

    def __init__(self, padding, mode="replicate", value=0.0, noise=None):
        super().__init__()
        padding = tuple(padding)
        if len(padding) != 4 or any(int(p) != p for p in padding):
            raise ValueError(f"padding must be four whole numbers (left, right, top, bottom), got {padding}")
        padding = tuple(int(p) for p in padding)
        if min(padding) < 0:
            raise ValueError(f"pads must not be negative (got {padding}): cropping is not a padding bend")
        if mode not in _PAD_MODES:
            raise ValueError(f"unknown padding mode {mode!r} ({' | '.join(_PAD_MODES)})")
        if noise is not None:
            noise = th.as_tensor(noise)
            if noise.dim() not in (2, 3, 4) or (noise.dim() == 4 and noise.shape[0] != 1):
                raise ValueError(f"bend noise must be one static plane [H, W], [C, H, W] or [1, C, H, W] (got shape {tuple(noise.shape)})")
            noise = noise.reshape((-1,) + tuple(noise.shape[-2:])).float()
        self.padding, self.mode, self.value, self.noise = padding, mode, float(value), noise
        self._dev = {}  # device -> the noise plane there; entries are never evicted: a captured graph keeps reading them

    def static_shape(self, shape):
        """Shape of the padded map for an input of ``shape`` [B, C, h, w]; refuses what the kernel refuses."""
        b, c, h, w = (int(v) for v in shape)
        left, right, top, bottom = self.padding
        if self.mode == "reflect" and (max(left, right) >= w or max(top, bottom) >= h):
            raise RuntimeError(f"reflect pads {self.padding} must be smaller than the map ({h} x {w})")
        if self.mode == "circular" and (max(left, right) > w or max(top, bottom) > h):
            raise RuntimeError(f"circular pads {self.padding} must not exceed the map ({h} x {w})")
        return (b, c, h + top + bottom, w + left + right)

    def _noise_plane(self, x, shape):
        if self.noise is None:
            return None
        if tuple(self.noise.shape[1:]) != tuple(shape[2:]) or self.noise.shape[0] not in (1, shape[1]):
            raise RuntimeError(f"bend noise {tuple(self.noise.shape)} does not match the padded map {tuple(shape)}: "
                               f"expected [1 or {shape[1]}, {shape[2]}, {shape[3]}]")
        key = str(x.device)
        if key not in self._dev:
            self._dev[key] = self.noise.to(x.device).contiguous()
        return self._dev[key]

    def _launch(self, x, y):
        b, c, h, w = x.shape
        if b > 64 or c > 65535:
            raise RuntimeError(f"bends serve batches of up to 64 frames and maps of up to 65535 channels (got {b} x {c})")
        nz = self._noise_plane(x, y.shape)
        _lib.call("maua_bend_pad_f32", x, y, b, c, h, w, *self.padding, _PAD_MODES[self.mode], self.value, nz, 0 if nz is None else nz.shape[0])
        return y

    def forward(self, x):
        x = _lib.require_cuda(x, "x")
        return self._launch(x, th.empty(self.static_shape(x.shape), dtype=x.dtype, device=x.device))

    def run_static(self, x, out, src):
        """Inside a captured forward: writes into the static buffer ``out`` of ``static_shape(x.shape)``; ``src`` is unused (nothing is
        per frame) and nothing is allocated once the noise plane lives on the device (the warm-up forward before the capture)."""
        if tuple(out.shape) != self.static_shape(x.shape):
            raise RuntimeError(f"padding bend: output buffer {tuple(out.shape)} for a padded map {self.static_shape(x.shape)}")
        return self._launch(x, out)


def _inverse_maps_translate(t):
    """dst = src + t  ->  src = dst - t (pixels)."""
    t = t.reshape(-1, 2).float()
    m = th.zeros(t.shape[0], 6, device=t.device)  # stays where the modulation lives (HBM during a render)
    m[:, 0] = 1.0
    m[:, 4] = 1.0
    m[:, 2] = -t[:, 0]
    m[:, 5] = -t[:, 1]
    return m


def _inverse_maps_scale(s, cw, ch):
    s = s.float()
    if s.dim() == 1:
        s = s[:, None].expand(-1, 2)
    cx, cy = (cw - 1) / 2.0, (ch - 1) / 2.0
    m = th.zeros(s.shape[0], 6, device=s.device)
    m[:, 0] = 1.0 / s[:, 0]
    m[:, 4] = 1.0 / s[:, 1]
    m[:, 2] = cx - cx / s[:, 0]
    m[:, 5] = cy - cy / s[:, 1]
    return m


def _inverse_maps_rotate(angle_deg, cw, ch):
    a = th.deg2rad(angle_deg.float().reshape(-1))
    cx, cy = (cw - 1) / 2.0, (ch - 1) / 2.0
    cos, sin = th.cos(a), th.sin(a)
    # forward (OpenCV/kornia get_rotation_matrix2d): dst = R(src - c) + c with R = [[cos, sin], [-sin, cos]];
    # inverse: src = R^T (dst - c) + c
    m = th.zeros(a.shape[0], 6, device=a.device)
    m[:, 0], m[:, 1] = cos, -sin
    m[:, 3], m[:, 4] = sin, cos
    m[:, 2] = cx - cos * cx + sin * cy
    m[:, 5] = cy - sin * cx - cos * cy
    return m


class Translate(NetworkBend):
    """Horizontal scrolling (reference :52-72): three STACKED reflection pads (w/2 | w/2, then w | w, then w | 0 — each
    mirrors the canvas built so far, which is what makes a scroll of w pixels land on the same features), add noise,
    translate, centre crop."""

    def __init__(self, modulation, h, w, noise):
        pads = [(int(w / 2), int(w / 2), 0, 0), (w, w, 0, 0), (w, 0, 0, 0)]
        sequential_fn = lambda b: AffineReflectWarp(_inverse_maps_translate(b), pads, noise)  # noqa: E731
        super().__init__(sequential_fn, modulation)


class Zoom(NetworkBend):
    def __init__(self, modulation, h, w):
        padding = int(max(h, w)) - 1
        pads = (padding,) * 4
        sequential_fn = lambda b: AffineReflectWarp(_inverse_maps_scale(b, w + 2 * padding, h + 2 * padding), pads)  # noqa: E731
        super().__init__(sequential_fn, modulation)


class Rotate(NetworkBend):
    def __init__(self, modulation, h, w):
        padding = int(max(h, w) * (1 - math.sqrt(2) / 2))
        pads = (padding,) * 4
        sequential_fn = lambda b: AffineReflectWarp(_inverse_maps_rotate(b, w + 2 * padding, h + 2 * padding), pads)  # noqa: E731
        super().__init__(sequential_fn, modulation)


class Ablate(NetworkBend):
    """Zero the channels ``channels``: always (no modulation), or on the frames whose modulation is above 0.5 (a gate: the other
    frames pass through; realised as a multiplication by 0 or 1)."""

    def __init__(self, modulation=None, channels=None):
        if modulation is None:
            super().__init__(lambda _: PointBend("ablate", None, channels), None)
        else:
            super().__init__(lambda m: PointBend("multiply", (th.as_tensor(m) <= 0.5).float(), channels), modulation)


class Invert(NetworkBend):
    """x -> 1 - x on the channels ``channels``."""

    def __init__(self, channels=None):
        super().__init__(lambda _: PointBend("invert", None, channels), None)


class ScalarMultiply(NetworkBend):
    def __init__(self, modulation, channels=None):
        super().__init__(lambda m: PointBend("multiply", m, channels), modulation)


class BinaryThreshold(NetworkBend):
    """x -> 1 where x exceeds the frame's modulation, else 0."""

    def __init__(self, modulation, channels=None):
        super().__init__(lambda m: PointBend("threshold", m, channels), modulation)


class Erode(NetworkBend):
    """Minimum over a square window of radius round(modulation) pixels (0 .. 16) around every pixel."""

    def __init__(self, modulation, channels=None):
        super().__init__(lambda m: MorphBend("erode", th.round(th.as_tensor(m).float()), channels), modulation)


class Dilate(NetworkBend):
    """Maximum over a square window of radius round(modulation) pixels (0 .. 16) around every pixel."""

    def __init__(self, modulation, channels=None):
        super().__init__(lambda m: MorphBend("dilate", th.round(th.as_tensor(m).float()), channels), modulation)


_REMAP_OPS = {"mirror": 0, "kaleidoscope": 1, "swirl": 2, "ripple": 3, "displace": 4}  # `op` of maua_bend_remap_f32
_REMAP_BORDERS = {"reflect": 0, "clamp": 1}                                             # `border` of maua_bend_remap_f32
_REMAP_PARAMS = 4                                                                       # MAUA_BEND_REMAP_PARAMS
_MAX_SECTORS = 64


class RemapBend(_ChannelBend):
    """y = x sampled bilinearly at a per-pixel source coordinate (``op`` one of _REMAP_OPS) on the channels ``channels``, the others
    copied through: one launch of maua_bend_remap_f32, whose header comment defines every op.  ``table`` [rows, 4] holds the device's
    parameter rows (angles in radians, the mirror's normal as a unit vector); ``border``: how a coordinate outside the map is folded
    back, one of _REMAP_BORDERS; ``field`` [F, 2, fh, fw]: the static flow-field bank of "displace".  What the device would pass through
    as a bad row is refused here."""

    def __init__(self, op, table, channels, border="reflect", field=None, n_channels=None):
        if op not in _REMAP_OPS:
            raise ValueError(f"unknown remap bend {op!r} ({' | '.join(_REMAP_OPS)})")
        if border not in _REMAP_BORDERS:
            raise ValueError(f"unknown border {border!r} ({' | '.join(_REMAP_BORDERS)})")
        table = th.as_tensor(table).float()
        if table.dim() != 2 or table.shape[0] < 1 or table.shape[1] != _REMAP_PARAMS:
            raise ValueError(f"remap bend parameters must be [n_frames, {_REMAP_PARAMS}] (got shape {tuple(table.shape)})")
        if not bool(th.isfinite(table).all()):
            raise ValueError(f"{op} bend: the modulation holds a NaN or an infinity")
        if op == "kaleidoscope" and not bool(((th.round(table[:, 0]) >= 1) & (th.round(table[:, 0]) <= _MAX_SECTORS)).all()):
            raise ValueError(f"kaleidoscope sectors must lie in 1 .. {_MAX_SECTORS}")
        if op in ("swirl", "ripple") and not bool((table[:, 1] > 0).all()):
            raise ValueError(f"{op} bend: the {'radius' if op == 'swirl' else 'wavelength'} must be positive")
        if (field is not None) != (op == "displace"):
            raise ValueError("a flow field goes with the displace bend, and only with it")
        if field is not None:
            field = th.as_tensor(field)
            if field.dim() != 4 or field.shape[1] != 2 or min(field.shape) < 1:
                raise ValueError(f"the flow field must be a bank [F, 2, fh, fw] of (dx, dy) planes (got shape {tuple(field.shape)})")
            field = field.float()
            if not bool(th.isfinite(field).all()):
                raise ValueError("the flow field holds a NaN or an infinity")
        super().__init__(table, channels, n_channels)
        self.op, self.border, self.field = _REMAP_OPS[op], _REMAP_BORDERS[border], field
        self._field_dev = {}  # device -> the field bank there; never evicted, like _dev

    def _launch(self, x, y, table, mask, src):
        b, c, h, w = x.shape
        field = None
        if self.field is not None:
            key = str(x.device)
            if key not in self._field_dev:
                self._field_dev[key] = self.field.to(x.device).contiguous()
            field = self._field_dev[key]
        frames, fh, fw = (0, 0, 0) if field is None else (field.shape[0], field.shape[2], field.shape[3])
        _lib.call("maua_bend_remap_f32", x, y, b, c, h, w, self.op, self.border, table, self.sequence_rows, field, frames, fh, fw, mask, src)
        return y


def _modulation_columns(name, modulation, columns):
    """The column rule of the remap bends: ``modulation`` is [n_frames] (the first parameter) or [n_frames, k] (the first k parameters, in
    the order of ``columns`` = ((name, constant or None), ...)); every parameter without a column takes its keyword constant for all
    frames.  Returns [n_frames, len(columns)] where the modulation lives."""
    m = th.as_tensor(modulation).float()
    if m.dim() == 1:
        m = m[:, None]
    if m.dim() != 2 or m.shape[0] < 1 or not 1 <= m.shape[1] <= len(columns):
        raise ValueError(f"{name} modulation must be [n_frames] or [n_frames, k] with k <= {len(columns)} columns "
                         f"({', '.join(c for c, _ in columns)}), got shape {tuple(m.shape)}")
    missing = columns[m.shape[1]:]
    for column, constant in missing:
        if constant is None:
            raise ValueError(f"{name} needs {column}: as a modulation column or as the keyword {column}=")
    if missing:
        m = th.cat([m, th.tensor([float(c) for _, c in missing], device=m.device).expand(m.shape[0], -1)], 1)
    return m


def _remap_rows(*columns):
    """[n_frames, 4] device rows from up to four columns (the rest 0)."""
    rows = th.zeros(columns[0].shape[0], _REMAP_PARAMS, device=columns[0].device)
    for i, column in enumerate(columns):
        rows[:, i] = column
    return rows


class Mirror(NetworkBend):
    """Mirror across a line: the side the normal points away from shows the other side's reflection.  Modulation columns: ``angle`` of the
    normal in degrees (0: the normal points along +x, so the left half mirrors the right half; 90: the top mirrors the bottom), ``offset`` of
    the line from the map's centre along the normal, in pixels."""

    def __init__(self, modulation, offset=0.0, channels=None, border="reflect"):
        def make(m):
            m = _modulation_columns("Mirror", m, (("angle", None), ("offset", offset)))
            a = th.deg2rad(m[:, 0])
            return RemapBend("mirror", _remap_rows(th.cos(a), th.sin(a), m[:, 1]), channels, border)

        super().__init__(make, modulation)


class Kaleidoscope(NetworkBend):
    """Fold the map into ``sectors`` mirrored wedges about its centre.  Modulation columns: ``rotation`` of the sampled content in degrees,
    ``angle`` of the wedge pattern in degrees, ``sectors`` (rounded, 1 .. 64)."""

    def __init__(self, modulation, angle=0.0, sectors=6, channels=None, border="reflect"):
        def make(m):
            m = _modulation_columns("Kaleidoscope", m, (("rotation", None), ("angle", angle), ("sectors", sectors)))
            return RemapBend("kaleidoscope", _remap_rows(m[:, 2], th.deg2rad(m[:, 1]), th.deg2rad(m[:, 0])), channels, border)

        super().__init__(make, modulation)


class Swirl(NetworkBend):
    """Rotate about the centre by an angle that decays with the distance r from it: ``strength`` exp(-r / ``radius``).  Modulation columns:
    ``strength`` in degrees, ``radius`` in pixels (> 0)."""

    def __init__(self, modulation, radius=None, channels=None, border="reflect"):
        def make(m):
            m = _modulation_columns("Swirl", m, (("strength", None), ("radius", radius)))
            return RemapBend("swirl", _remap_rows(th.deg2rad(m[:, 0]), m[:, 1]), channels, border)

        super().__init__(make, modulation)


class Ripple(NetworkBend):
    """Push every pixel along its radius by ``amplitude`` sin(2 pi (r / ``wavelength`` - ``phase``)).  Modulation columns: ``amplitude`` in
    pixels, ``wavelength`` in pixels (> 0), ``phase`` in cycles (a rising phase moves the rings outwards)."""

    def __init__(self, modulation, wavelength=None, phase=0.0, channels=None, border="reflect"):
        def make(m):
            m = _modulation_columns("Ripple", m, (("amplitude", None), ("wavelength", wavelength), ("phase", phase)))
            return RemapBend("ripple", _remap_rows(m[:, 0], m[:, 1], m[:, 2]), channels, border)

        super().__init__(make, modulation)


class Displace(NetworkBend):
    """Displace along a flow field ("liquid"): ``field`` [F, 2, fh, fw] is a static looping bank of (dx, dy) planes (an ``ar.perlin_noise``
    loop, say), stretched over the map.  Modulation columns: ``amplitude`` in pixels per unit of the field, ``position`` in the loop in
    frames of the bank (fractional positions blend neighbouring frames, any value wraps: a modulated speed is a cumulative sum)."""

    def __init__(self, modulation, field, position=0.0, channels=None, border="reflect"):
        def make(m):
            m = _modulation_columns("Displace", m, (("amplitude", None), ("position", position)))
            return RemapBend("displace", _remap_rows(m[:, 0], m[:, 1]), channels, border, field=field)

        super().__init__(make, modulation)
