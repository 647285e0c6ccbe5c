"""Whole-forward reference of the StyleGAN2 generator for the dispatch-level tests (tests/test_forward_routes_host.py,
tests/test_forward_matrix_gpu.py): nothing here needs a GPU, and nothing here comes from a kernel under test.

  reference(case) / rounding(case)   the oracle's layer functions (oracle/stylegan2_oracle.py) walked in float64 / float32 on the CPU from the
                                     seeded state dict: every activation map before and after its bend, the image after every resolution
  bounds(case)                       per-element bounds  4 * G * max |fp32 - fp64|  of every map and image (``MARGIN``, ``winograd_gain``)
  expected_route(g, batch, flags)    the documented dispatch rules of models/stylegan2.py restated as a pure host function
  reachable_modes()                  conv_mode over every layer of every supported generator
  reachable_routes()                 the (mode, path, prescaled, posted, rgb, family) tuples of expected_route over every supported generator
                                     in the three orientations (square, 2:1 behind a widening layer-0 bend, 1:2)
  CASES                              the whole-forward cases of the GPU matrix, shared with the host test that proves their coverage

THE BOUND.  A correct fp32 forward differs from the fp64 one by rounding that grows with depth and with the data, so it is measured, per
map, on the case's own operands: E_l = max |fp32 - fp64| / max |fp64| of map l from the two CPU forwards (E_img: absolute, on the image).
A kernel may accumulate in another order than the CPU's fp32 convolution (margin 4, as tests/pitch_ref.py and tests/iir_ref.py take over an
fp32 emulation), and the Winograd forms amplify rounding where the oracle's direct convolution does not: G = the largest ratio
(rounding of the fp32 emulation of the mode a layer takes) / (rounding of the fp32 direct form) on the same operands over the layers of
the test generators, measured on the CPU by tools/forward_tolerance.py and recorded in tests/golden/forward_tolerance.json.  The direct
form of that ratio accumulates in float32 term after term, as E's own forward does: measured against conv_ref._direct_conv, which sums in
float64 and rounds once, the ratio counts the accumulation a second time (36 instead of 2.5; both are in the JSON, only the first is used).
G is taken over the layers of the cases of one orientation (square, 2:1, 1:2): the ratio is a maximum over the elements of seeded operands
and moves with the shape (2.2 .. 4.7 for the 2-D Winograd form at 16 x 32 over four seeds, 4.68 on the recorded one), and the shapes
only a 2:1 generator runs must not widen the bound of a square forward.
"""
import dataclasses
import functools
import json
import math
import os

import torch

from maua_stylegan2_amd import seeding
from oracle import ops_oracle as ops
from oracle import stylegan2_oracle as so

import conv_ref

MARGIN = 4.0  # over the fp32 CPU forward (tests/pitch_ref.py, tests/iir_ref.py)
TOLERANCE_JSON = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "forward_tolerance.json")
OLD_IMAGE_TOL = 1e-3  # the whole-generator bound of tests/test_generator_gpu.py; every image bound here must be 10 x tighter
# ... but for these square cases from before that was asserted, on checkpoints at ToRGB gain 1 (images of max |x| 4 .. 8 and std 2 .. 3, where
# the absolute bound is 4 .. 8 x what it is on a [-1, 1] image): 1.0e-4 .. 1.4e-4 on one host and up to 20 % apart on another, which
# blocks its fp32 sums otherwise.  name -> asserted ceiling of the image bound (5 x under OLD_IMAGE_TOL).
IMAGE_BOUND_EXCEPTIONS = {name: 2e-4 for name in ("256-cm2-b8", "512-cm1-b1", "1024-cm1-b1", "latent-input", "bend-torgb")}

PATHS = ("const", "plain", "lowres", "rgb_partial", "torgb", "pair", "fused")


@functools.lru_cache(maxsize=None)
def winograd_gain(orient="square"):
    """G (>= 1): the largest per-mode ratio of tests/golden/forward_tolerance.json over the layers of the cases of ``orient``."""
    with open(TOLERANCE_JSON) as f:
        table = json.load(f)
    return max(1.0, max(float(v) for v in table["G_by_orientation"][orient].values()))


# ---- cases ---------------------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Case:
    """One whole forward.  The fields up to ``blur`` decide what is computed (the reference depends on them alone); the others decide which
    kernels compute it.  ``noise``: "frame" ([B, 1, h, w] per layer), "shared" ([1, 1, h, w]), "buffer" (None: the checkpoint's buffers) or
    "mix" (the three in turn over the layers).  ``trunc``: per-frame truncation of the 2 * batch frames, or None.  ``bends``: ((layer id,
    "flip" | "point"), ...).  ``blur``: None, "asym" (conv_ref.asymmetric_taps) or "nonsep" (a 4 x 4 matrix of rank 2) in place of every
    Blur's taps.  ``gen`` / ``cls``: attributes set on the Generator / on the layer classes for the forward.  ``u8``: None, or whether
    ``tap_float_image`` is on for a forward captured with ``frames_u8``.  ``acts``: return_activation_maps (eager only).  ``orient``:
    "square", "wide" (a replicate ``ar.Pad((2, 2, 0, 0))`` on layer id 0 makes the 4 x 4 constant 4 x 8: every map is 2:1) or "tall"
    (``ar.Pad((0, 0, 2, 2))``, 8 x 4, 1:2); a non-square generator is built with ``output_size`` 1920 / 1080, whose noise buffers have the
    maps' shapes (a captured forward is bound to noise of the buffers' shapes only), seeded here."""
    name: str
    size: int
    cm: int
    batch: int
    seed: int
    constant_input: bool = True
    min_rgb_size: int = 4
    unsaturated: bool = False
    trunc: tuple = None
    noise: str = "frame"
    bends: tuple = ()
    blur: str = None
    gen: tuple = ()
    cls: tuple = ()
    u8: bool = None
    acts: bool = False
    orient: str = "square"

    @property
    def math_key(self):
        return (self.size, self.cm, self.batch, self.seed, self.constant_input, self.min_rgb_size, self.unsaturated, self.trunc, self.noise,
                self.bends, self.blur, self.orient)

    @property
    def all_bends(self):
        """``bends`` behind the orientation's widening bend on layer id 0."""
        return (() if self.orient == "square" else ((0, "pad"),)) + tuple(self.bends)

    @property
    def output_size(self):
        """What ``Generator(output_size=...)`` is built with (None: square noise buffers)."""
        return OUTPUT_SIZE[self.orient]

    @property
    def capturable(self):
        """capture_graph takes bends with ``run_static`` only and hands out no activation maps."""
        return not self.acts and all(kind in ("point", "pad") for _, kind in self.all_bends)


ORIENTATIONS = ("square", "wide", "tall")
OUTPUT_SIZE = {"square": None, "wide": 1920, "tall": 1080}
PADS = {"wide": (2, 2, 0, 0), "tall": (0, 0, 2, 2)}  # (left, right, top, bottom) of the layer-0 bend


def aspect(orient):
    """(rows, columns) of every map of the orientation as multiples of the square generator's side."""
    return {"square": (1, 1), "wide": (1, 2), "tall": (2, 1)}[orient]


_LOW = (("StyledConv", "fused_blur_min_width", 32),)  # 128^2, cm 1: convs.8 (64^2 -> 128^2, 256 -> 128 channels) then takes "fused"


def _switch(name, **kw):
    kw.setdefault("cls", ())
    kw["cls"] = _LOW + tuple(kw["cls"])
    return Case(name, 128, 1, 2, kw.pop("seed", 21), **kw)


CASES = [
    # default thresholds
    Case("512-cm1-b1", 512, 1, 1, 11),
    Case("256-cm2-b8", 256, 2, 8, 12),
    Case("64-cm2-b3", 64, 2, 3, 13),
    Case("1024-cm1-b1", 1024, 1, 1, 14),  # the only home of mode 4 and of mode 0 above 4^2 (16-channel layers): see reachable_modes
    # switches, 128^2 cm 1 batch 2
    _switch("acts", acts=True),
    _switch("no-style-fold", gen=(("style_fold", False),)),
    _switch("no-rgb-fusion", gen=(("disable_rgb_fusion", True),)),
    _switch("no-partial-rgb", cls=(("StyledConv", "partial_rgb_fusion", False),)),
    _switch("no-lowres-fusion", cls=(("StyledConv", "lowres_fusion", False),)),
    _switch("no-lowres-up2d", cls=(("StyledConv", "lowres_up2d", False),)),
    _switch("no-upconv-winograd", cls=(("ModulatedConv2d", "upconv_winograd", False),)),
    _switch("truncation", trunc=(0.7, 1.0, 0.4, 0.9)),
    _switch("noise-shared", noise="shared"),
    _switch("noise-buffer", noise="buffer"),
    _switch("noise-mix", noise="mix"),
    _switch("latent-input", constant_input=False, trunc=(0.8, 0.6, 1.0, 0.5)),
    _switch("min-rgb-16", min_rgb_size=16),
    _switch("min-rgb-above", min_rgb_size=256),
    _switch("blur-asym", blur="asym"),
    _switch("blur-nonsep", blur="nonsep"),
    # bends: eager (a plain nn.Module) on the constant, then on a layer of every path; captured (a run_static point bend) on three of them
    _switch("bend-const", bends=((0, "flip"),)),
    _switch("bend-lowres", bends=((3, "flip"),)),       # convs.1, 8^2 plain
    _switch("bend-lowres-up", bends=((4, "flip"),)),    # convs.2, 8^2 -> 16^2
    _switch("bend-pair", bends=((8, "flip"),)),         # convs.6, 32^2 -> 64^2 (512 input channels: not fusable)
    _switch("bend-rgb-partial", bends=((9, "flip"),)),  # convs.7, 64^2, 256 channels
    _switch("bend-fused", bends=((10, "flip"),)),       # convs.8
    _switch("bend-last", bends=((11, "flip"),)),        # convs.9, 128 channels
    Case("bend-torgb", 256, 1, 1, 22, bends=((13, "flip"),)),          # convs.11, 64 channels at 256^2: "torgb" unbent
    _switch("bend-point-const", bends=((0, "point"),)),
    _switch("bend-point-fused", bends=((10, "point"),)),
    _switch("bend-point-two", bends=((7, "point"), (9, "point"))),     # convs.5 (first mode-5 layer) and convs.7
    # uint8 frames from the captured forward
    Case("u8-torgb-tap", 256, 1, 2, 23, unsaturated=True, u8=True),
    Case("u8-torgb", 256, 1, 2, 23, unsaturated=True, u8=False),
    Case("u8-partial-tap", 64, 1, 2, 24, unsaturated=True, u8=True),
    Case("u8-partial", 64, 1, 2, 24, unsaturated=True, u8=False),
    Case("u8-bend-tap", 256, 1, 2, 23, unsaturated=True, u8=True, bends=((13, "point"),)),
    Case("u8-bend", 256, 1, 2, 23, unsaturated=True, u8=False, bends=((13, "point"),)),
    # non-square generators (the layer-0 ar.Pad): the smallest ones that reach the layer routes no square generator takes (reachable_routes).
    # All on the unsaturated checkpoint (images of std 0.3 .. 1 instead of 2 .. 3, the range a render delivers): the image bound is absolute,
    # and with the G of the 2:1 maps it stays 10 x under OLD_IMAGE_TOL only on such an image (test_fp32_forward_is_inside_its_own_bounds)
    Case("wide-64-cm2-b3", 64, 2, 3, 31, orient="wide", unsaturated=True),  # conv1 at 4 x 8 through the convolution, 1/lowres>, mode 5 and mode 6 pair at 16 x 32
    Case("tall-64-cm2-b1", 64, 2, 1, 32, orient="tall", unsaturated=True),  # conv1 at 8 x 4, mode 2 lowres at 32 x 16, 1/pair> with split K
    Case("tall-64-cm2-b8", 64, 2, 8, 33, orient="tall", noise="shared", unsaturated=True),  # ... without
    Case("wide-256-cm1-b2-tap", 256, 1, 2, 34, orient="wide", unsaturated=True, u8=True),  # fused from a 128 x 256 input; 256 x 512 frames
    Case("wide-256-cm1-b2", 256, 1, 2, 34, orient="wide", unsaturated=True, u8=False),
    Case("tall-256-cm1-b2-tap", 256, 1, 2, 35, orient="tall", unsaturated=True, u8=True),  # 512 x 256 frames, convs.10 as pair
    Case("tall-256-cm1-b2", 256, 1, 2, 35, orient="tall", unsaturated=True, u8=False),
    Case("wide-64-cm2-b2", 64, 2, 2, 36, orient="wide", noise="buffer", unsaturated=True),  # the 2:1 noise buffers of Generator(output_size=1920)
    Case("wide-1024-cm1-b1", 1024, 1, 1, 37, orient="wide", unsaturated=True),  # mode 4 and the 16-channel direct + ToRGB layer on 2:1 maps
]
CASE_BY_NAME = {c.name: c for c in CASES}
assert len(CASE_BY_NAME) == len(CASES)

# modes of reachable_modes() that only a configuration too heavy for a few-second test reaches, with the reason (the kernel-instance tests
# cover them in isolation).  Empty: the 1024^2 cm 1 case above reaches what nothing smaller does.
MODES_NOT_IN_CASES = {}
# cases that would belong to the list and are left out, with the reason
CASES_LEFT_OUT = {
    "tall-1024-cm1-b1": "the portrait twin of wide-1024-cm1-b1 (mode 4 and the 16-channel direct + ToRGB layer on 1:2 maps): a second fp64 "
                        "and fp32 CPU walk of a 2-megapixel generator, twice the time of 1024-cm1-b1's, for one more orientation of "
                        "two layers; the 1:2 frame epilogue, the fused layer and the pair are in tall-256-cm1-b2",
}

POINT_GAIN = 0.75  # the captured bend: PointBend("multiply", [0.75]) — exact in fp32 and fp64


def nonseparable_taps():
    """A 4 x 4 tap matrix of rank 2 with the sum 4 of a Blur's taps (upsample_factor ** 2): asymmetric_taps with 1 / 16 moved from one
    diagonal entry to another — every entry stays an integer / 16."""
    k = conv_ref.asymmetric_taps().clone()
    k[0, 0] += 1.0 / 16.0
    k[1, 1] -= 1.0 / 16.0
    return k


def blur_taps(case):
    return {None: None, "asym": conv_ref.asymmetric_taps(), "nonsep": nonseparable_taps()}[case.blur]


def state_dict(case):
    gain = seeding.unsaturated_rgb_gain(case.size) if case.unsaturated else 1.0
    sd = seeding.seeded_state_dict(case.size, seed=case.seed, channel_multiplier=case.cm, constant_input=case.constant_input, rgb_gain=gain)
    taps = blur_taps(case)
    if taps is not None:
        for key in sd:
            if key.endswith("conv.blur.kernel"):
                sd[key] = taps.clone()
    if case.orient != "square":  # the buffers of Generator(output_size=1920 | 1080), seeded (the constructor draws them with torch.randn)
        for i, hw in enumerate(noise_shapes(case)):
            sd[f"noises.noise_{i}"] = torch.from_numpy(seeding.seeded_array(case.seed, f"noises.{case.orient}_{i}", (1, 1) + hw))
    return sd


def noise_shapes(case):
    """(h, w) of every noise map of the case's generator."""
    mh, mw = aspect(case.orient)
    return [(mh * r, mw * r) for r in seeding.noise_sizes(case.size)]


def noise_form(case, layer):
    return case.noise if case.noise != "mix" else ("buffer", "shared", "frame")[layer % 3]


def inputs(case):
    """The seeded inputs of the case's 2 * batch frames (the captured forward is bound to all of them; the eager forward and the reference
    take the first ``batch``): dict(sd, latents [2B, n_latent, 512], noise (per layer None / [1, 1, h, w] / [2B, 1, h, w]), trunc [2B] or
    None, tl [1, 512] or None)."""
    n = 2 * case.batch
    log_size = int(math.log2(case.size))
    if case.orient == "square":
        per_frame = seeding.seeded_noise(n, case.size, seed=case.seed + 2)
    else:
        per_frame = [torch.from_numpy(seeding.seeded_array(case.seed + 2, f"noise_{i}", (n, 1) + hw)) for i, hw in enumerate(noise_shapes(case))]
    noise = []
    for i, nz in enumerate(per_frame):
        form = noise_form(case, i)
        noise.append(None if form == "buffer" else nz[:1].contiguous() if form == "shared" else nz)
    trunc = tl = None
    if case.trunc is not None:
        assert len(case.trunc) == n
        trunc = torch.tensor(case.trunc, dtype=torch.float32)
        tl = torch.from_numpy(seeding.seeded_array(case.seed + 3, "truncation_latent", (1, 512)))
    return dict(sd=state_dict(case), latents=seeding.seeded_latents(n, 2 * log_size - 2, seed=case.seed + 1), noise=noise, trunc=trunc, tl=tl)


def frames(noise, first, count):
    """The noise list of frames [first, first + count) as Generator.forward takes it."""
    return [nz if nz is None or nz.shape[0] == 1 else nz[first: first + count].contiguous() for nz in noise]


class FlipGain(torch.nn.Module):
    """The eager bend of the matrix: a plain module without run_static."""

    def forward(self, x):
        return x.flip(-1) * 0.5 + 0.25


def bend_callables(case):
    """{layer id: fp64 / fp32 callable}: the exact restatement of device_bends(case) (0.5, 0.25 and 0.75 are exact in every format)."""
    fns = {"flip": lambda x: x.flip(-1) * 0.5 + 0.25, "point": lambda x: x * POINT_GAIN,
           "pad": lambda x: torch.nn.functional.pad(x, PADS[case.orient], mode="replicate")}  # (copies: exact in every format)
    return {layer: fns[kind] for layer, kind in case.all_bends}


def device_bends(case):
    from maua_stylegan2_amd.audioreactive.bend import Pad, PointBend

    make = {"flip": FlipGain, "point": lambda: PointBend("multiply", [POINT_GAIN], None), "pad": lambda: Pad(PADS[case.orient])}
    return [{"layer": layer, "transform": make[kind]()} for layer, kind in case.all_bends]


# ---- the reference walk ------------------------------------------------------------------------------------------------------------------
def walk(sd, latents, noise, trunc=None, tl=None, bends=None, min_rgb_size=4):
    """Generator.forward of the reference (models/stylegan2.py:526-576, input_is_latent) from the oracle's layer functions, in the dtype of
    ``latents`` (``sd`` must hold the same).  Returns dict(raw = every activation map before its bend, acts = after it (what
    return_activation_maps hands out), images = the image after every resolution from 4^2 up (None below min_rgb_size), image = the last,
    styles = every layer's [B, Cin] styles)."""
    dt = latents.dtype
    size = min(sd[[k for k in sd if k.startswith("noises.noise_")][-1]].shape[-2:])  # (the short side: 2:1 buffers double the other)
    log_size = int(math.log2(size))
    b = latents.shape[0]
    noise = [sd[f"noises.noise_{i}"] if nz is None else nz.to(dt) for i, nz in enumerate(noise)]
    if trunc is not None:
        t = trunc.to(dt).reshape(-1)
        center = tl.to(dt) if tl is not None else torch.zeros(1, latents.shape[-1], dtype=dt)
        latents = center[None] + t[:, None, None] * (latents - center[None])
    bends = bends or {}
    raw, acts, images, styles = [], [], [], []

    def layer(layer_id, prefix, x, lat_row, nz, up):
        y = so.styled_conv(sd, prefix, x, latents[:, lat_row], nz, up)
        styles.append(so.equal_linear(latents[:, lat_row], sd[f"{prefix}.conv.modulation.weight"], sd[f"{prefix}.conv.modulation.bias"]))
        raw.append(y)
        y = bends[layer_id](y) if layer_id in bends else y
        acts.append(y)
        return y

    if "input.linear.weight" in sd:
        w_in = sd["input.linear.weight"]
        first = torch.nn.functional.linear(latents[:, 0], w_in * (1 / math.sqrt(w_in.shape[1])))
        out = ops.fused_leaky_relu(ops.fused_leaky_relu(first, sd["input.linear.bias"]), sd["input.activate.bias"]).reshape(b, -1, 4, 4)
    else:
        out = sd["input.input"].repeat(b, 1, 1, 1)
    if 0 in bends:
        out = bends[0](out)
    out = layer(1, "conv1", out, 0, noise[0], False)
    current = 4
    image = so.to_rgb(sd, "to_rgb1", out, latents[:, 1]) if min_rgb_size <= current else None
    images.append(image)
    i = 1
    for n in range(log_size - 2):
        current *= 2
        out = layer(2 * n + 2, f"convs.{2 * n}", out, i, noise[2 * n + 1], True)
        out = layer(2 * n + 3, f"convs.{2 * n + 1}", out, i + 1, noise[2 * n + 2], False)
        if min_rgb_size <= current:
            image = so.to_rgb(sd, f"to_rgbs.{n}", out, latents[:, i + 2], image)
        images.append(image)
        i += 2
    return dict(raw=raw, acts=acts, images=images, image=image, styles=styles)


def posted_map(fwd, i):
    """Map i as a layer that posts stores it (the style fold): multiplied by the styles of the layer behind it."""
    return fwd["raw"][i] * fwd["styles"][i + 1][:, :, None, None]


def walk_as(dt, sd, latents, noise, trunc=None, tl=None, bends=None, min_rgb_size=4):
    """``walk`` with the state dict and every input cast to ``dt`` first."""
    with torch.no_grad():
        return walk({k: v.to(dt) for k, v in sd.items()}, latents.to(dt), [None if nz is None else nz.to(dt) for nz in noise],
                    trunc, tl, bends, min_rgb_size)


@functools.lru_cache(maxsize=None)
def _forward(math_key, dt):
    case = next(c for c in CASES if c.math_key == math_key)
    inp = inputs(case)
    b = case.batch
    return walk_as(dt, inp["sd"], inp["latents"][:b], frames(inp["noise"], 0, b), None if inp["trunc"] is None else inp["trunc"][:b], inp["tl"],
                   bend_callables(case), case.min_rgb_size)


def reference(case):
    """The case's first ``batch`` frames in float64.  Shared by every case with the same ``math_key``; treat as read-only."""
    return _forward(case.math_key, torch.float64)


def rounding(case):
    """The same forward in float32 on the CPU."""
    return _forward(case.math_key, torch.float32)


def _max_abs_diff(a, b):
    return float((a.double() - b.double()).abs().max())


def bounds_of(ref, rnd, gain=None):
    """Per-element bounds of a forward from its float64 and float32 CPU walks: for map l  4 * G * E_l * max |ref_l|  with
    E_l = max |fp32_l - fp64_l| / max |fp64_l|  (= 4 * G * max |fp32_l - fp64_l|), for an image  4 * G * max |fp32 - fp64|.  Same layout as
    ``walk`` (None where there is no image), plus posted = the bounds of posted_map(i) and E = the relative figures."""
    g = winograd_gain() if gain is None else gain

    def one(a64, a32):
        return None if a64 is None else MARGIN * g * _max_abs_diff(a32, a64)

    out = {key: [one(a, b) for a, b in zip(ref[key], rnd[key])] for key in ("raw", "acts", "images")}
    out["image"] = one(ref["image"], rnd["image"])
    out["posted"] = [one(posted_map(ref, i), posted_map(rnd, i)) for i in range(len(ref["raw"]) - 1)]
    out["E"] = [_max_abs_diff(b, a) / float(a.abs().max()) for a, b in zip(ref["acts"], rnd["acts"])]
    return out


def bounds(case):
    return bounds_of(reference(case), rounding(case), winograd_gain(case.orient))


def check(name, got, want, bound):
    """(worst error / bound, message): every element of ``got`` (a float32 tensor on any device) against the float64 ``want``."""
    err = float((got.detach().cpu().double() - want).abs().max())
    assert tuple(got.shape) == tuple(want.shape), (name, tuple(got.shape), tuple(want.shape))
    return err / bound, f"{name}: max |got - fp64| = {err:.3e}, bound {bound:.3e} ({err / bound:.2f} of it)"


# ---- uint8 frames ----------------------------------------------------------------------------------------------------------------------------
def frames_u8_reference(image64, bound):
    """(levels [B, H, W, 3] uint8 = floor((clamp(x) + 1) * 127.5), ambiguous [B, H, W, 3] bool) from the fp64 image alone: a pixel is
    ambiguous when its fp64 value lies within ``bound`` * 127.5 of a boundary between two levels, i.e. where an fp32 image inside its
    bound may land on the neighbouring level; everywhere else the frame must be exact."""
    v = ((image64.clamp(-1, 1) + 1) * 127.5).permute(0, 2, 3, 1)
    levels = v.floor().clamp(0, 255)
    margin = bound * 127.5
    near = ((v - v.floor()) < margin) | ((v.floor() + 1 - v) < margin)
    # (the ends of the range: below level 0 / above 255 there is no neighbouring level — a clamped pixel further than the bound inside the
    # clamp is exact; v == 255.0 exactly is level 255)
    clamped = (image64.permute(0, 2, 3, 1) <= -1 - bound) | (image64.permute(0, 2, 3, 1) >= 1 + bound)
    return levels.to(torch.uint8), near & ~clamped


# ---- reachable modes -----------------------------------------------------------------------------------------------------------------------------
def skeleton(size, cm, constant_input=True, min_rgb_size=4, taps=None, output_size=None):
    """A Generator on the meta device (no weights: shapes, class thresholds and the host predicates are all the route depends on) with real
    blur taps on its up-sampling layers."""
    from maua_stylegan2_amd.models.stylegan2 import Generator

    with torch.device("meta"):
        g = Generator(size, 512, 8, channel_multiplier=cm, constant_input=constant_input, min_rgb_size=min_rgb_size, output_size=output_size)
    k = torch.from_numpy(seeding.fir_kernel_2d((1, 3, 3, 1), gain=4.0).copy()) if taps is None else taps.clone()
    for conv in g.convs[0::2]:
        conv.conv.blur.kernel = k.clone()
    return g


def layer_shapes(g, orient="square"):
    """(tag, StyledConv, layer id, (input h, input w)) of every 3 x 3 layer in forward order, behind the orientation's layer-0 bend."""
    mh, mw = aspect(orient)
    out = [("conv1", g.conv1, 1, (4 * mh, 4 * mw))]
    for n in range(g.log_size - 2):
        out.append((f"convs.{2 * n}", g.convs[2 * n], 2 * n + 2, (4 * 2 ** n * mh, 4 * 2 ** n * mw)))
        out.append((f"convs.{2 * n + 1}", g.convs[2 * n + 1], 2 * n + 3, (8 * 2 ** n * mh, 8 * 2 ** n * mw)))
    return out


SIZES = (8, 16, 32, 64, 128, 256, 512, 1024)


def reachable_modes(orient="square"):
    """{mode: [(size, cm, tag), ...]}: conv_mode of every layer of every supported generator (sizes 8 .. 1024, channel multipliers 1 and 2)
    of the orientation at the thresholds in force.  conv_mode does not look at the batch (1 and 8 give the same modes: asserted by the
    host test through the plan of the split-K kernels, which does not either)."""
    found = {}
    for size in SIZES:
        for cm in (1, 2):
            g = skeleton(size, cm)
            for tag, layer, _, (h, w) in layer_shapes(g, orient):
                found.setdefault(layer.conv.conv_mode(h, w), []).append((size, cm, tag))
    return found


def route_key(r):
    """What reachable_routes enumerates of a Route (the uint8 writer is a property of the forward, not of the layer's shape)."""
    return (r.mode, r.path, r.prescaled, r.posted, r.rgb, r.family)


def reachable_routes(batches=(1, 8)):
    """{orientation: {(mode, path, prescaled, posted, rgb, family): [(size, cm, batch, tag), ...]}} of expected_route over every supported
    generator (sizes 8 .. 1024, channel multipliers 1 and 2) at default switches, the non-square ones behind their layer-0 bend.  The
    batch enters through the split-K workspace only (maua_modconv_ws_floats: a layer that splits K folds no ToRGB): 1 and 8 are the ends."""
    found = {}
    for orient in ORIENTATIONS:
        here = found.setdefault(orient, {})
        for size in SIZES:
            for cm in (1, 2):
                g = skeleton(size, cm, output_size=OUTPUT_SIZE[orient])
                for batch in batches:
                    flags = dict(orient=orient, bends=() if orient == "square" else (0,))
                    for tag, r in expected_route(g, batch, flags).items():
                        here.setdefault(route_key(r), []).append((size, cm, batch, tag))
    return found


# ---- the route -------------------------------------------------------------------------------------------------------------------------------
@dataclasses.dataclass(frozen=True)
class Route:
    """What one layer of a forward did.  mode: conv_mode of its input shape.  path: StyledConv.last_path.  prescaled: its input arrived
    multiplied by its styles.  posted: it stored its map multiplied by the consumer's.  rgb: how the resolution's ToRGB ran — "folded"
    (in the convolution's epilogue), "partial" (partial sums left by the layer + the plane-sum pass), "separate" (a pass of its own over
    the feature map) or None (up-sampling layers; resolutions below min_rgb_size).  u8: on the last layer of a forward that delivers uint8
    frames, "layer" (written by its epilogue) or "pass" (maua_frames_to_u8); else None.  family: the kernel family of the convolution
    ("mfma": csrc/modconv.hip modes 0 - 4, "w2d": modconv_w2d.hip, "up2d": modconv_up2d.hip, "const": constconv.hip, no modconv launch)."""
    mode: int
    path: str
    prescaled: bool
    posted: bool
    rgb: str
    u8: str
    family: str


def _separable_4x4(k):
    k = k.double()
    if tuple(k.shape) != (4, 4) or float(k.sum()) == 0.0:
        return False
    return bool(torch.linalg.matrix_rank(k, tol=1e-9) == 1)


def _mfma_plan(lib_mod, batch, cin, cout, h, w, mode):
    """(BM, wave rows, several images per tile) of the csrc/modconv.hip instance for the shape, from the library's host-side plan."""
    rc, name = lib_mod.planned_modconv_instance(batch, cin, cout, h, w, mode)
    assert rc == 0, (rc, cin, cout, h, w, mode)
    args = [a.strip() for a in name[name.index("<") + 1: name.index(">")].split(",")]
    return int(args[0]), int(args[2]), args[4] == "true"


def expected_route(g, batch, flags=None):
    """{tag: Route} of one forward of ``g`` (a Generator on any device, the meta device included) at ``batch`` — the rules as README / DESIGN
    and the docstrings of models/stylegan2.py state them, layer by layer, without calling StyledConv.run.  ``flags``: acts
    (return_activation_maps), bends (layer ids that carry a bend), frames_u8, tap (Generator.tap_float_image), orient (the shape the
    layer-0 bend gives the constant: every rule looks at a layer's input rows and columns separately).  The generator's own switches
    (style_fold, disable_rgb_fusion, min_rgb_size) and the class thresholds are read where they live."""
    from maua_stylegan2_amd import _lib
    from maua_stylegan2_amd.models.stylegan2 import ConstantInput

    flags = dict(flags or {})
    bent = set(flags.get("bends", ()))
    acts, frames_u8, tap = bool(flags.get("acts")), bool(flags.get("frames_u8")), bool(flags.get("tap", g.tap_float_image))
    lib = _lib.load()
    fold = g.style_fold and not acts
    orient = flags.get("orient", "square")
    assert orient == "square" or 0 in bent, "a non-square forward has a bend on layer id 0"
    layers = layer_shapes(g, orient)
    route = {}

    def mode_of(idx):
        _, layer, _, (h, w) = layers[idx]
        return layer.conv.conv_mode(h, w)

    def wants_post(idx):
        """The layer at ``idx`` stores its map for the layer behind it pre-multiplied: fold on, no bend on its own id, and a consumer whose
        kernel has an instance without the style multiplies (modes 5 and 6)."""
        if idx + 1 >= len(layers) or not fold or layers[idx][2] in bent:
            return False
        return mode_of(idx + 1) in (5, 6)

    prescaled = False
    image_exists = False
    for idx, (tag, layer, layer_id, (h, w)) in enumerate(layers):
        conv = layer.conv
        cin, cout = conv.in_channel, conv.out_channel
        mode = mode_of(idx)
        is_last = idx == len(layers) - 1
        post = wants_post(idx)
        n_ws = lib.maua_modconv_ws_floats(batch, cin, cout, h, w, mode)
        family = {0: "mfma", 1: "mfma", 2: "mfma", 3: "mfma", 4: "mfma", 5: "w2d", 6: "up2d"}[mode]
        if conv.upsample:
            k = conv.blur.kernel
            low = layer.lowres_fusion and not prescaled and mode == 1 and lib.maua_lowres_ok(cin, cout, h, w, 1)
            if (layer.fused_blur_min_width <= w and mode == 6 and tuple(conv.blur.pad) == (1, 1) and _separable_4x4(k)
                    and lib.maua_upconv_blur_ok(cin, cout, h, w)):
                path = "fused"
            elif low and tuple(k.shape) == (4, 4) and tuple(conv.blur.pad) == (1, 1):
                path = "lowres"
                if layer.lowres_up2d and lib.maua_lowres_ok(cin, cout, h, w, 6):
                    family = "up2d"
            else:
                path = "pair"
            route[tag] = Route(mode, path, prescaled, post, None, None, family)
            prescaled = post
            continue
        # plain layers: conv1 and the second layer of every resolution
        wants_rgb = g.min_rgb_size <= min(h, w)  # (the resolution's nominal size: the short side)
        offer = wants_rgb and layer_id not in bent and not g.disable_rgb_fusion
        low = layer.lowres_fusion and not prescaled and mode in (0, 2, 3) and lib.maua_lowres_ok(cin, cout, h, w, mode)
        const = (idx == 0 and isinstance(g.input, ConstantInput) and layer.lowres_fusion and 0 not in bent
                 and lib.maua_const_conv_ok(cin, cout, 4, 4))
        single_tile = False  # the ToRGB-in-the-epilogue kernels: all channels of a pixel in one wave row of one workgroup, no split-K
        if offer and cout <= 64 and n_ws == 0:
            if mode == 5:
                single_tile = lib.maua_modconv_w2d_mtiles(cin, cout, h, w) == 1
            else:
                bm, wave_rows, multi = _mfma_plan(_lib, batch, cin, cout, h, w, mode)
                single_tile = cout <= bm and wave_rows == 1 and not multi
        posted = False
        if const:
            path, family, rgb = "const", "const", "partial" if offer else None
        elif single_tile:
            path, rgb, posted = "torgb", "folded", post and mode == 5
        elif (offer and cout > 64 and layer.partial_rgb_fusion and n_ws == 0 and mode == 5
              and lib.maua_modconv_w2d_mtiles(cin, cout, h, w) > 1):
            path, rgb, posted = "rgb_partial", "partial", post
        elif low and offer and layer.partial_rgb_fusion and w % 4 == 0 and not post:
            path, rgb = "lowres", "partial"
        else:
            path, rgb = "plain", None
        if rgb is None and wants_rgb:
            rgb = "separate"
        image_exists = image_exists or wants_rgb
        u8 = None
        if is_last and frames_u8 and image_exists:
            u8 = "layer" if path == "torgb" else "pass"
        route[tag] = Route(mode, path, prescaled, posted, rgb, u8, family)
        prescaled = posted
    return route


def route_flags(case):
    return dict(acts=case.acts, bends=tuple(layer for layer, _ in case.all_bends), frames_u8=case.u8 is not None, tap=bool(case.u8),
                orient=case.orient)


class switched:
    """Context: the case's class attributes (``cls``) set on StyledConv / ModulatedConv2d, restored on exit."""

    def __init__(self, case):
        self.case, self.keep = case, []

    def __enter__(self):
        from maua_stylegan2_amd.models import stylegan2 as sg

        for cls_name, attr, value in self.case.cls:
            cls = getattr(sg, cls_name)
            self.keep.append((cls, attr, cls.__dict__[attr]))
            setattr(cls, attr, value)
        return self

    def __exit__(self, *exc):
        for cls, attr, value in reversed(self.keep):
            setattr(cls, attr, value)
        return False


def case_skeleton(case):
    g = skeleton(case.size, case.cm, case.constant_input, case.min_rgb_size, blur_taps(case), case.output_size)
    for attr, value in case.gen:
        setattr(g, attr, value)
    return g


def case_route(case):
    """expected_route of the case on a weightless generator (host tests; the GPU test calls expected_route on the generator it runs)."""
    with switched(case):
        return expected_route(case_skeleton(case), case.batch, route_flags(case))
