"""Audio-reactive lens effects (no counterpart in the reference): ``ar.Lens`` builds the per-frame row table and the Gaussian tap tables
that csrc/lens.hip applies to the generator's fp32 image — bloom, sharpen / soften, vignette —, in front of the grade and of every
quantiser (render.lens_frames / render.render_lensed; a plugin hands it over as ``args.lens``).

A row is 16 float32 (include/maua_hip.h, maua_lens_apply_f32): threshold, knee, bloom_rgb[3] (gain x tint), sharpen, vignette, vig_inner,
vig_outer, reserved[7].  Per frame the device extracts the soft-knee highlights, averages them over d x d blocks, blurs that map with the
frame's Gaussian, blurs the image with the sharpen's short Gaussian, and writes  y = x + sharpen (x - soft) + 2 bloom_rgb up(bloom),
darkened towards the corners by the vignette.  A row with bloom 0, sharpen 0 and vignette 0 passes its frame through bit for bit.

The plan rule (the maxima are taken over the rows of the WHOLE JOB's table that have a bloom, or a sharpen — ``plan_max``,
which slices and the blocks of a sharded job keep): sigma_px = bloom_size * h; d is the smallest of 1, 2, 4, 8 with max sigma_px / d <= 6, else 8; radius =
ceil(3 max sigma_px / d), refused above 64; taps exp(-k^2 / (2 (sigma_px / d)^2)) in float64, normalised to w[0] + 2 sum w[k] = 1, cast to
float32; sigma 0 is the delta.  The sharpen's taps likewise with d = 1 and sigma = sharpen_radius, refused above 8 px.
"""
import math

import numpy as np
import torch as th

from . import frame_table
from .frame_table import FrameTable, collect, host64

__all__ = ["Lens", "LENS_ROW"]

LENS_ROW = 16
_THRESHOLD, _KNEE, _BLOOM, _SHARPEN, _VIGNETTE, _INNER, _OUTER = 0, 1, 2, 5, 6, 7, 8
REDUCTIONS = (1, 2, 4, 8)
SIGMA_PER_REDUCTION = 6.0
MAX_RADIUS = 64
MAX_SHARPEN_SIGMA = 8.0


def plan_reduction(sigma_max):
    """The reduction d of a bloom whose widest Gaussian has ``sigma_max`` pixels: the smallest of 1, 2, 4, 8 with sigma_max / d <= 6, else 8."""
    for d in REDUCTIONS:
        if sigma_max / d <= SIGMA_PER_REDUCTION:
            return d
    return REDUCTIONS[-1]


def gaussian_taps(sigmas, radius):
    """float32 [n, radius + 1] half-kernels, w[0] the centre: exp(-k^2 / (2 sigma^2)) in float64, normalised so that w[0] + 2 sum w[k] = 1;
    a sigma of 0 gives the delta."""
    sigmas = np.atleast_1d(np.asarray(sigmas, np.float64))
    k = np.arange(radius + 1, dtype=np.float64)
    out = np.zeros((len(sigmas), radius + 1), np.float64)
    for i, s in enumerate(sigmas):
        if s == 0:
            out[i, 0] = 1.0
            continue
        g = np.exp(-k * k / (2.0 * s * s))
        out[i] = g / (g[0] + 2.0 * g[1:].sum())
    return out.astype(np.float32)


class Lens(FrameTable):
    """Lens effects: one parameter row per rendered frame, or one row for all of them.

    Every argument is a scalar or a per-frame sequence — [n_frames] or [n_frames, 1]; the tint a triple (R, G, B) or [n_frames, 3]; torch
    or numpy, host or device.  ``n_frames`` None: the length of the sequences (they must agree), one row without any.

      bloom            gain of the glow added to the image (>= 0); 0 switches it off
      bloom_size       the Gaussian's sigma as a FRACTION OF THE FRAME'S HEIGHT (>= 0): one plugin serves 256^2 and 1024^2 checkpoints
      bloom_threshold  display-range level (0 .. 1) above which a pixel glows;  bloom_knee (>= 0): half-width of the soft transition
      bloom_tint       colour of the glow, folded with the gain into the row
      sharpen          amount of unsharp masking, y = x + sharpen (x - blur(x)); negative softens
      sharpen_radius   sigma of that blur in pixels (0 .. 8)
      vignette         strength: the corners are scaled by 1 - vignette (in display range)
      vignette_inner / vignette_outer   radii (corner = 1) between which the smoothstep falls; outer > inner

    Refused: non-finite values, bloom < 0, knee < 0, a threshold outside [0, 1], negative sizes, outer <= inner, sequences of different
    lengths.  The device checks none of this."""

    def __init__(self, n_frames=None, *, bloom=0, bloom_size=0.02, bloom_threshold=0.7, bloom_knee=0.1, bloom_tint=(1, 1, 1), sharpen=0,
                 sharpen_radius=1.0, vignette=0, vignette_inner=0.5, vignette_outer=1.0):
        n, (bloom, size, threshold, knee, tint, sharpen, radius, vignette, inner, outer) = collect("Lens", n_frames, [
            ("bloom", bloom, 1, False), ("bloom_size", bloom_size, 1, False), ("bloom_threshold", bloom_threshold, 1, False),
            ("bloom_knee", bloom_knee, 1, False), ("bloom_tint", bloom_tint, 3, False), ("sharpen", sharpen, 1, False),
            ("sharpen_radius", sharpen_radius, 1, False), ("vignette", vignette, 1, False), ("vignette_inner", vignette_inner, 1, False),
            ("vignette_outer", vignette_outer, 1, False)])
        if np.any(bloom < 0):
            raise ValueError("Lens: bloom must not be negative")
        if np.any(knee < 0):
            raise ValueError("Lens: bloom_knee must not be negative")
        if np.any(threshold < 0) or np.any(threshold > 1):
            raise ValueError("Lens: bloom_threshold must lie in [0, 1]")
        if np.any(size < 0) or np.any(radius < 0):
            raise ValueError("Lens: bloom_size and sharpen_radius must not be negative")
        rows = np.zeros((n, LENS_ROW), np.float64)
        rows[:, _THRESHOLD], rows[:, _KNEE] = threshold[:, 0], knee[:, 0]
        rows[:, _BLOOM:_BLOOM + 3] = bloom * tint
        rows[:, _SHARPEN], rows[:, _VIGNETTE] = sharpen[:, 0], vignette[:, 0]
        rows[:, _INNER], rows[:, _OUTER] = inner[:, 0], outer[:, 0]
        with np.errstate(over="ignore"):
            table = rows.astype(np.float32)
        self._init(table, np.broadcast_to(size[:, 0], (n,)).copy(), np.broadcast_to(radius[:, 0], (n,)).copy())

    def _init(self, table, bloom_size, sharpen_sigma, plan_max=None):
        if not np.all(np.isfinite(table)):
            raise ValueError("Lens: the parameters overflow float32 or are not finite")
        if np.any(table[:, _OUTER] <= table[:, _INNER]):
            raise ValueError("Lens: vignette_outer must be greater than vignette_inner")
        if np.any(sharpen_sigma > MAX_SHARPEN_SIGMA):
            raise ValueError(f"Lens: a sharpen_radius of {float(sharpen_sigma.max()):g} px is refused: the sharpen's Gaussian is a short one "
                             f"(sigma <= {MAX_SHARPEN_SIGMA:g} px); a wide soft glow is what bloom is for")
        self.table = table
        self.bloom_size = bloom_size
        self.sharpen_sigma = sharpen_sigma
        for a in (self.table, self.bloom_size, self.sharpen_sigma):
            a.setflags(write=False)
        self.identity = (table[:, _BLOOM:_BLOOM + 3] == 0).all(axis=1) & (table[:, _SHARPEN] == 0) & (table[:, _VIGNETTE] == 0)
        # what the plan rule takes its maxima over: the largest bloom_size among the rows that have a bloom and the largest sharpen sigma
        # among the rows that have a sharpen (0 without any) — of the WHOLE JOB's table: a slice keeps the table's pair, so that every
        # rank of a sharded job derives the reduction, the radii and the taps the one-rank job derives
        blooming, sharpening = (table[:, _BLOOM:_BLOOM + 3] != 0).any(axis=1), table[:, _SHARPEN] != 0
        own = (float(bloom_size[blooming].max()) if blooming.any() else 0.0, float(sharpen_sigma[sharpening].max()) if sharpening.any() else 0.0)
        if plan_max is None:
            plan_max = own
        else:
            plan_max = (float(plan_max[0]), float(plan_max[1]))
            if not all(math.isfinite(v) for v in plan_max) or plan_max[0] < own[0] or plan_max[1] < own[1] or plan_max[1] > MAX_SHARPEN_SIGMA:
                raise ValueError(f"Lens: plan_max {plan_max} must be finite, at least this table's own maxima {own} and at most "
                                 f"{MAX_SHARPEN_SIGMA:g} px for the sharpen")
        self.plan_max = plan_max
        self._device = {}

    @classmethod
    def from_tables(cls, table, bloom_size, sharpen_sigma, plan_max=None):
        """A lens from a finished row table [n, 16] and its per-row bloom sizes and sharpen sigmas [n] (validated as the constructor does).
        ``plan_max``: the (bloom_size, sharpen sigma) maxima the plan rule uses when the table is a block of a longer one (``.plan_max`` of
        the whole table); None: this table's own."""
        table = np.array(host64(table), np.float32)
        size, sigma = np.array(host64(bloom_size), np.float64).reshape(-1), np.array(host64(sharpen_sigma), np.float64).reshape(-1)
        if table.ndim != 2 or table.shape[1] != LENS_ROW or table.shape[0] < 1:
            raise ValueError(f"Lens.from_tables: the table must be [n, {LENS_ROW}], got {table.shape}")
        if size.shape != (table.shape[0],) or sigma.shape != (table.shape[0],):
            raise ValueError(f"Lens.from_tables: {table.shape[0]} rows need as many bloom sizes and sharpen sigmas, got {size.shape[0]} and {sigma.shape[0]}")
        if not (np.all(np.isfinite(size)) and np.all(np.isfinite(sigma))) or np.any(size < 0) or np.any(sigma < 0):
            raise ValueError("Lens.from_tables: the sizes must be finite and not negative")
        if not np.all(np.isfinite(table)):
            raise ValueError("Lens.from_tables: the table holds non-finite values")
        if np.any(table[:, _BLOOM:_BLOOM + 3] < 0) or np.any(table[:, _KNEE] < 0) or np.any(table[:, _THRESHOLD] < 0) or np.any(table[:, _THRESHOLD] > 1):
            raise ValueError("Lens.from_tables: bloom and knee must not be negative, the threshold lies in [0, 1]")
        self = cls.__new__(cls)
        self._init(table, size, sigma, plan_max)
        return self

    @property
    def has_bloom(self):
        return bool((self.table[:, _BLOOM:_BLOOM + 3] != 0).any())

    @property
    def has_sharpen(self):
        return bool((self.table[:, _SHARPEN] != 0).any())

    def __repr__(self):
        return f"Lens({self._count()}, bloom={self.has_bloom}, sharpen={self.has_sharpen}, identity={int(self.identity.sum())})"

    def plan(self, h, w):
        """(d, bloom radius, bloom taps [n, radius + 1], sharpen radius, sharpen taps) on the host for frames of h x w (the plan rule).  The
        maxima are ``plan_max``: those of the rows that have a bloom (a sharpen) in the whole job's table — a lens without a bloom plans
        d = 1 and radius 0 whatever its bloom_size says, and a block of a sharded table plans as the table does."""
        if h < 1 or w < 1:
            raise ValueError(f"Lens.plan: a frame of {h} x {w}")
        sigma_max = self.plan_max[0] * float(h)
        d = plan_reduction(sigma_max)
        rb = int(math.ceil(3.0 * sigma_max / d))
        if rb > MAX_RADIUS:
            raise ValueError(f"Lens: a bloom_size of {self.plan_max[0]:g} on frames {h} px high is a Gaussian of sigma {sigma_max:.1f} px: "
                             f"at the coarsest reduction ({d}) its radius is {rb} taps, the device kernel serves {MAX_RADIUS} "
                             f"(bloom_size <= {MAX_RADIUS * d / 3.0 / h:.3f} at this height)")
        rs = int(math.ceil(3.0 * self.plan_max[1]))
        return d, rb, gaussian_taps(self.bloom_size * float(h) / d, rb), rs, gaussian_taps(self.sharpen_sigma, rs)

    def operands(self, device, h, w):
        """(rows [n, 16], d, bloom radius, bloom taps [n, radius + 1], sharpen radius, sharpen taps [n, radius + 1]) as float32 tensors on
        ``device`` for frames of h x w (computed and uploaded once per device and size)."""
        device = th.device(device)
        key = (str(device), int(h), int(w))
        if key not in self._device:
            d, rb, bt, rs, st = self.plan(int(h), int(w))
            up = lambda a: th.from_numpy(np.array(a)).to(device)
            self._device[key] = (up(self.table), d, rb, up(bt), rs, up(st))
        return self._device[key]

    def tables(self):
        """(table, bloom_size, sharpen_sigma, plan_max): ``Lens.from_tables(*x.tables())`` is x, planned as x is."""
        return self.table, self.bloom_size, self.sharpen_sigma, self.plan_max

    def _block(self, lo, hi):
        return Lens.from_tables(self.table[lo:hi], self.bloom_size[lo:hi], self.sharpen_sigma[lo:hi], self.plan_max)  # (plans as this table does)


SPEC_KEYS = ("bloom", "bloom_size", "bloom_threshold", "bloom_knee", "bloom_tint", "sharpen", "sharpen_radius", "vignette", "vignette_inner",
             "vignette_outer")


def parse_spec(text):
    """A static lens as text, ``"bloom=0.8,bloom_size=0.03,sharpen=0.4,vignette=0.3"`` (the --lens flag), -> the keyword arguments of Lens.
    Keys: SPEC_KEYS; a value is a number, bloom_tint three numbers joined by ``:`` (``bloom_tint=1:0.8:0.6``)."""
    return frame_table.parse_spec("--lens", text, {k: (3,) if k == "bloom_tint" else (1,) for k in SPEC_KEYS})
