"""Plugin for renders that move with the bar: ``examples/onbeat.py`` with the bar found instead of assumed — ``ar.bar_phase``,
``ar.bar_beats`` and ``ar.beat_phase(method="bar")`` from one bar-pointer decode, so a waltz loops in three and a march in four.

  * Latents: every beat of the bar has its own latent (``ar.bar_beats`` rows weight the first ``metre`` entries of the selection), and
    the rest of the selection is walked as a loop whose position is ``ar.bar_phase``: it closes on the downbeat in any metre and
    follows tempo changes without a loop count.
  * Bends: an ``ar.Swirl`` on every other channel of the 16-px maps whose angle is ``(1 - beat_phase) ** 4`` — a kick on every beat,
    stronger on beat 0 of the bar.  The transform implements ``run_static``, so the render stays on the hipGraph lanes.
  * Noise: the default plugin's fast and slow fields, cross-faded by the same kick.
"""
import torch

import maua_stylegan2_amd.audioreactive as ar
from maua_stylegan2_amd.audioreactive.examples import default

SWIRL_LAYER = 4            # layer id of the 16-px feature maps
SWIRL_DEGREES, SWIRL_RADIUS = 120.0, 5.0
SWIRL_CHANNELS = range(0, 512, 2)
OFFBEAT_KICK = 0.5         # the kick of the beats that are not the downbeat, relative to it
BEAT_MIX = 0.5             # how much of a frame's latent is its beat's own, the rest is the loop through the bar
BEAT_SMOOTH = 2            # video frames of Gaussian smoothing on the beat rows


def initialize(args):
    args.beat = ar.beat_phase(args.audio, args.sr, args.n_frames, method="bar")
    args.bar = ar.bar_phase(args.audio, args.sr, args.n_frames)
    args.rows = ar.bar_beats(args.audio, args.sr, args.n_frames, smooth=BEAT_SMOOTH)
    args.metre = args.rows.shape[1]
    on_downbeat = ar.bar_beats(args.audio, args.sr, args.n_frames)[:, 0]
    args.kick = (1 - args.beat) ** 4 * (OFFBEAT_KICK + (1 - OFFBEAT_KICK) * on_downbeat)
    return args


def get_latents(selection, args):
    """The beat's own latent (the first ``metre`` entries of the selection) mixed with the selection walked as a closed loop, linearly
    interpolated at the loop position ``args.bar`` in [0, 1)."""
    n = selection.shape[0]
    pos = args.bar.to(selection.device) * n
    lo = pos.floor().long() % n
    frac = (pos - pos.floor())[:, None, None].to(selection.dtype)
    loop = selection[lo] * (1 - frac) + selection[(lo + 1) % n] * frac
    rows = args.rows / args.rows.sum(1, keepdim=True).clamp(min=1e-6)
    own = ar.chroma_weight_latents(rows, selection[torch.arange(args.metre) % n])
    return ar.gaussian_filter(BEAT_MIX * own + (1 - BEAT_MIX) * loop, 1)


def get_bends(args):
    channels = list(SWIRL_CHANNELS)
    return [{"layer": SWIRL_LAYER, "modulation": SWIRL_DEGREES * torch.as_tensor(args.kick).float().cpu(),
             "transform": lambda m: ar.Swirl(m, radius=SWIRL_RADIUS, channels=channels)}]


def get_noise(height, width, scale, num_scales, args):
    if width > default.NOISE_MAX_WIDTH:
        return None
    beat = args.kick[:, None, None, None].cuda()
    jittery = default._filtered_field(args.n_frames, height, width, default.FAST_SIGMA)
    field = default._crossfade(beat, jittery, default._filtered_field(args.n_frames, height, width, default.SLOW_SIGMA))
    return field / (field.std() * 2.5)
