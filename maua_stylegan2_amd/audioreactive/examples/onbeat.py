"""Plugin for renders that move on the beat: ``ar.beat_phase`` and ``ar.pulse`` instead of band-limited onsets and hand-tuned loop counts.

  * Bends: an ``ar.Swirl`` on every other channel of the 16-px maps whose angle is ``(1 - beat_phase) ** 4`` — a kick on every beat
    that has died away before the next one, whatever the tempo does.  The transform implements ``run_static``, so the render stays on
    the hipGraph lanes.
  * Latents: the selection is walked as a loop that comes round once per four beats: ``ar.beat_phase(division=0.25)`` is the loop
    position, so the loop follows tempo changes without a loop count.
  * Noise: the default plugin's fast and slow fields, cross-faded by ``ar.pulse`` (the pulse curve itself: near 1 on the beat).
"""
import torch

import maua_stylegan2_amd.audioreactive as ar
from maua_stylegan2_amd.audioreactive.examples import default

SWIRL_LAYER = 4            # layer id of the 16-px feature maps
SWIRL_DEGREES, SWIRL_RADIUS = 120.0, 5.0
SWIRL_CHANNELS = range(0, 512, 2)
BEATS_PER_LOOP = 4


def initialize(args):
    args.beat = ar.beat_phase(args.audio, args.sr, args.n_frames)
    args.bar = ar.beat_phase(args.audio, args.sr, args.n_frames, division=1.0 / BEATS_PER_LOOP)
    args.pulse = ar.pulse(args.audio, args.sr, args.n_frames, power=2)
    args.kick = (1 - args.beat) ** 4
    return args


def get_latents(selection, args):
    """The selection as a closed loop, linearly interpolated at the loop position ``args.bar`` in [0, 1)."""
    n = selection.shape[0]
    pos = args.bar.to(selection.device) * n
    lo = pos.floor().long() % n
    frac = (pos - pos.floor())[:, None, None].to(selection.dtype)
    latents = selection[lo] * (1 - frac) + selection[(lo + 1) % n] * frac
    return ar.gaussian_filter(latents, 1)


def get_bends(args):
    channels = list(SWIRL_CHANNELS)
    return [{"layer": SWIRL_LAYER, "modulation": SWIRL_DEGREES * torch.as_tensor(args.kick).float().cpu(),
             "transform": lambda m: ar.Swirl(m, radius=SWIRL_RADIUS, channels=channels)}]


def get_noise(height, width, scale, num_scales, args):
    if width > default.NOISE_MAX_WIDTH:
        return None
    beat = args.pulse[:, None, None, None].cuda()
    jittery = default._filtered_field(args.n_frames, height, width, default.FAST_SIGMA)
    field = default._crossfade(beat, jittery, default._filtered_field(args.n_frames, height, width, default.SLOW_SIGMA))
    return field / (field.std() * 2.5)
