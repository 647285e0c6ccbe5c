"""Plugin for renders that leave TRAILS: the default plugin's latents and noise, with a frame feedback per frame on the device.

``initialize`` builds an ``ar.Feedback`` and leaves it in ``args.feedback``; the render feeds every frame's output back under the next
one (csrc/feedback.hip), in front of the lens, the grade and the quantiser.  One rank only: a recurrence cannot be sharded.

  * Mode ``max``: the brighter of the new frame and the trail wins, so the picture itself is never washed out.
  * Gain: ``ar.rms``, the level of the track; trails last HALF_LIFE[1] seconds when it is loud and HALF_LIFE[0] when it is quiet.
  * Zoom: the onsets below 150 Hz (``ar.onsets``); a kick pushes the old picture outward by up to KICK_ZOOM per frame: an echo tunnel opens
    on the hit and closes between hits.
  * Tint: a slow cosine between TINTS, so that old echoes drift in colour while the newest keeps the picture's own.
"""
import math

import torch

import maua_stylegan2_amd.audioreactive as ar
from maua_stylegan2_amd.audioreactive.examples import default

HALF_LIFE = (0.15, 0.6)  # seconds: quiet, loud
KICK_ZOOM = 0.04
DRIFT = 0.002  # zoom - 1 between hits: the trail creeps outward
ROTATE = 0.2  # degrees per frame
TINTS = ((1.0, 0.93, 0.86), (0.86, 0.93, 1.0))
TINT_PERIOD = 8.0  # seconds


def initialize(args):
    args = default.initialize(args)  # lo_onsets (<= 150 Hz), hi_onsets
    n = args.n_frames
    fps = n / float(args.duration)  # RENDERED frames a second: with --subframes the gain compounds per sub-frame
    kick = torch.as_tensor(ar.onsets(args.audio, args.sr, n, fmax=150, smooth=5, clip=97, power=2)).float().cpu().reshape(-1).clamp(0, 1)
    level = torch.as_tensor(ar.rms(args.audio, args.sr, n, smooth=10, clip=97, power=1)).float().cpu().reshape(-1).clamp(0, 1)
    half_life = HALF_LIFE[0] + (HALF_LIFE[1] - HALF_LIFE[0]) * level
    gain = 0.5 ** (1.0 / (half_life * fps))  # ar.Feedback.gain_for, per frame
    phase = 0.5 - 0.5 * torch.cos(2 * math.pi * torch.arange(n) / (TINT_PERIOD * fps))
    warm, cool = (torch.tensor(t) for t in TINTS)
    tint = warm[None] + (cool - warm)[None] * phase[:, None]
    args.feedback = ar.Feedback(n, gain=gain, zoom=1.0 + DRIFT + KICK_ZOOM * kick, rotate=ROTATE, tint=tint, mode="max", border="mirror")
    return args


get_latents = default.get_latents
get_noise = default.get_noise
