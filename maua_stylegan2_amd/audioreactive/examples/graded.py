"""Plugin for renders whose COLOUR follows the music: the default plugin's latents and noise, graded per frame on the device.

``initialize`` builds an ``ar.Grade`` and leaves it in ``args.grade``; the render applies its row to every frame's fp32 image, in front of
the 8-, 10- or 16-bit quantiser (csrc/grade.hip), so a flash has the generator's whole range to work with.

  * Exposure: the onsets below 150 Hz, up to +0.8 stops on a kick, back to neutral between hits.
  * Saturation: ``ar.rms``, the level of the track, from 0.85 (quiet) to 1.35 (loud).
  * Hue: the strongest ``ar.chroma`` class per frame, smoothed over about two seconds, turns the hue by up to +-25 degrees.

Frames whose row is neutral leave the device exactly as the ungraded render delivers them.  A film look on top: ``--grade_lut look.cube``.
"""
import torch

import maua_stylegan2_amd.audioreactive as ar
from maua_stylegan2_amd.audioreactive.examples import default

FLASH_STOPS = 0.8
SATURATION = (0.85, 1.35)
HUE_DEGREES = 25.0
HUE_SMOOTH = 60  # frames at 30 fps


def initialize(args):
    args = default.initialize(args)  # lo_onsets (<= 150 Hz), hi_onsets
    kick = torch.as_tensor(args.lo_onsets).float().cpu()
    level = ar.rms(args.audio, args.sr, args.n_frames, smooth=10, clip=97, power=1).float().cpu()
    chroma = ar.chroma(args.audio, args.sr, args.n_frames).float().cpu()
    # the strongest pitch class as an angle on the circle of its index, smoothed as a vector so that it cannot jump through the wrap
    angle = chroma.argmax(1).float() * (2 * torch.pi / chroma.shape[1])
    circle = ar.gaussian_filter(torch.stack([angle.cos(), angle.sin()], 1), HUE_SMOOTH).cpu()
    hue = HUE_DEGREES * torch.sin(torch.atan2(circle[:, 1], circle[:, 0]))
    args.grade = ar.Grade(args.n_frames, exposure=FLASH_STOPS * kick.clamp(0, 1),
                          saturation=SATURATION[0] + (SATURATION[1] - SATURATION[0]) * level.clamp(0, 1), hue=hue)
    return args


get_latents = default.get_latents
get_noise = default.get_noise
