"""Plugin for renders whose LIGHT follows the music: the default plugin's latents and noise, with a lens per frame on the device.

``initialize`` builds an ``ar.Lens`` and leaves it in ``args.lens``; the render passes every frame's fp32 image through it, in front of the
grade and of the 8-, 10- or 16-bit quantiser (csrc/lens.hip), so the glow keeps the highlights the generator computed beyond the display
range.

  * Bloom: the onsets below 150 Hz; the highlights spread into a warm glow of up to BLOOM on a kick, none between hits.
  * Vignette: ``ar.rms``, the level of the track; the corners close in when it is quiet (VIGNETTE[0]) and open when it is loud (VIGNETTE[1]).
  * Sharpen: a constant light unsharp mask, chiefly for checkpoints delivered above their size (--deliver_size).

Frames whose row is neutral leave the device exactly as the plain render delivers them.
"""
import torch

import maua_stylegan2_amd.audioreactive as ar
from maua_stylegan2_amd.audioreactive.examples import default

BLOOM = 0.9
BLOOM_SIZE = 0.025  # sigma, as a fraction of the frame's height
BLOOM_TINT = (1.0, 0.85, 0.7)
VIGNETTE = (0.45, 0.1)
SHARPEN = 0.0


def initialize(args):
    args = default.initialize(args)  # lo_onsets (<= 150 Hz), hi_onsets
    kick = torch.as_tensor(args.lo_onsets).float().cpu().reshape(-1)
    level = ar.rms(args.audio, args.sr, args.n_frames, smooth=10, clip=97, power=1).float().cpu().reshape(-1)
    args.lens = ar.Lens(args.n_frames, bloom=BLOOM * kick.clamp(0, 1), bloom_size=BLOOM_SIZE, bloom_threshold=0.6, bloom_knee=0.15,
                        bloom_tint=BLOOM_TINT, sharpen=SHARPEN, vignette=VIGNETTE[0] + (VIGNETTE[1] - VIGNETTE[0]) * level.clamp(0, 1))
    return args


get_latents = default.get_latents
get_noise = default.get_noise
