"""Plugin for 2:1 renders: ``--out_size 1920`` (landscape) and ``--out_size 1080`` (portrait) without writing a plugin.

Latents and noise are the default plugin's.  ``get_bends`` adds the one transform a StyleGAN2 generator needs to produce 2:1 frames: a
static bend on layer id 0 that repeats the learned 4 x 4 constant outwards to 4 x 8 (8 x 4 for portrait) and adds a little static noise
that disguises the repetition — the examples' ``Sequential(ReplicationPad2d((2, 2, 0, 0)), AddNoise(...))`` expressed as ``ar.Pad``, which
runs inside the captured forward, so the render stays on the hipGraph lanes.  The noise maps ``get_noise`` is asked for are 2:1 already
(generate() doubles the long side for these output sizes) and match the 2:1 layers.
"""
import torch

import maua_stylegan2_amd.audioreactive as ar
from maua_stylegan2_amd.audioreactive.examples.default import get_latents, get_noise, initialize  # noqa: F401

PADS = {1920: (2, 2, 0, 0), 1080: (0, 0, 2, 2)}  # (left, right, top, bottom) on the 4 x 4 constant
NOISE_AMPLITUDE = 0.025
NOISE_SEED = 0


def get_bends(args):
    out_size = getattr(args, "out_size", None)
    if out_size not in PADS:
        raise ValueError(f"the wide plugin renders --out_size 1920 or 1080 (got {out_size})")
    left, right, top, bottom = PADS[out_size]
    # a generator of its own: the plane is the same on every rank of a sharded job and leaves the global random stream alone
    rng = torch.Generator().manual_seed(NOISE_SEED)
    noise = NOISE_AMPLITUDE * torch.randn((1, 1, 4 + top + bottom, 4 + left + right), generator=rng)
    return [{"layer": 0, "transform": ar.Pad(PADS[out_size], mode="replicate", noise=noise)}]
