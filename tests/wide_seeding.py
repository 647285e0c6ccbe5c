"""Seeded checkpoints and oracle forwards for generators built for 2:1 output (``Generator(..., output_size=1920 | 1080)``): their noise
buffers are [1, 1, r, 2r] (1920) or [1, 1, 2r, r] (1080), and a layer-0 bend widens the 4 x 4 constant accordingly."""
from collections import OrderedDict

import torch

from maua_stylegan2_amd import seeding


def noise_shapes(size, out_size):
    """(h, w) of every noise map of a ``size``-px generator built for ``out_size``."""
    mul_h, mul_w = (2 if out_size == 1080 else 1), (2 if out_size == 1920 else 1)
    return [(mul_h * r, mul_w * r) for r in seeding.noise_sizes(size)]


def wide_state_dict(size, out_size, seed, rgb_gain=1.0):
    """``seeding.seeded_state_dict`` with seeded 2:1 noise buffers: what ``Generator(size, ..., output_size=out_size)`` loads strictly."""
    sd = seeding.seeded_state_dict(size, seed=seed, rgb_gain=rgb_gain)
    for i, hw in enumerate(noise_shapes(size, out_size)):
        sd[f"noises.noise_{i}"] = torch.from_numpy(seeding.seeded_array(seed, f"noises.wide_{i}", (1, 1) + hw))
    return sd


def build_wide(size, out_size, sd, dev):
    from maua_stylegan2_amd.models.stylegan2 import Generator

    g = Generator(size, 512, 8, channel_multiplier=2, constant_input=True, output_size=out_size)
    g.load_state_dict(sd, strict=True)
    return g.to(dev).eval()


def oracle_forward(sd, latents, noise, bends):
    """``oracle.stylegan2_oracle.generator_forward`` on a wide checkpoint.  The oracle reads the generator's resolution off the WIDTH of
    the last ``noises.noise_*`` buffer, which a 2:1 buffer doubles: it is handed the weights with square placeholders of the true side, and
    every noise map explicitly (``noise[i]`` None: the checkpoint's 2:1 buffer), so the placeholders are never read."""
    from oracle import stylegan2_oracle as so

    n = sum(k.startswith("noises.noise_") for k in sd)
    maps = [sd[f"noises.noise_{i}"] if noise[i] is None else noise[i] for i in range(n)]
    told = OrderedDict(sd)
    for i in range(n):
        side = min(sd[f"noises.noise_{i}"].shape[-2:])
        told[f"noises.noise_{i}"] = torch.full((1, 1, side, side), float("nan"))
    return so.generator_forward(told, latents, maps, bends=bends)
