"""Plugin for "liquid" renders: the coordinate-remap bends driven by the audio, all inside the captured forward.

Latents and noise are the default plugin's.  ``get_bends`` adds three bends:
  * an ``ar.Displace`` on the 32-px maps whose flow field is a looping Perlin noise bank — the loudness (RMS) sets how far the features
    are pushed along the flow, and the bass onsets speed the loop up (the loop position is the cumulative sum of a per-frame speed;
    fractional positions blend neighbouring frames of the bank);
  * an ``ar.Swirl`` on every other channel of the 16-px maps, twisted by the treble onsets;
  * an ``ar.Kaleidoscope`` on the 64-px maps whose content rotates with the loudness.
Every per-frame quantity travels in the bends' ``modulation`` (a sharded job cuts exactly that to a rank's frames); the flow field and the
channel list are static.  All three transforms implement ``run_static``, so the render stays on the hipGraph lanes.
"""
import torch

import maua_stylegan2_amd.audioreactive as ar
from maua_stylegan2_amd.audioreactive.examples import default
from maua_stylegan2_amd.audioreactive.examples.default import get_latents, get_noise  # noqa: F401

LIQUID_LAYER, SWIRL_LAYER, KALEIDOSCOPE_LAYER = 6, 4, 8   # layer ids: 32-px, 16-px and 64-px feature maps
FIELD_FRAMES, FIELD_SIZE, FIELD_RES = 64, 32, (8, 4, 4)  # a loop of 64 flow fields of 32 x 32 with a 4 x 4 Perlin lattice
AMPLITUDE = 3.0            # pixels of the 32-px map per unit of the (unit-variance) flow at full loudness
BASE_SPEED, ONSET_SPEED = 0.25, 1.5   # bank frames per video frame: at rest, and added at a full bass onset
SWIRL_DEGREES, SWIRL_RADIUS = 120.0, 5.0
SWIRL_CHANNELS = range(0, 512, 2)
SECTORS, ROTATION_DEGREES = 6, 90.0


def initialize(args):
    args = default.initialize(args)
    args.rms = ar.rms(args.audio, args.sr, args.n_frames, smooth=10, clip=50, power=1)
    return args


def flow_field():
    """[FIELD_FRAMES, 2, FIELD_SIZE, FIELD_SIZE]: two independent Perlin loops (tileable in time) as the dx and the dy planes."""
    planes = [ar.perlin_noise((FIELD_FRAMES, FIELD_SIZE, FIELD_SIZE), FIELD_RES, tileable=(True, False, False)) for _ in range(2)]
    field = torch.stack(planes, 1)
    return field / field.std()


def get_bends(args):
    rms, bass, treble = (torch.as_tensor(v).float().cpu() for v in (args.rms, args.lo_onsets, args.hi_onsets))
    field = flow_field()
    position = torch.cumsum(BASE_SPEED + ONSET_SPEED * bass, 0)
    liquid = torch.stack([AMPLITUDE * (0.25 + 0.75 * rms), position], 1)  # columns: amplitude, loop position
    channels = list(SWIRL_CHANNELS)
    return [
        {"layer": LIQUID_LAYER, "modulation": liquid, "transform": lambda m: ar.Displace(m, field)},
        {"layer": SWIRL_LAYER, "modulation": SWIRL_DEGREES * treble,
         "transform": lambda m: ar.Swirl(m, radius=SWIRL_RADIUS, channels=channels)},
        {"layer": KALEIDOSCOPE_LAYER, "modulation": ROTATION_DEGREES * rms, "transform": lambda m: ar.Kaleidoscope(m, sectors=SECTORS)},
    ]
