"""Plugin for renders that follow the levels of four frequency bands — "bass / mids / highs" with a fast attack and a slow release.

``ar.bands`` filters the track through a Butterworth bank on the device (20-150, 150-600, 600-2500, 2500-8000 Hz), takes the level of
every band per video frame and runs it through an attack / release follower: a kick drum opens its envelope at once and lets it fall over
a third of a second, where an onset envelope would only mark the hit.

  * Bends: the bass band twists the 16-px feature maps (``ar.Swirl`` on every other channel, inside the captured forward).
  * Latents: the two mid bands weight entries 1 and 2 of the selection against entry 0, which holds while the mids are quiet.
  * Noise: a fast and a slow field cross-faded by the top band — per-frame fields up to 256 px, an ``ar.NoiseSynth`` recipe of two loops
    above (the 512^2 / 1024^2 layers), as in examples/hires_noise.py.
"""
import torch

import maua_stylegan2_amd.audioreactive as ar
from maua_stylegan2_amd.audioreactive.examples import default
from maua_stylegan2_amd.audioreactive.examples.hires_noise import LOOP_FRAMES, _loop

EDGES = (20, 150, 600, 2500, 8000)
ATTACK, RELEASE = 0, 8  # video frames at 30 fps
SWIRL_LAYER, SWIRL_DEGREES, SWIRL_RADIUS = 4, 90.0, 5.0
SWIRL_CHANNELS = range(0, 512, 2)
LATENT_SMOOTH = 2


def initialize(args):
    args.bands = ar.bands(args.audio, args.sr, args.n_frames, edges=EDGES, attack=ATTACK, release=RELEASE)
    args.bass, args.top = args.bands[:, 0].contiguous(), args.bands[:, -1].contiguous()
    return args


def get_latents(selection, args):
    if selection.shape[0] < 3:
        raise ValueError(f"examples/bands.py blends three latents: the selection needs 3 entries (got {selection.shape[0]})")
    mids = args.bands[:, 1:3].to(selection.device, selection.dtype)
    rest = (1 - mids.sum(1, keepdim=True)).clamp(min=0)
    weights = torch.cat([rest, mids], 1)
    weights = weights / weights.sum(1, keepdim=True)
    return ar.gaussian_filter(ar.chroma_weight_latents(weights, selection[:3]), LATENT_SMOOTH)


def get_noise(height, width, scale, num_scales, args):
    top = args.top.to("cuda", torch.float32)
    if width <= default.NOISE_MAX_WIDTH:
        jittery = default._filtered_field(args.n_frames, height, width, default.FAST_SIGMA)
        field = default._crossfade(top[:, None, None, None], jittery, default._filtered_field(args.n_frames, height, width, default.SLOW_SIGMA))
        return field / (field.std() * 2.5)
    period = min(LOOP_FRAMES, args.n_frames)
    jittery = _loop(period, height, width, default.FAST_SIGMA)
    slow = _loop(period, height, width, min(default.SLOW_SIGMA, max(period / 8, 1)))
    recipe = ar.NoiseSynth(height, width, [ar.noise_term(jittery, envelope=top), ar.noise_term(slow, envelope=1 - top)])
    return recipe.with_gain(1 / (2.5 * float(recipe.std())))


def get_bends(args):
    bass = torch.as_tensor(args.bass).float().cpu()
    channels = list(SWIRL_CHANNELS)
    return [{"layer": SWIRL_LAYER, "modulation": SWIRL_DEGREES * bass, "transform": lambda m: ar.Swirl(m, radius=SWIRL_RADIUS, channels=channels)}]
