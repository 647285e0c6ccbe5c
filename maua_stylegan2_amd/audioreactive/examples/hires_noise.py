"""The default plugin with audio-reactive noise on EVERY scale, the 512^2 and 1024^2 layers included.

Latents and the noise of the scales up to 256 px are the default plugin's.  Above, a per-frame ``[n_frames, 1, h, w]`` field no longer
fits (4 MB per frame and slot at 1024^2), so ``get_noise`` returns an ``ar.NoiseSynth`` recipe instead: two circularly filtered loops of
``LOOP_FRAMES`` frames, one fast and one slow, cross-faded by the same onset envelopes.  The default's cross-fade chain is linear in its two
fields, so it is two terms with one envelope each; the generator evaluates them per batch inside its captured forward.
"""
import torch

import maua_stylegan2_amd.audioreactive as ar
from maua_stylegan2_amd.audioreactive.examples import default
from maua_stylegan2_amd.audioreactive.examples.default import FAST_SIGMA, NOISE_MAX_WIDTH, SLOW_SIGMA, get_latents, initialize  # noqa: F401

LOOP_FRAMES = 240  # period of the two loops (8 s at 30 fps); a clip shorter than that is its own period


def _loop(period, height, width, sigma):
    """``ar.gaussian_filter`` is circular in time: a filtered random field IS a seamless loop of its length."""
    return ar.gaussian_filter(torch.randn((period, 1, height, width), device="cuda"), sigma)


def get_noise(height, width, scale, num_scales, args):
    if width <= NOISE_MAX_WIDTH:
        return default.get_noise(height, width, scale, num_scales, args)
    period = min(LOOP_FRAMES, args.n_frames)
    jittery = _loop(period, height, width, FAST_SIGMA)
    # (the filter wraps around while its radius, 4 sigma at 30 fps, stays inside the loop: the slow field's sigma is capped at period / 8)
    slow = _loop(period, height, width, min(SLOW_SIGMA, max(period / 8, 1)))
    # default.get_noise's chain  field = slow;  field = e * jittery + (1 - e) * field  per band, as coefficients of the two fields
    on_jittery = torch.zeros(args.n_frames, device="cuda")
    on_slow = torch.ones(args.n_frames, device="cuda")
    bands = (["lo_onsets"] if width < 128 else []) + (["hi_onsets"] if width > 32 else [])
    for band in bands:
        envelope = getattr(args, band).to("cuda", torch.float32)
        on_jittery, on_slow = envelope + (1 - envelope) * on_jittery, (1 - envelope) * on_slow
    recipe = ar.NoiseSynth(height, width, [ar.noise_term(jittery, envelope=on_jittery), ar.noise_term(slow, envelope=on_slow)])
    return recipe.with_gain(1 / (2.5 * float(recipe.std())))  # the default's normalisation, from a sample of the frames
