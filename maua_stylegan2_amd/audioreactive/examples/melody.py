"""Plugin for renders that follow the melody: ``ar.pitch`` instead of the chromagram.

  * Latents: the pitch height of the lead (65 Hz .. 2.1 kHz after harmonic separation) walks along the latent selection
    (``ar.pitch_weight_latents``: low notes sit at the first entries, high notes at the last), smoothed, with the default plugin's
    onset-driven jumps on top.
  * Bends: a second pitch track, band-passed to 65 .. 260 Hz — the bass line under the lead — twists every other channel of the 16-px
    maps with an ``ar.Swirl`` whose angle is the bass line's height around its own mean.  The transform implements ``run_static``, so the
    render stays on the hipGraph lanes.
  * Noise and the onset envelopes are the default plugin's.
"""
import torch

import maua_stylegan2_amd.audioreactive as ar
from maua_stylegan2_amd.audioreactive.examples import default
from maua_stylegan2_amd.audioreactive.examples.default import get_noise  # noqa: F401

BASS_FMAX = 260            # Hz: the band of the second pitch track
SWIRL_LAYER = 4            # layer id of the 16-px feature maps
SWIRL_DEGREES, SWIRL_RADIUS = 240.0, 5.0
SWIRL_CHANNELS = range(0, 512, 2)


def initialize(args):
    args = default.initialize(args)
    args.melody = ar.pitch(args.audio, args.sr, args.n_frames)
    args.bass_line = ar.pitch(args.audio, args.sr, args.n_frames, fmax=BASS_FMAX, bandpass=True)
    return args


def get_latents(selection, args):
    latents = ar.gaussian_filter(ar.pitch_weight_latents(args.melody, selection), 4)
    for band in ("hi_onsets", "lo_onsets"):  # treble first, bass on top of it
        envelope = getattr(args, band)[:, None, None]
        latents = default._crossfade(envelope, selection[[default.JUMP_TARGETS[band]]], latents)
    return ar.gaussian_filter(latents, 2, causal=0.2)


def get_bends(args):
    bass = torch.as_tensor(args.bass_line).float().cpu()
    channels = list(SWIRL_CHANNELS)
    return [{"layer": SWIRL_LAYER, "modulation": SWIRL_DEGREES * (bass - bass.mean()),
             "transform": lambda m: ar.Swirl(m, radius=SWIRL_RADIUS, channels=channels)}]
