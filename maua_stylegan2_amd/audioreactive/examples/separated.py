"""Plugin for renders that follow the separated SOUND of a track's sources: ``ar.separate`` splits the clip into three stems (low,
middle, high — the factorisation's components in three contiguous runs of ascending spectral centroid), and every feature is taken of
a stem instead of a band-pass of the mix.

  * Latents: the pitch of the LOWEST stem (the bass line, without the lead above it) walks along the latent selection
    (``ar.pitch`` -> ``ar.pitch_weight_latents``), smoothed, with the default plugin's onset-driven jumps on top.
  * Noise: the onsets of the HIGHEST stem (hats, snare) take the place of the bass onsets in the default plugin's noise cross-fade.
  * Bends: the loudness of the lowest stem (``ar.rms``) twists every other channel of the 16-px maps with the ``ar.Swirl`` of
    ``stems.py``.  The transform implements ``run_static``, so the render stays on the hipGraph lanes.
"""
import torch

import maua_stylegan2_amd.audioreactive as ar
from maua_stylegan2_amd.audioreactive.examples import default, stems

N_COMPONENTS = 9           # components of the factorisation, three per stem
N_STEMS = 3
BASS_FMAX = 520            # Hz: the pitch range searched in the lowest stem


def initialize(args):
    args = default.initialize(args)
    args.separated = ar.separate(args.audio, args.sr, n_components=N_COMPONENTS, groups=N_STEMS)
    low, high = args.separated[0], args.separated[-1]
    args.bass_line = ar.pitch(low, args.sr, args.n_frames, fmax=BASS_FMAX, margin=None)
    args.bass_level = ar.rms(low, args.sr, args.n_frames, smooth=10, clip=97, power=1)
    args.hits = ar.onsets(high, args.sr, args.n_frames, margin=None, fmin=200, smooth=1, clip=99, power=2)
    return args


def get_latents(selection, args):
    latents = ar.gaussian_filter(ar.pitch_weight_latents(args.bass_line, selection), 4)
    for band in ("hi_onsets", "lo_onsets"):  # treble first, bass on top of it
        envelope = getattr(args, band)[:, None, None]
        latents = default._crossfade(envelope, selection[[default.JUMP_TARGETS[band]]], latents)
    return ar.gaussian_filter(latents, 2, causal=0.2)


def get_noise(height, width, scale, num_scales, args):
    return stems.get_noise(height, width, scale, num_scales, args)  # (args.hits: here the onsets of the highest stem)


def get_bends(args):
    level = torch.as_tensor(args.bass_level).float().cpu()
    channels = list(stems.SWIRL_CHANNELS)
    return [{"layer": stems.SWIRL_LAYER, "modulation": stems.SWIRL_DEGREES * (level - level.mean()),
             "transform": lambda m: ar.Swirl(m, radius=stems.SWIRL_RADIUS, channels=channels)}]
