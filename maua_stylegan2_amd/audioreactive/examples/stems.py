"""Plugin for renders that follow the sound SOURCES of a track: ``ar.components`` instead of the chromagram.

  * Latents: the magnitude spectrogram is factorised into ``N_STEMS`` sources (``ar.components``: spectral templates ordered from the
    lowest to the highest, one envelope per source and frame); the envelopes weight the first ``N_STEMS`` entries of the latent
    selection (``ar.chroma_weight_latents``), smoothed, with the default plugin's onset-driven jumps on top.  Two instruments that share
    a frequency band — which the band-split onsets cannot tell apart — pull toward different latents.
  * Bends: the lowest source (the bass or the kick) twists every other channel of the 16-px maps with an ``ar.Swirl`` whose angle
    follows its envelope.  The transform implements ``run_static``, so the render stays on the hipGraph lanes.
  * Noise: the brightest source of the PERCUSSIVE part of the track (hats, snare) takes the place of the bass onsets in the default
    plugin's noise cross-fade.
"""
import torch

import maua_stylegan2_amd.audioreactive as ar
from maua_stylegan2_amd.audioreactive.examples import default

N_STEMS = 4                # sources, and entries of the latent selection they weight
STEM_FLOOR = 0.05          # weight every source keeps, so that a silent frame is the mean of the entries and not the zero latent
SWIRL_LAYER = 4            # layer id of the 16-px feature maps
SWIRL_DEGREES, SWIRL_RADIUS = 180.0, 5.0
SWIRL_CHANNELS = range(0, 512, 2)


def initialize(args):
    args = default.initialize(args)
    args.stems = ar.components(args.audio, args.sr, args.n_frames, n_components=N_STEMS, smooth=3)
    args.hits = ar.components(args.audio, args.sr, args.n_frames, n_components=2, margin=8, smooth=1, power=2)[:, -1]
    return args


def get_latents(selection, args):
    weights = args.stems + STEM_FLOOR
    weights = weights / weights.sum(dim=1, keepdim=True)
    latents = ar.gaussian_filter(ar.chroma_weight_latents(weights, selection[:N_STEMS]), 4)
    for band in ("hi_onsets", "lo_onsets"):  # treble first, bass on top of it
        envelope = getattr(args, band)[:, None, None]
        latents = default._crossfade(envelope, selection[[default.JUMP_TARGETS[band]]], latents)
    return ar.gaussian_filter(latents, 2, causal=0.2)


def get_noise(height, width, scale, num_scales, args):
    if width > default.NOISE_MAX_WIDTH:
        return None
    hits = args.hits[:, None, None, None].cuda()
    treble = args.hi_onsets[:, None, None, None].cuda()
    jittery = default._filtered_field(args.n_frames, height, width, default.FAST_SIGMA)
    field = default._filtered_field(args.n_frames, height, width, default.SLOW_SIGMA)
    if width < 128:  # coarse scales follow the percussive source
        field = default._crossfade(hits, jittery, field)
    if width > 32:  # fine scales follow the treble
        field = default._crossfade(treble, jittery, field)
    return field / (field.std() * 2.5)


def get_bends(args):
    lowest = torch.as_tensor(args.stems[:, 0]).float().cpu()
    channels = list(SWIRL_CHANNELS)
    return [{"layer": SWIRL_LAYER, "modulation": SWIRL_DEGREES * (lowest - lowest.mean()),
             "transform": lambda m: ar.Swirl(m, radius=SWIRL_RADIUS, channels=channels)}]
