"""Plugin for tracks with a song structure: every section of the track loops through its own stretch of the latent selection.

``get_latents`` segments the track (``ar.laplacian_segmentation``: section boundaries and one label per section type), gives every section
type ``KEYS_PER_SECTION`` consecutive selection entries starting at its label, so a chorus that returns looks like itself again, and lets
each section run round its entries on a closed spline, the louder sections (mean of the rms envelope from ``initialize``) a little faster.
The whole sequence is one ``ar.loop_sections`` call, built on the device in a single launch however many sections the track has; a
Gaussian filter then softens the cuts between sections.  Noise is the default plugin's.
"""
import maua_stylegan2_amd.audioreactive as ar
from maua_stylegan2_amd.audioreactive.examples.default import get_noise  # noqa: F401

SECTION_TYPES = 4      # k of the segmentation: how many kinds of section to tell apart
KEYS_PER_SECTION = 4   # selection entries one section type loops through
LOUD_EXTRA_LOOPS = 1.0  # a section of full loudness makes this many more rounds than a silent one
CUT_SIGMA = 3          # frames over which a cut between sections is softened


def initialize(args):
    args.rms = ar.rms(args.audio, args.sr, args.n_frames, smooth=10, clip=60, power=1)
    return args


def get_latents(selection, args):
    times, labels = ar.laplacian_segmentation(args.audio, args.sr, k=SECTION_TYPES)
    bounds = [min(max(int(round(t / args.duration * args.n_frames)), 0), args.n_frames) for t in times]
    spans = list(zip(bounds, bounds[1:]))
    frames = [max(stop - start, 0) for start, stop in spans]
    loudness = [float(args.rms[start:stop].mean()) if stop > start else 0.0 for start, stop in spans]
    n_loops = [min(1.0 + LOUD_EXTRA_LOOPS * loud, max(n, 1)) for loud, n in zip(loudness, frames)]  # at least one frame per round
    key_starts = [label % len(selection) for label in labels]
    latents = ar.loop_sections(selection, frames, key_starts, min(KEYS_PER_SECTION, len(selection)), n_loops, n_frames=args.n_frames)
    return ar.gaussian_filter(latents, CUT_SIGMA)
