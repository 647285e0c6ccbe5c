"""``melody.py`` with the probabilistic tracker: both pitch tracks come from ``ar.pitch(method="pyin")``.

Use it where the lead is not a clean solo line — a mixed track, a noisy recording, a separated stem: plain YIN falls to a subharmonic
wherever no lag gets under its threshold, and the voicing gate, hold and median of ``ar.pitch`` only paper over that; the pYIN decoder
keeps every candidate of a frame and picks the path that moves least.  Latents, bends and noise are ``melody.py``'s.
"""
import maua_stylegan2_amd.audioreactive as ar
from maua_stylegan2_amd.audioreactive.examples import default
from maua_stylegan2_amd.audioreactive.examples.melody import BASS_FMAX, get_bends, get_latents, get_noise  # noqa: F401


def initialize(args):
    args = default.initialize(args)
    args.melody = ar.pitch(args.audio, args.sr, args.n_frames, method="pyin")
    args.bass_line = ar.pitch(args.audio, args.sr, args.n_frames, fmax=BASS_FMAX, bandpass=True, method="pyin")
    return args
