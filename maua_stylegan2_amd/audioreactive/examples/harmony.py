"""Plugin for renders that follow the harmony: one latent per chord root, switching where the chord changes.

  * Latents: ``ar.chords(by="root", relative_to="key")`` weights the first twelve entries of the selection — entry 0 is the tonic of
    the clip's key, entry 7 its dominant — where the default plugin mixes them by the twelve smeared envelopes of ``ar.chroma``.  The
    picture holds still inside a chord and moves in a step with the music.  Needs a selection of at least twelve latents.
  * Noise: the default plugin's fast and slow fields, cross-faded by ``1 - confidence`` of the chord decoder: calm where the harmony is
    clear, restless through changes, dissonance and noise.
  * Bends: none.
"""
import maua_stylegan2_amd.audioreactive as ar
from maua_stylegan2_amd.audioreactive.examples import default

VOCABULARY = "triads"
LATENT_SMOOTH, DOUBT_SMOOTH = 2, 4


def initialize(args):
    track = ar.raw_chords(args.audio, args.sr, vocabulary=VOCABULARY)
    args.chords = ar.chords(args.audio, args.sr, args.n_frames, by="root", relative_to="key", smooth=LATENT_SMOOTH, track=track)
    doubt = ar.lerp_resize(1.0 - track.confidence, args.n_frames)
    args.doubt = ar.gaussian_filter(doubt, DOUBT_SMOOTH).clamp(0, 1).cpu()
    return args


def get_latents(selection, args):
    if selection.shape[0] < 12:
        raise ValueError(f"examples/harmony.py weights one latent per chord root: the selection needs 12 entries (got {selection.shape[0]})")
    return ar.chroma_weight_latents(args.chords, selection[:12])


def get_noise(height, width, scale, num_scales, args):
    if width > default.NOISE_MAX_WIDTH:
        return None
    doubt = args.doubt[:, None, None, None].cuda()
    jittery = default._filtered_field(args.n_frames, height, width, default.FAST_SIGMA)
    field = default._crossfade(doubt, jittery, default._filtered_field(args.n_frames, height, width, default.SLOW_SIGMA))
    return field / (field.std() * 2.5)
