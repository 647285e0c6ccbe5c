"""Drop-in for the reference's ``audioreactive`` package: everything star-exported as ``ar.*``
(/root/reference/audioreactive/__init__.py:1-5)."""
from . import signal as _signal_module
from .bars import *  # noqa: F401,F403  (bar_model, bar_viterbi, raw_bars, downbeats, metre, bar_phase, bar_beats: the bar-pointer model, no counterpart in the reference)
from .beat import *  # noqa: F401,F403  (raw_plp, tempogram, pulse, tempo, beats, beat_phase: the predominant local pulse, no counterpart in the reference)
from .bend import *  # noqa: F401,F403
from .decompose import *  # noqa: F401,F403  (nmf, decompose, components: spectrogram factorisation, no counterpart in the reference)
from .feedback import *  # noqa: F401,F403  (Feedback: frame feedback — trails, echo tunnels — on the fp32 image, no counterpart in the reference)
from .filters import *  # noqa: F401,F403  (sosfilt, sosfiltfilt, bandpass, envelope, bands: recursive filters on the device, no counterpart in the reference)
from .grade import *  # noqa: F401,F403  (Grade, load_cube, save_cube, lut_from_function: colour grading of the fp32 image, no counterpart in the reference)
from .harmony import *  # noqa: F401,F403  (viterbi, hmm_posterior, chord_vocabulary, raw_chords, chords, key: chords and key, no counterpart in the reference)
from .latent import *  # noqa: F401,F403
from .lens import *  # noqa: F401,F403  (Lens: bloom, sharpen and vignette on the fp32 image, no counterpart in the reference)
from .noise import *  # noqa: F401,F403  (NoiseSynth, noise_term: synthesised noise slots, no counterpart in the reference)
from .signal import *  # noqa: F401,F403
from .signal import set_SMF  # noqa: F401
from ..models.stylegan2 import Generator  # noqa: F401,E402  (the reference's latent.py leaks it into ar.* through its star import)
from .util import *  # noqa: F401,F403,E402  (diagnostics: info + matplotlib plots, imported lazily)
