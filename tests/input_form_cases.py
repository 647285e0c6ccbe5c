"""The table behind tests/test_input_forms_*.py: one row per public ``ar.*`` function whose body, or whose private helper, launches a
native entry, with small valid operands, and the shape mismatches every such function has to refuse.

Operand values are drawn as float32 (or small integers) once, here, on the host, so that every form of an operand — float64, another
device, a strided view — holds exactly the same numbers and every cast the glue makes is exact.  Nothing in this module touches a
device: the GPU test puts the operands where a form wants them.

Which answer a form gets is fixed here, not discovered at run time: a row ACCEPTS every form of every varied operand (same dtype,
shape and bits as the canonical call) unless ``refuse`` names the (operand, form) pair, which must then raise ValueError / TypeError
naming the function without a launch.  No row refuses anything today: every function normalises through ``signal._to_dev`` (or its
module's own helper), which hands a canonical operand back as it is and moves everything else to the current device."""
import numpy as np

SR = 22050
N_AUDIO = 4099  # > n_fft / 2 (the reflect pad), no multiple of the hop, 1 + 4099 // 512 = 9 frames
FORMS = ("canon", "np64", "cpu32", "dev64", "strided", "otherdev")


class Operand:
    """``values``: the numbers, a numpy array of the canonical dtype.  ``where``: the documented home of the operand, "np" (a clip or a
    host table: numpy) or "dev" (a contiguous tensor on the device)."""

    def __init__(self, values, where="dev"):
        self.values, self.where = np.ascontiguousarray(values), where


class Row:
    """``name``: "module.function".  ``call(m, o)``: runs it with the modules ``m`` (attributes signal, decompose, ...) and the operands
    ``o`` (name -> array or tensor).  ``varied``: the operands that are given in every form.  ``covers``: the enclosing functions
    ("module.function") of the ``_lib.call`` sites this row runs."""

    def __init__(self, name, operands, call, varied, covers, refuse=()):
        self.name, self.operands, self.call, self.varied, self.covers, self.refuse = name, operands, call, tuple(varied), tuple(covers), frozenset(refuse)

    @property
    def function(self):
        return self.name.split(".", 1)[1]


def _rng(seed):
    return np.random.default_rng(seed)


def _f32(seed, *shape, positive=False):
    x = _rng(seed).standard_normal(shape).astype(np.float32)
    return np.abs(x) + np.float32(0.01) if positive else x


def _audio():
    t = np.arange(N_AUDIO, dtype=np.float64) / SR
    tone = 0.4 * np.sin(2 * np.pi * 220.0 * t) * (1.0 + 0.5 * np.sin(2 * np.pi * 3.0 * t))
    return (tone + 0.05 * _rng(1).standard_normal(N_AUDIO)).astype(np.float32)


def _clip():
    return {"audio": Operand(_audio(), "np")}


def _log_probs(seed, *shape):
    p = _rng(seed).random(shape) + 0.1
    return np.log(p / p.sum(-1, keepdims=True)).astype(np.float32)


def _probs(seed, *shape):
    p = _rng(seed).random(shape) + 0.1
    return (p / p.sum(-1, keepdims=True)).astype(np.float32)


def _links(seed, s):
    d = np.abs(_rng(seed).standard_normal((s, s))).astype(np.float32)
    d = np.minimum(d, d.T)
    d[_rng(seed + 1).random((s, s)) < 0.5] = -1.0
    return d


def _bank_sos():
    import scipy.signal

    return np.stack([scipy.signal.butter(4, band, "bp", output="sos") for band in ([0.1, 0.3], [0.2, 0.5])])  # [2, 4, 6]


F, T, K = 13, 70, 3          # a spectrogram: T is above the 64 the matrix entries tile by
S, N_HMM = 3, 5              # hidden states, frames
N_TEMPI, WIN = 7, 8          # a tempogram table [7, 8, 2]
BAR_INTERVAL, BAR_WIDTH = np.array([2, 3], np.int32), np.array([1, 1], np.int32)
SYNC_BOUNDS = np.array([0, 3, 10, 11, 40, T], np.int32)

ROWS = [
    # ------------------------------------------------------------------------------------------------ signal
    Row("signal.stft_power", _clip(), lambda m, o: m.signal.stft_power(o["audio"]), ["audio"], ["signal.stft_power"]),
    Row("signal.stft_complex", _clip(), lambda m, o: m.signal.stft_complex(o["audio"]), ["audio"], ["signal.stft_complex"]),
    Row("signal.project", {"fb": Operand(_f32(2, F, T), "np"), "p": Operand(_f32(3, T, 9))},
        lambda m, o: m.signal.project(o["fb"], o["p"]), ["fb", "p"], ["signal.project"]),
    Row("signal.hpss", _clip(), lambda m, o: m.signal.hpss(o["audio"]), ["audio"], ["signal.hpss"]),
    Row("signal.resample", {"x": Operand(_f32(4, 9, 3))}, lambda m, o: m.signal.resample(o["x"], 14), ["x"], ["signal.resample"]),
    Row("signal.gaussian_filter", {"x": Operand(_f32(5, T, 3))}, lambda m, o: m.signal.gaussian_filter(o["x"], 2), ["x"],
        ["signal.gaussian_filter"]),
    Row("signal.cens", {"ch": Operand(_f32(6, 12, T, positive=True))}, lambda m, o: m.signal.cens(o["ch"]), ["ch"], ["signal.cens"]),
    Row("signal.nn_filter", {"ch": Operand(_f32(7, 12, T, positive=True))}, lambda m, o: m.signal.nn_filter(o["ch"]), ["ch"],
        ["signal.nn_filter"]),
    Row("signal.cqt_magnitude", _clip(), lambda m, o: m.signal.cqt_magnitude(o["audio"], SR, n_bins=12, fmin=440.0, bins_per_octave=12),
        ["audio"], ["signal.cqt_magnitude"]),
    Row("signal.raw_pitch", _clip(), lambda m, o: m.signal.raw_pitch(o["audio"], SR), ["audio"], ["signal.raw_pitch"]),
    Row("signal.raw_pyin", _clip(), lambda m, o: m.signal.raw_pyin(o["audio"], SR), ["audio"], ["signal._pyin_stages"]),
    # ------------------------------------------------------------------------------------------------ decompose
    Row("decompose.nmf", {"V": Operand(_f32(8, F, T, positive=True)), "W": Operand(_f32(9, F, K, positive=True))},
        lambda m, o: m.decompose.nmf(o["V"], K, n_iter=3, W=o["W"]), ["V", "W"], ["decompose._iterate"]),
    Row("decompose.nmf_divergence", {"V": Operand(_f32(8, F, T, positive=True)), "W": Operand(_f32(9, F, K, positive=True)),
                                     "H": Operand(_f32(10, K, T, positive=True))},
        lambda m, o: m.decompose.nmf_divergence(o["V"], o["W"], o["H"]), ["V", "W", "H"], ["decompose.nmf_divergence"]),
    Row("decompose.separate", _clip(), lambda m, o: m.decompose.separate(o["audio"], SR, n_components=K, n_iter=3), ["audio"],
        ["decompose._masked_spectra", "decompose.separate"]),
    # ------------------------------------------------------------------------------------------------ beat
    Row("beat.raw_plp", _clip(), lambda m, o: m.beat.raw_plp(o["audio"], SR, tempo_min=60, tempo_max=240, tempo_step=30, win=WIN), ["audio"],
        ["beat.tempogram_peak", "beat.pulse_synth"]),
    Row("beat.tempogram_peak", {"env": Operand(_f32(11, T, positive=True)), "table": Operand(_f32(12, N_TEMPI, WIN, 2)),
                                "prior": Operand(_f32(13, N_TEMPI, positive=True))},
        lambda m, o: m.beat.tempogram_peak(o["env"], o["table"], o["prior"], want_tgram=True), ["env", "table", "prior"],
        ["beat.tempogram_peak"]),
    Row("beat.pulse_synth", {"bins": Operand(_rng(14).integers(-1, N_TEMPI, T).astype(np.int32)), "phase": Operand(_f32(15, T)),
                             "window": Operand(_f32(16, WIN, positive=True)), "omega": Operand(_f32(17, N_TEMPI, positive=True))},
        lambda m, o: m.beat.pulse_synth(o["bins"], o["phase"], o["window"], o["omega"]), ["bins", "phase", "window", "omega"],
        ["beat.pulse_synth"]),
    # ------------------------------------------------------------------------------------------------ segment
    Row("segment.tempogram", {"env": Operand(_f32(18, T, positive=True))}, lambda m, o: m.segment.tempogram(o["env"], 16), ["env"],
        ["segment.tempogram"]),
    Row("segment.beat_dp", {"onset": Operand(_f32(19, T, positive=True))}, lambda m, o: m.segment.beat_dp(o["onset"], 5), ["onset"],
        ["segment.beat_dp"]),
    Row("segment.beat_sync", {"x": Operand(_f32(20, 5, T)), "bounds": Operand(SYNC_BOUNDS, "np")},
        lambda m, o: m.segment.beat_sync(o["x"], o["bounds"], True), ["x", "bounds"], ["segment.beat_sync"]),
    Row("segment.knn_links", {"x": Operand(_f32(21, 5, T))}, lambda m, o: m.segment.knn_links(o["x"], 3), ["x"], ["segment.knn_links"]),
    Row("segment.rec_affinity", {"links": Operand(_links(22, T))}, lambda m, o: m.segment.rec_affinity(o["links"], 0.5), ["links"],
        ["segment.rec_affinity"]),
    # ------------------------------------------------------------------------------------------------ harmony, bars
    Row("harmony.viterbi", {"logobs": Operand(_log_probs(23, N_HMM, S)), "log_trans": Operand(_log_probs(24, S, S)),
                            "log_init": Operand(_log_probs(25, S))},
        lambda m, o: m.harmony.viterbi(o["logobs"], o["log_trans"], o["log_init"]), ["logobs", "log_trans", "log_init"], ["harmony.viterbi"]),
    Row("harmony.hmm_posterior", {"obs": Operand(_probs(26, N_HMM, S)), "trans": Operand(_probs(27, S, S)), "init": Operand(_probs(28, S))},
        lambda m, o: m.harmony.hmm_posterior(o["obs"], o["trans"], o["init"]), ["obs", "trans", "init"], ["harmony._posterior"]),
    Row("bars.bar_viterbi", {"logobs": Operand(_log_probs(29, N_HMM, 3)), "log_change": Operand(_log_probs(30, 2, 2))},
        lambda m, o: m.bars.bar_viterbi(o["logobs"], BAR_INTERVAL, BAR_WIDTH, o["log_change"], (3, 4)), ["logobs", "log_change"],
        ["bars.bar_viterbi"]),
    # ------------------------------------------------------------------------------------------------ filters
    Row("filters.sosfilt", {"x": Operand(_f32(31, 2, T)), "zi": Operand(_f32(32, 2, 4, 2))},
        lambda m, o: m.filters.sosfilt(_bank_sos(), o["x"], zi=o["zi"]), ["x", "zi"], ["filters._run"]),
    Row("filters.sosfiltfilt", {"x": Operand(_f32(33, 150))}, lambda m, o: m.filters.sosfiltfilt(_bank_sos()[0], o["x"]), ["x"],
        ["filters._run"]),
    Row("filters.envelope", {"x": Operand(_f32(34, T, 3)), "y0": Operand(_f32(35, 3))},
        lambda m, o: m.filters.envelope(o["x"], 2, 5, y0=o["y0"]), ["x", "y0"], ["filters.envelope"]),
    # ------------------------------------------------------------------------------------------------ latent
    Row("latent.perlin_noise", {"gradients": Operand(_f32(36, 3, 4, 5, 3), "np")},
        lambda m, o: m.latent.perlin_noise((4, 6, 8), (2, 3, 4), gradients=o["gradients"]), ["gradients"], ["latent.perlin_noise"]),
    Row("latent.loop_sections", {"selection": Operand(_f32(37, 5, 2, 7))},
        lambda m, o: m.latent.loop_sections(o["selection"], [9, 6], [0, 2], 4, 1), ["selection"], ["latent._loop_sequence"]),
]

# call sites no row runs, each with its reason
EXCLUDED_MODULES = {
    "bend": "the tensor operands are the generator's own feature maps; test_bend_* cover the table arguments",
    "noise": "NoiseSynth builds its table from its own banks; test_noise_synth_gpu.py covers the recipe arguments",
}
EXCLUDED_FUNCTIONS = {
    "signal._median5": "private: pitch() and tempo() hand it a float32 device tensor they made themselves",
    "segment.spectral_embedding": "launches on the eigenvectors it computes itself; its arguments are outputs of rec_affinity and beat_sync",
}


# ------------------------------------------------------------------------------------------------ shape mismatches
class Mismatch:
    """``call(m, put)`` runs ``function`` with one tied dimension off by one; ``put`` places a numpy array as the canonical device
    tensor.  It must raise ValueError naming the function and launch nothing."""

    def __init__(self, name, function, call):
        self.name, self.function, self.call = name, function, call


def _mismatches():
    out = []

    def add(name, function, call):
        out.append(Mismatch(name, function, call))

    pos = dict(positive=True)
    for d, tag in ((1, "+1"), (-1, "-1")):
        add(f"project[p-rows{tag}]", "project", lambda m, put, d=d: m.signal.project(_f32(2, F, T), put(_f32(3, T + d, 9))))
        add(f"nmf_divergence[H-rows{tag}]", "nmf_divergence",
            lambda m, put, d=d: m.decompose.nmf_divergence(put(_f32(8, F, T, **pos)), put(_f32(9, F, K, **pos)), put(_f32(10, K + d, T, **pos))))
        add(f"nmf_divergence[H-cols{tag}]", "nmf_divergence",
            lambda m, put, d=d: m.decompose.nmf_divergence(put(_f32(8, F, T, **pos)), put(_f32(9, F, K, **pos)), put(_f32(10, K, T + d, **pos))))
        add(f"nmf_divergence[W-rows{tag}]", "nmf_divergence",
            lambda m, put, d=d: m.decompose.nmf_divergence(put(_f32(8, F, T, **pos)), put(_f32(9, F + d, K, **pos)), put(_f32(10, K, T, **pos))))
        add(f"nmf[W-rows{tag}]", "nmf", lambda m, put, d=d: m.decompose.nmf(put(_f32(8, F, T, **pos)), K, n_iter=3, W=put(_f32(9, F + d, K, **pos))))
        add(f"nmf[W-cols{tag}]", "nmf", lambda m, put, d=d: m.decompose.nmf(put(_f32(8, F, T, **pos)), K, n_iter=3, W=put(_f32(9, F, K + d, **pos))))
        add(f"tempogram_peak[prior{tag}]", "tempogram_peak",
            lambda m, put, d=d: m.beat.tempogram_peak(put(_f32(11, T, **pos)), put(_f32(12, N_TEMPI, WIN, 2)), put(_f32(13, N_TEMPI + d, **pos))))
        for function, data in (("viterbi", _log_probs), ("hmm_posterior", _probs)):
            add(f"{function}[matrix{tag}]", function,
                lambda m, put, d=d, f=function, g=data: getattr(m.harmony, f)(put(g(23, N_HMM, S)), put(g(24, S + d, S)), put(g(25, S))))
            add(f"{function}[vector{tag}]", function,
                lambda m, put, d=d, f=function, g=data: getattr(m.harmony, f)(put(g(23, N_HMM, S)), put(g(24, S, S)), put(g(25, S + d))))
        add(f"sosfilt[zi-sections{tag}]", "sosfilt", lambda m, put, d=d: m.filters.sosfilt(_bank_sos(), put(_f32(31, 2, T)), zi=put(_f32(32, 2, 4 + d, 2))))
        add(f"sosfilt[zi-filters{tag}]", "sosfilt", lambda m, put, d=d: m.filters.sosfilt(_bank_sos(), put(_f32(31, 2, T)), zi=put(_f32(32, 2 + d, 4, 2))))
        add(f"sosfilt[x-rows{tag}]", "sosfilt", lambda m, put, d=d: m.filters.sosfilt(_bank_sos(), put(_f32(31, 2 + d, T))))
        add(f"bar_viterbi[width{tag}]", "bar_viterbi",
            lambda m, put, d=d: m.bars.bar_viterbi(put(_log_probs(29, N_HMM, 3)), BAR_INTERVAL, np.ones(2 + d, np.int32), put(_log_probs(30, 2, 2))))
        add(f"bar_viterbi[log_change{tag}]", "bar_viterbi",
            lambda m, put, d=d: m.bars.bar_viterbi(put(_log_probs(29, N_HMM, 3)), BAR_INTERVAL, BAR_WIDTH, put(_log_probs(30, 2 + d, 2))))
    # bounds beyond the frame count: one frame past the end, one before the start
    add("beat_sync[bounds+1]", "beat_sync", lambda m, put: m.segment.beat_sync(put(_f32(20, 5, T)), np.array([0, 3, 10, T + 1]), True))
    add("beat_sync[bounds-1]", "beat_sync", lambda m, put: m.segment.beat_sync(put(_f32(20, 5, T)), np.array([-1, 3, 10, T]), True))
    return out


MISMATCHES = _mismatches()
