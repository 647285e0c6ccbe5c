"""What every native entry the audio modules launch reads and writes, restated from the entries' comments in include/maua_hip.h, and a
wrapper of ``_lib.call`` that refuses a launch whose buffers do not fit that statement.

A spec is a function of the entry's arguments as ``_lib.call`` receives them (everything but the trailing stream) that returns a list
of ``(argument index, dtype, minimum numel)``, one per tensor operand; the minimum is computed from the integer arguments alone, the
way the header states the layout, never from the tensors and never from what the Python callers happen to allocate.  ``dtype`` is a
torch dtype, or a tuple of them where the header's C type has more than one torch spelling (uint16_t).  Operands the header lets be
NULL are named in ``NULLABLE``.  Struct tables that live in device memory travel as uint8 tensors of the struct's size.

``checked_call(real_call)`` is a drop-in for ``_lib.call``: it looks the spec up, checks every tensor operand's dtype and numel and
raises AssertionError BEFORE forwarding on any mismatch, so that no test built on it starts a kernel on a mistyped or undersized
buffer; otherwise it forwards and counts one launch."""
import inspect

import numpy as np
import torch as th

F32, F64, I32, U8 = th.float32, th.float64, th.int32, th.uint8
U16 = (th.int16, getattr(th, "uint16", th.int16))  # uint16_t: torch code that predates torch.uint16 carries its bits in int16

# maua_frame_source_t: int32 frame0, int32 pad_, two pointers, 32 noise pointers, 32 int64 strides
FRAME_SOURCE_BYTES = 4 + 4 + 8 + 8 + 32 * 8 + 32 * 8
# maua_noise_synth_slot_t: pointer dst, int32 hw, slot, n_terms, float gain, uint64 seed, 4 terms of (3 pointers, int32 period, phase)
NOISE_SYNTH_SLOT_BYTES = 8 + 4 + 4 + 4 + 4 + 8 + 4 * (3 * 8 + 4 + 4)

SPECS = {}
NULLABLE = {}


def spec(name, nullable=()):
    def register(fn):
        assert name not in SPECS, name
        SPECS[name] = fn
        NULLABLE[name] = frozenset(nullable)
        return fn

    return register


def _query(name, *args):
    """A host query of the library (workspace sizes the header defines only through it)."""
    from maua_stylegan2_amd import _lib

    return int(getattr(_lib.load(), name)(*[int(a) for a in args]))


# ------------------------------------------------------------------------------------------------ signal
@spec("maua_temporal_fir_f32")
def _temporal_fir(x, taps, y, n_frames, features, radius):
    return [(0, F32, n_frames * features), (1, F32, 2 * radius + 1), (2, F32, n_frames * features)]


@spec("maua_stft_power_f32")
def _stft_power(y, n_samples, window, n_fft, hop, p, n_frames):
    return [(0, F32, n_samples), (2, F32, n_fft), (5, F32, (n_fft // 2 + 1) * n_frames)]


@spec("maua_stft_complex_f32")
def _stft_complex(y, n_samples, window, n_fft, hop, out_re, out_im, n_frames):
    spectrum = (n_fft // 2 + 1) * n_frames
    return [(0, F32, n_samples), (2, F32, n_fft), (5, F32, spectrum), (6, F32, spectrum)]


@spec("maua_istft_f32")
def _istft(in_re, in_im, window, n_fft, hop, n_frames, frames_ws, y, n_samples):
    spectrum = (n_fft // 2 + 1) * n_frames
    return [(0, F32, spectrum), (1, F32, spectrum), (2, F32, n_fft), (6, F32, n_frames * n_fft), (7, F32, n_samples)]


@spec("maua_median_filter_f32")
def _median_filter(x, y, rows, cols, size, axis):
    return [(0, F32, rows * cols), (1, F32, rows * cols)]


@spec("maua_softmask_apply_f32")
def _softmask(re, im, x, x_ref, margin, power, split_zeros, out_re, out_im, n):
    return [(i, F32, n) for i in (0, 1, 2, 3, 7, 8)]


@spec("maua_filterbank_f32")
def _filterbank(fb, p, out, m, k, n, to_db, amin):
    return [(0, F32, m * k), (1, F32, k * n), (2, F32, m * n)]


@spec("maua_resample_f64")
def _resample(x, n, features, y, num):
    return [(0, F64, n * features), (3, F64, num * features)]


@spec("maua_cqt_mag_f32")
def _cqt_mag(y, n_samples, freqs, lengths, n_bins, hop, sr, out, n_frames):
    return [(0, F32, n_samples), (2, F32, n_bins), (3, I32, n_bins), (7, F32, n_bins * n_frames)]


@spec("maua_chroma_cens_f32")
def _chroma_cens(ch, out, n_bins, n_frames, win_len):
    return [(0, F32, n_bins * n_frames), (1, F32, n_bins * n_frames)]


@spec("maua_nn_median_f32", nullable=(6,))
def _nn_median(ch, out, n_bins, n_frames, k, width, ws):
    return [(0, F32, n_bins * n_frames), (1, F32, n_bins * n_frames), (6, F64, min(n_frames, 1024) * n_frames)]


@spec("maua_yin_f32", nullable=(10,))
def _yin(y, n_samples, frame, hop, tau_min, tau_max, threshold, lag, aperiodicity, tau_int, cmndf, n_frames):
    return [(0, F32, n_samples), (7, F32, n_frames), (8, F32, n_frames), (9, I32, n_frames), (10, F32, n_frames * (tau_max + 1))]


@spec("maua_pyin_candidates_f32")
def _pyin_candidates(cmndf, n_frames, tau_min, tau_max, cum_prior, n_thr, no_trough_prob, bin_edge_period, n_bins, obs, period, voiced_prob):
    return [(0, F32, n_frames * (tau_max + 1)), (4, F32, n_thr + 1), (7, F32, n_bins + 1), (9, F32, n_frames * n_bins),
            (10, F32, n_frames * n_bins), (11, F32, n_frames)]


@spec("maua_pyin_viterbi_f64")
def _pyin_viterbi(logobs_voiced, logobs_unvoiced, n_frames, n_bins, width, log_tri, log_norm, log_init, log_stay, log_switch, delta_last,
                  backptr, states):
    return [(0, F32, n_frames * n_bins), (1, F32, n_frames), (5, F64, 2 * width + 1), (6, F64, n_bins), (10, F64, 2 * n_bins),
            (11, U16, n_frames * 2 * n_bins), (12, I32, n_frames)]


# ------------------------------------------------------------------------------------------------ beat
@spec("maua_tempogram_peak_f32", nullable=(5, 9))
def _tempogram_peak(env, n, table, win, n_tempi, prior, bins, phase, power, tgram):
    return [(0, F32, n), (2, F32, n_tempi * win * 2), (5, F32, n_tempi), (6, I32, n), (7, F32, n), (8, F32, n), (9, F32, n * n_tempi)]


@spec("maua_pulse_synth_f32")
def _pulse_synth(bins, phase, n, window, win, omega, n_tempi, pulse):
    return [(0, I32, n), (1, F32, n), (3, F32, win), (5, F32, n_tempi), (7, F32, n)]


# ------------------------------------------------------------------------------------------------ harmony, bars
@spec("maua_hmm_viterbi_f64")
def _hmm_viterbi(logobs, log_trans, log_init, n_frames, n_states, delta_last, backptr, states):
    return [(0, F32, n_frames * n_states), (1, F64, n_states * n_states), (2, F64, n_states), (5, F64, n_states),
            (6, U8, n_frames * n_states), (7, I32, n_frames)]


@spec("maua_hmm_posterior_f64")
def _hmm_posterior(obs, trans, init, n_frames, n_states, gamma, scale):
    return [(0, F32, n_frames * n_states), (1, F64, n_states * n_states), (2, F64, n_states), (5, F64, n_frames * n_states),
            (6, F64, n_frames)]


@spec("maua_bar_viterbi_f64")
def _bar_viterbi(logobs, n_frames, interval, width, log_change, n_tempi, beats_per_bar, n_models, ws, score, path):
    ws_bytes = _query("maua_bar_ws_bytes", n_frames, n_tempi, max(int(b) for b in beats_per_bar), n_models)
    return [(0, F32, n_frames * 3), (4, F64, n_tempi * n_tempi), (8, U8, ws_bytes), (9, F64, n_models), (10, I32, n_models * n_frames * 3)]


# ------------------------------------------------------------------------------------------------ decompose
@spec("maua_nmf_kl_f32")
def _nmf_kl(v, w, h, F, T, K, n_iter, update_w, update_h, eps):
    return [(0, F32, F * T), (1, F32, F * K), (2, F32, K * T)]


@spec("maua_nmf_kl_div_f32")
def _nmf_kl_div(v, w, h, F, T, K, eps, d_cols):
    return [(0, F32, F * T), (1, F32, F * K), (2, F32, K * T), (7, F64, T)]


@spec("maua_nmf_separate_f32")
def _nmf_separate(re, im, w, h, group, F, T, K, G, power, g0, n_out, out_re, out_im):
    return [(0, F32, F * T), (1, F32, F * T), (2, F32, F * K), (3, F32, K * T), (12, F32, n_out * F * T), (13, F32, n_out * F * T)]


# ------------------------------------------------------------------------------------------------ segment
@spec("maua_tempogram_f32")
def _tempogram(env, n_frames, win, ws, tg):
    return [(0, F32, n_frames), (3, F64, _query("maua_tempogram_ws_doubles", n_frames, win)), (4, F32, win)]


@spec("maua_beat_track_f64")
def _beat_track(onset, n_frames, period, localscore, cumscore, backlink):
    return [(0, F64, n_frames), (3, F64, n_frames), (4, F64, n_frames), (5, I32, n_frames)]


@spec("maua_beat_sync_f32")
def _beat_sync(x, rows, n_frames, bounds, n_spans, median, out):
    return [(0, F32, rows * n_frames), (3, I32, n_spans + 1), (6, F32, rows * n_spans)]


@spec("maua_knn_links_f32")
def _knn_links(x, d, s, k, width, links):
    return [(0, F32, d * s), (5, F32, s * s)]


@spec("maua_rec_affinity_f32")
def _rec_affinity(links, s, bandwidth, rec, rec_filt):
    return [(0, F32, s * s), (3, F32, s * s), (4, F32, s * s)]


# ------------------------------------------------------------------------------------------------ filters
@spec("maua_sosfilt_f64", nullable=(3, 4, 8, 9, 10, 11))
def _sosfilt(sos, n_filters, n_sections, x_f32, x_f64, n_signals, n, chunk, zi, y_f64, y_f32, zf, ws):
    state = n_filters * n_sections * 2
    return [(0, F64, n_filters * n_sections * 6), (3, F32, n_signals * n), (4, F64, n_signals * n), (8, F64, state),
            (9, F64, n_filters * n), (10, F32, n_filters * n), (11, F64, state),
            (12, F64, _query("maua_sosfilt_ws_doubles", n_filters, n_sections, n, chunk))]


@spec("maua_env_follow_f32", nullable=(1,))
def _env_follow(x, y0, y, n_frames, n_cols, attack_coef, release_coef):
    return [(0, F32, n_frames * n_cols), (1, F32, n_cols), (2, F32, n_frames * n_cols)]


# ------------------------------------------------------------------------------------------------ latent
@spec("maua_perlin3d_f32")
def _perlin3d(grad, out, n0, n1, n2, r0, r1, r2):
    return [(0, F32, (r0 + 1) * (r1 + 1) * (r2 + 1) * 3), (1, F32, n0 * n1 * n2)]


@spec("maua_keyframe_blend_f32")
def _keyframe_blend(bank, n_bank, feats, key_idx, weights, row_of_frame, sec_of_frame, out, n_frames, n_sections, n_rows, kmax):
    return [(0, F32, n_bank * feats), (3, I32, n_sections * kmax), (4, F32, n_rows * kmax), (5, I32, n_frames), (6, I32, n_frames),
            (7, F32, n_frames * feats)]


# ------------------------------------------------------------------------------------------------ noise, bends
@spec("maua_noise_synth_f32", nullable=(4,))
def _noise_synth(table, n_slots, batch, frame0, src):
    return [(0, U8, n_slots * NOISE_SYNTH_SLOT_BYTES), (4, U8, FRAME_SOURCE_BYTES)]


@spec("maua_affine_reflect_warp_mapped_f32", nullable=(11, 12, 13, 14))
def _affine_warp_mapped(x, m, y, batch, channels, h, w, pad_l, pad_r, pad_t, pad_b, add_noise, xmap, ymap, src):
    maps = batch * channels * h * w
    # m: one map per sample; with a frame source it is the sequence of the render, of which rows frame0 .. frame0 + batch - 1 are read
    return [(0, F32, maps), (1, F32, batch * 6), (2, F32, maps), (11, F32, (h + pad_t + pad_b) * (w + pad_l + pad_r)),
            (12, I32, w + pad_l + pad_r), (13, I32, h + pad_t + pad_b), (14, U8, FRAME_SOURCE_BYTES)]


@spec("maua_bend_point_f32", nullable=(6, 8, 9))
def _bend_point(x, y, batch, channels, hw, op, param, param_rows, chan_mask, src):
    return [(0, F32, batch * channels * hw), (1, F32, batch * channels * hw), (6, F32, param_rows), (8, U8, channels),
            (9, U8, FRAME_SOURCE_BYTES)]


@spec("maua_bend_morph_f32", nullable=(9, 10))
def _bend_morph(x, y, batch, channels, h, w, op, radius, radius_rows, chan_mask, src):
    return [(0, F32, batch * channels * h * w), (1, F32, batch * channels * h * w), (7, I32, radius_rows), (9, U8, channels),
            (10, U8, FRAME_SOURCE_BYTES)]


@spec("maua_bend_pad_f32", nullable=(12,))
def _bend_pad(x, y, batch, channels, h, w, pad_l, pad_r, pad_t, pad_b, mode, value, noise, noise_channels):
    padded = (h + pad_t + pad_b) * (w + pad_l + pad_r)
    return [(0, F32, batch * channels * h * w), (1, F32, batch * channels * padded), (12, F32, noise_channels * padded)]


@spec("maua_bend_remap_f32", nullable=(10, 14, 15))
def _bend_remap(x, y, batch, channels, h, w, op, border, param, param_rows, field, field_frames, field_h, field_w, chan_mask, src):
    maps = batch * channels * h * w
    return [(0, F32, maps), (1, F32, maps), (8, F32, param_rows * 4), (10, F32, field_frames * 2 * field_h * field_w), (14, U8, channels),
            (15, U8, FRAME_SOURCE_BYTES)]


# ------------------------------------------------------------------------------------------------ the wrapper
def arity(name):
    """Arguments the spec of ``name`` takes: the entry's own, without the stream."""
    return len(inspect.signature(SPECS[name]).parameters)


def violations(name, args):
    """What is wrong with the operands of a call of ``name`` with ``args`` (strings; empty: the launch may go ahead)."""
    if name not in SPECS:
        return [f"{name}: no operand spec in tests/entry_specs.py"]
    if len(args) != arity(name):
        return [f"{name}: {len(args)} arguments, the spec takes {arity(name)}"]
    bad, named = [], {}
    for index, dtype, numel in SPECS[name](*args):
        named[index] = (dtype if isinstance(dtype, tuple) else (dtype,), int(numel))
    for index, a in enumerate(args):
        if isinstance(a, th.Tensor) and index not in named:
            bad.append(f"{name}: argument {index} is a tensor the spec does not name")
    for index, (dtypes, numel) in sorted(named.items()):
        a = args[index]
        if a is None:
            if index not in NULLABLE[name]:
                bad.append(f"{name}: argument {index} is None, the header does not allow NULL there")
        elif isinstance(a, th.Tensor):
            if a.dtype not in dtypes:
                bad.append(f"{name}: argument {index} is {a.dtype}, expected {' or '.join(str(d) for d in dtypes)}")
            if a.numel() < numel:
                bad.append(f"{name}: argument {index} has {a.numel()} elements, expected at least {numel}")
        elif not isinstance(a, (int, np.integer)):  # (an address the caller computed passes unchecked, as in _lib.call)
            bad.append(f"{name}: argument {index} is a {type(a).__name__}, expected a tensor")
    return bad


def checked_call(real_call):
    """A drop-in for ``_lib.call`` that forwards to ``real_call`` only what fits the entry's spec.  ``.launches`` counts the forwarded
    calls that returned, ``.refused`` the ones held back."""

    def call(name, *args, device=None):
        bad = violations(name, args)
        if bad:
            call.refused += 1
            raise AssertionError("; ".join(bad))
        real_call(name, *args, device=device)
        call.launches += 1

    call.launches = call.refused = 0
    return call
