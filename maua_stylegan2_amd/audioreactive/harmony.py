"""Chords and key on the MI355X: chord labels from a template likelihood behind a hidden Markov model, and the global key.  No
counterpart in the reference; librosa is not a dependency, the definitions are include/maua_hip.h ("Hidden Markov models with a dense
transition matrix"), tests/hmm_ref.py and DESIGN.md 4.21.

Pipeline of :func:`raw_chords`: the constant-Q chromagram of ``signal.raw_chroma(type="cqt")`` without its peak normalisation, CENS or
nearest-neighbour filter -> every frame's cosine against unit-norm binary chord templates (``signal.project``) -> ``kappa`` times that
as the log-likelihood of a frame given a chord, frames quieter than ``silence`` times the loudest one going to the no-chord state ``N``
-> the most probable path (maua_hmm_viterbi_f64) and the per-frame posteriors (maua_hmm_posterior_f64) of a chain that stays in its
chord for ``hold`` seconds on average and moves to every other state alike.  :func:`viterbi` and :func:`hmm_posterior` expose the two
decoders for any model of up to 128 states, as librosa.sequence does for librosa users.  Everything else is a handful of torch ops on
[frames, states].
"""
import math
import warnings

import numpy as np
import torch as th

from .. import _lib
from . import signal as _sig

__all__ = ["viterbi", "hmm_posterior", "chord_vocabulary", "raw_chords", "chords", "key", "ChordTrack", "CHORD_QUALITIES", "NOTE_NAMES",
           "HMM_MAX_STATES", "HMM_MAX_FRAMES"]

HMM_MAX_STATES = 128      # MAUA_HMM_MAX_STATES, MAUA_HMM_MAX_FRAMES (include/maua_hip.h)
HMM_MAX_FRAMES = 1 << 22

NOTE_NAMES = ("C", "C#", "D", "D#", "E", "F", "F#", "G", "G#", "A", "A#", "B")
CHORD_QUALITIES = {"maj": (0, 4, 7), "min": (0, 3, 7), "7": (0, 4, 7, 10), "maj7": (0, 4, 7, 11), "min7": (0, 3, 7, 10), "dim": (0, 3, 6),
                   "aug": (0, 4, 8), "sus4": (0, 5, 7)}
_VOCABULARIES = {"triads": ("maj", "min"), "sevenths": tuple(CHORD_QUALITIES)}

# Krumhansl & Kessler, "Tracing the dynamic changes in perceived tonal organization in a spatial representation of musical keys",
# Psychological Review 1982: probe-tone ratings of the twelve pitch classes against a major and a minor context, tonic first
KK_MAJOR = (6.35, 2.23, 3.48, 2.33, 4.38, 4.09, 2.52, 5.19, 2.39, 3.66, 2.29, 2.88)
KK_MINOR = (6.33, 2.68, 3.52, 5.38, 2.60, 3.53, 2.54, 4.75, 3.98, 2.69, 3.34, 3.17)


# ------------------------------------------------------------------------------------------------ the two decoders
def _check_shape(n_frames, n_states, what):
    if not 1 <= n_states <= HMM_MAX_STATES:
        raise ValueError(f"{what}: {n_states} states, the device decoders take 1 .. {HMM_MAX_STATES}")
    if not 1 <= n_frames <= HMM_MAX_FRAMES:
        raise ValueError(f"{what}: {n_frames} frames, the device decoders take 1 .. {HMM_MAX_FRAMES}: decode the clip in parts")


def _operands(frames, matrix, vector, what):
    """The three operands on the current device: frames [T, S] float32, matrix [S, S] and vector [S] float64."""
    frames, matrix, vector = (x if isinstance(x, th.Tensor) else np.asarray(x) for x in (frames, matrix, vector))
    if len(frames.shape) != 2:
        raise ValueError(f"{what}: the observations must be [frames, states] (got {tuple(frames.shape)})")
    n_frames, n_states = frames.shape
    _check_shape(n_frames, n_states, what)  # (before anything touches the device)
    if tuple(matrix.shape) != (n_states, n_states) or tuple(vector.shape) != (n_states,):
        raise ValueError(f"{what}: {n_states} states need a [{n_states}, {n_states}] transition matrix and {n_states} initial values "
                         f"(got {tuple(matrix.shape)} and {tuple(vector.shape)})")
    return _sig._to_dev(frames, th.float32), _sig._to_dev(matrix, th.float64), _sig._to_dev(vector, th.float64)


def viterbi(logobs, log_trans, log_init):
    """The most probable state path of a hidden Markov model: ``(states int32 [T], delta_last float64 [S])`` as device tensors.
    ``logobs`` [T, S] are the log-likelihoods of every frame under every state (computed in float32), ``log_trans`` [S, S] the
    log-probabilities of moving from state row to state column, ``log_init`` [S] those of the first state; tensors or arrays, -inf for
    what is forbidden.  Ties go to the lowest state.  ``delta_last.max()`` is the log-probability of the path up to what the rows of
    ``logobs`` leave out.  maua_hmm_viterbi_f64: S <= 128, T <= 2^22."""
    logobs, log_trans, log_init = _operands(logobs, log_trans, log_init, "viterbi")
    n_frames, n_states = logobs.shape
    dev = logobs.device
    delta_last = th.empty(n_states, dtype=th.float64, device=dev)
    backptr = th.empty((n_frames, n_states), dtype=th.uint8, device=dev)
    states = th.empty(n_frames, dtype=th.int32, device=dev)
    _lib.call("maua_hmm_viterbi_f64", logobs, log_trans, log_init, n_frames, n_states, delta_last, backptr, states)
    return states, delta_last


def _posterior(obs, trans, init):
    obs, trans, init = _operands(obs, trans, init, "hmm_posterior")
    n_frames, n_states = obs.shape
    gamma = th.empty((n_frames, n_states), dtype=th.float64, device=obs.device)
    scale = th.empty(n_frames, dtype=th.float64, device=obs.device)
    _lib.call("maua_hmm_posterior_f64", obs, trans, init, n_frames, n_states, gamma, scale)
    return gamma, scale


def hmm_posterior(obs, trans, init):
    """The probability of every state in every frame given ALL the observations: ``(gamma float64 [T, S] on the device, loglik)``.
    ``obs`` [T, S] are likelihoods >= 0 (not logarithms; any positive factor per frame is fine, ``exp(logobs - logobs.max(1))`` keeps
    them in range), ``trans`` [S, S] and ``init`` [S] probabilities.  ``loglik`` is the log-likelihood of the observations as given,
    a float.  Scaled forward-backward, maua_hmm_posterior_f64: S <= 128, T <= 2^22.  A frame whose likelihoods are all zero has no
    posterior: NaN from there on."""
    gamma, scale = _posterior(obs, trans, init)
    return gamma, float(scale.log().sum())


# ------------------------------------------------------------------------------------------------ the chord model
def chord_vocabulary(kind="triads"):
    """``(names, templates float32 [S, 12])``: unit-norm binary templates in root-major order per quality — ``C:maj ... B:maj,
    C:min ... B:min, ...`` — and last the no-chord state ``N`` with the flat template.  ``kind``: "triads" (maj, min: 25 states),
    "sevenths" (maj, min, 7, maj7, min7, dim, aug, sus4: 97 states) or an iterable of quality names from ``CHORD_QUALITIES``."""
    if isinstance(kind, str):
        if kind not in _VOCABULARIES:
            raise ValueError(f"chord_vocabulary: unknown kind {kind!r}: use 'triads', 'sevenths' or a list of qualities from {list(CHORD_QUALITIES)}")
        qualities = _VOCABULARIES[kind]
    else:
        qualities = tuple(kind)
        unknown = [q for q in qualities if q not in CHORD_QUALITIES]
        if unknown or not qualities or len(set(qualities)) != len(qualities):
            raise ValueError(f"chord_vocabulary: need distinct qualities from {list(CHORD_QUALITIES)} (got {list(qualities)})")
    names, rows = [], []
    for quality in qualities:
        for root in range(12):
            row = np.zeros(12)
            row[[(root + step) % 12 for step in CHORD_QUALITIES[quality]]] = 1.0
            names.append(f"{NOTE_NAMES[root]}:{quality}")
            rows.append(row / np.sqrt(row.sum()))
    names.append("N")
    rows.append(np.full(12, 1.0 / np.sqrt(12.0)))
    if len(names) > HMM_MAX_STATES:
        raise ValueError(f"chord_vocabulary: {len(names)} states, at most {HMM_MAX_STATES}")
    return names, np.asarray(rows, dtype=np.float32)


def silent_frames(energy, silence):
    """Frames whose energy (the sum of the unnormalised chroma) is at most ``silence`` times the clip's largest: bool [T]."""
    return energy <= silence * energy.max()


def unit_columns(chroma):
    """chroma [12, T] with every column scaled to Euclidean norm 1 (zero columns stay zero)."""
    norm = chroma.square().sum(0, keepdim=True).sqrt()
    return chroma / th.where(norm > 0, norm, th.ones_like(norm))


def chord_observations(cos, silent, kappa):
    """``logobs`` float32 [T, S] from the cosines [T, S] of the frames against the templates (``N`` last): ``kappa * cos``, and for a
    silent frame 0 everywhere and ``kappa`` at ``N``.  Plain torch, any device."""
    logobs = (float(kappa) * cos.float()).contiguous()
    quiet = th.zeros(cos.shape[1], dtype=th.float32, device=cos.device)
    quiet[-1] = float(kappa)
    return th.where(silent[:, None], quiet[None, :], logobs).contiguous()


def chord_transitions(n_states, frame_rate, hold):
    """``(log_trans [S, S], log_init [S])`` float64 arrays of a chain that stays with probability exp(-1 / (frame_rate hold)) — a mean
    stay of about ``hold`` seconds — moves to every other state alike, and starts anywhere."""
    if not (frame_rate > 0 and hold > 0):
        raise ValueError(f"chord_transitions: frame_rate and hold must be positive (got {frame_rate!r}, {hold!r})")
    stay = math.exp(-1.0 / (frame_rate * hold)) if n_states > 1 else 1.0
    trans = np.full((n_states, n_states), (1.0 - stay) / max(n_states - 1, 1), dtype=np.float64)
    np.fill_diagonal(trans, stay)
    return np.log(trans), np.full(n_states, -math.log(n_states), dtype=np.float64)


def likelihoods(logobs):
    """``exp(logobs - the row's maximum)`` float32 [T, S]: every row's largest likelihood is 1, so no frame sums to zero."""
    return (logobs - logobs.max(dim=1, keepdim=True).values).exp().contiguous()


def _audio(audio):
    return audio.detach().float().reshape(-1) if isinstance(audio, th.Tensor) else np.ascontiguousarray(audio, dtype=np.float32).reshape(-1)


def chromagram(audio, sr, margin=0, hop=512):
    """The unnormalised constant-Q chromagram [12, 1 + len / hop] on the device, row 0 = C: harmonic separation when ``margin`` is
    set, the tuning estimate, 7 octaves x 36 bins from C1 folded onto the pitch classes — ``raw_chroma(type="cqt")`` before its
    normalisation."""
    y = _audio(audio)
    if margin:
        y = _sig.harmonic(y, margin=margin)
    tuning = _sig.estimate_tuning(y, sr, bins_per_octave=36)
    return _sig.project(_sig.cq_to_chroma_matrix(), _sig.cqt_magnitude(y, sr, hop=hop, fmin=_sig.CQT_FMIN * 2.0 ** (tuning / 36)))


class ChordTrack:
    """What :func:`raw_chords` returns.  ``labels`` int32 [T]: the most probable chord sequence, indices into ``names`` (the last name
    is ``N``, no chord); ``times`` float64 numpy [T]: the frames' centres in seconds; ``posterior`` float32 [T, S]: every chord's
    probability per frame given the whole clip; ``confidence`` float32 [T]: the posterior of the decoded label.  Tensors are on the
    device."""

    def __init__(self, labels, names, times, posterior, confidence):
        self.labels, self.names, self.times, self.posterior, self.confidence = labels, names, times, posterior, confidence

    def __len__(self):
        return int(self.labels.shape[0])

    def segments(self):
        """[(start seconds, end seconds, name)] of the runs of equal labels."""
        lab = self.labels.cpu().numpy()
        cuts = [0] + (1 + np.flatnonzero(lab[1:] != lab[:-1])).tolist() + [len(lab)]
        step = float(self.times[1] - self.times[0]) if len(lab) > 1 else 0.0
        return [(float(self.times[a]), float(self.times[b - 1]) + step, self.names[int(lab[a])]) for a, b in zip(cuts[:-1], cuts[1:])]


def _chord_stages(audio, sr, vocabulary="triads", kappa=20.0, hold=1.0, margin=0, silence=0.02, hop=512):
    """Every intermediate of :func:`raw_chords` (the link-by-link test reads them)."""
    if not sr > 0:
        raise ValueError(f"sr must be positive (got {sr!r})")
    if not (kappa > 0 and math.isfinite(kappa)):
        raise ValueError(f"raw_chords: kappa must be positive and finite (got {kappa!r})")
    if not 0 <= silence < 1:
        raise ValueError(f"raw_chords: silence must lie in [0, 1) (got {silence!r})")
    names, templates = chord_vocabulary(vocabulary)
    n_states = len(names)
    log_trans, log_init = chord_transitions(n_states, float(sr) / hop, hold)
    chroma = chromagram(audio, sr, margin, hop)
    n_frames = chroma.shape[1]
    _check_shape(n_frames, n_states, "raw_chords")
    energy = chroma.sum(0)
    silent = silent_frames(energy, silence)
    cos = _sig.project(templates, unit_columns(chroma).contiguous()).t()
    logobs = chord_observations(cos, silent, kappa)
    obs = likelihoods(logobs)
    states, delta_last = viterbi(logobs, log_trans, log_init)
    gamma, scale = _posterior(obs, np.exp(log_trans), np.exp(log_init))
    posterior = gamma.float()
    confidence = posterior.gather(1, states.long()[:, None])[:, 0]
    return dict(names=names, templates=templates, log_trans=log_trans, log_init=log_init, chroma=chroma, energy=energy, silent=silent,
                cos=cos, logobs=logobs, obs=obs, labels=states, delta_last=delta_last, gamma=gamma, scale=scale, posterior=posterior,
                confidence=confidence, times=np.arange(n_frames, dtype=np.float64) * hop / float(sr))


def raw_chords(audio, sr, vocabulary="triads", kappa=20.0, hold=1.0, margin=0, silence=0.02, hop=512):
    """The chords of a clip per analysis frame, a :class:`ChordTrack` (labels, names, times, posterior, confidence) at sr / ``hop``
    frames per second, T = 1 + len / hop.  ``vocabulary``: what :func:`chord_vocabulary` takes.  ``kappa``: how sharply a frame prefers
    the template it resembles (log-likelihood = kappa cos).  ``hold``: the mean time in seconds the chain stays in a chord; longer
    means fewer, later changes.  ``margin``: harmonic separation before the chromagram, off by default — unlike ``ar.chroma`` — because
    it thins the partials that tell a seventh or a suspended chord from a triad.  ``silence``: frames whose chroma
    energy is at most this share of the loudest frame's are ``N``; the chromagram of a decaying tail is not zero and would decode to
    arbitrary chords."""
    s = _chord_stages(audio, sr, vocabulary, kappa, hold, margin, silence, hop)
    return ChordTrack(s["labels"], s["names"], s["times"], s["posterior"], s["confidence"])


# ------------------------------------------------------------------------------------------------ features per video frame
def chord_rows(labels, posterior, n_states, by="root", soft=False):
    """One row per analysis frame, float32 [T, 12] (``by="root"``: the chord's root, qualities merged) or [T, S - 1]
    (``by="chord"``): one-hot rows of the path, or with ``soft`` the posterior without ``N`` (summed over the qualities for "root").
    Frames labelled ``N`` (index S - 1) hold the row of the last chord before them, leading ones take the first chord's.  None when
    every frame is ``N``.  Plain torch, any device."""
    if by not in ("root", "chord"):
        raise ValueError(f"chords: unknown by={by!r}: use 'root' or 'chord'")
    n_chords = n_states - 1
    if n_chords < 1 or n_chords % 12:
        raise ValueError(f"chords: {n_states} states are not 12 roots per quality and N")
    labels = labels.long()
    sounding = labels < n_chords
    at = _sig.hold_fill(th.arange(labels.shape[0], device=labels.device), sounding)
    if at is None:
        return None
    if soft:
        rows = posterior[:, :n_chords].float()
    else:
        rows = th.zeros((labels.shape[0], n_chords), dtype=th.float32, device=labels.device)
        rows[sounding, labels[sounding]] = 1.0
    rows = rows[at]
    return rows.reshape(rows.shape[0], -1, 12).sum(1) if by == "root" else rows


def rotate_roots(rows, tonic):
    """Columns rotated so that column 0 (of every block of 12) is the pitch class ``tonic``: new[:, k] = old[:, (k + tonic) % 12]."""
    shape = rows.shape
    return th.roll(rows.reshape(shape[0], -1, 12), -int(tonic) % 12, dims=2).reshape(shape)


def chords(audio, sr, n_frames, by="root", soft=False, smooth=2, relative_to=None, device=None, track=None, **raw):
    """Chord weights per video frame, float32 [n_frames, 12] (``by="root"``) or [n_frames, S - 1] (``by="chord"``), rows summing to 1,
    a CPU tensor unless ``device=`` is given: what ``ar.chroma_weight_latents`` takes — one latent per root or per chord, switching
    where the chord changes.  :func:`raw_chords` (its arguments pass through; ``track=`` reuses a result) -> :func:`chord_rows` ->
    Fourier resampling to ``n_frames`` -> Gaussian smoothing when ``smooth`` > 0 -> clamped at 0 (the resampling rings on steps) and
    renormalised.  ``relative_to``: a tonic 0 .. 11, or "key" for that of :func:`key`: the root columns are rotated so that column 0 is
    the tonic and the same latent is "home" in every song.  A clip without a chord gives uniform rows and a warning."""
    if track is None:
        track = raw_chords(audio, sr, **raw)
    n_states = len(track.names)
    rows = chord_rows(track.labels, track.posterior, n_states, by, soft)
    if rows is None:
        warnings.warn("chords: no frame of the clip holds a chord; returning uniform rows", stacklevel=2)
        width = 12 if by == "root" else n_states - 1
        out = th.full((int(n_frames), width), 1.0 / width, dtype=th.float32, device=track.labels.device)
        return out.to(device if device is not None else "cpu")
    if relative_to is not None:
        tonic = key(audio, sr, margin=raw.get("margin", 0))[0] if isinstance(relative_to, str) and relative_to == "key" else relative_to
        if isinstance(tonic, str) or not 0 <= int(tonic) <= 11:
            raise ValueError(f"chords: relative_to must be a tonic 0 .. 11 or 'key' (got {relative_to!r})")
        rows = rotate_roots(rows, int(tonic))
    out = _sig.resample(rows, n_frames).float()
    if smooth > 0:
        out = _sig.gaussian_filter(out, smooth)
    out = out.clamp(min=0)
    total = out.sum(1, keepdim=True)
    out = th.where(total > 0, out / th.where(total > 0, total, th.ones_like(total)), th.full_like(out, 1.0 / out.shape[1]))
    return out.to(device if device is not None else "cpu")


def key_of_chroma(mean_chroma):
    """``(tonic, mode, name, scores [24])`` of a mean chroma vector [12] (row 0 = C): the Krumhansl-Kessler profile, rotated to each
    tonic, with the highest Pearson correlation; scores 0 .. 11 are the major keys by tonic, 12 .. 23 the minor ones, and the lowest
    index wins ties.  Plain torch in float64, any device."""
    x = mean_chroma.double().reshape(12)
    profiles = np.stack([np.roll(p, k) for p in (KK_MAJOR, KK_MINOR) for k in range(12)])
    prof = th.from_numpy(profiles).to(x.device)
    xc, pc = x - x.mean(), prof - prof.mean(1, keepdim=True)
    denom = xc.square().sum().sqrt() * pc.square().sum(1).sqrt()
    scores = th.where(denom > 0, (pc * xc).sum(1) / th.where(denom > 0, denom, th.ones_like(denom)), th.zeros_like(denom)).cpu()
    best = 0
    for k in range(1, 24):
        if float(scores[k]) > float(scores[best]):
            best = k
    tonic, mode = best % 12, ("major", "minor")[best // 12]
    return tonic, mode, f"{NOTE_NAMES[tonic]} {mode}", scores


def key(audio, sr, margin=0):
    """The key of a clip, ``(tonic 0 .. 11, "major" | "minor", name)``: the Krumhansl-Kessler profile with the highest Pearson
    correlation to the clip's mean unnormalised chroma (:func:`chromagram`; ``margin`` as there).  A GLOBAL estimate: one key for the
    whole clip, which a modulation blurs.  Tracking the key over time is out of scope (windowed versions of this
    wander to the dominant and back)."""
    return key_of_chroma(chromagram(audio, sr, margin).mean(1))[:3]
