"""Reference for the dense-transition hidden Markov model entries (csrc/hmm.hip: maua_hmm_viterbi_f64, maua_hmm_posterior_f64;
ar.viterbi, ar.hmm_posterior, ar.raw_chords): the definitions in include/maua_hip.h restated in numpy float64, loop for loop in the
defined order — the source walk of a target (i ascending) and the sums c_t (j ascending) are Python loops, only the independent
targets of one step are a numpy vector, which changes no operation and no order — brute-force enumeration for tiny models, four
deliberately wrong variants that the host test must catch, the shared case lists of the GPU test, and the synthetic chord clips and
the float64 chord chain of the feature tests."""
import itertools
import math

import numpy as np

MAX_STATES, MAX_FRAMES = 128, 1 << 22   # limits of include/maua_hip.h
VARIANTS = ("ties_high", "transposed", "no_init", "shifted_backptr")  # each one a plausible mistake; None is the definition


# ------------------------------------------------------------------------------------------------ the restatements
def viterbi(logobs, log_trans, log_init, variant=None):
    """(delta_last [S] float64, backptr [T, S] uint8, states [T] int32) of maua_hmm_viterbi_f64."""
    lo = np.asarray(logobs, np.float32).astype(np.float64)
    lt = np.asarray(log_trans, np.float64)
    li = np.asarray(log_init, np.float64)
    if variant == "transposed":
        lt = lt.T
    T, S = lo.shape
    with np.errstate(invalid="ignore"):
        delta = lo[0].copy() if variant == "no_init" else li + lo[0]
        back = np.zeros((T, S), np.uint8)
        back[0] = np.arange(S)
        for t in range(1, T):
            best = delta[0] + lt[0]
            idx = np.zeros(S, np.uint8)
            for i in range(1, S):
                cand = delta[i] + lt[i]
                take = cand >= best if variant == "ties_high" else cand > best   # False for a NaN on either side: nothing replaces
                best = np.where(take, cand, best)
                idx[take] = i
            delta = best + lo[t]
            back[t] = idx
        s, top = 0, delta[0]
        for k in range(1, S):
            if (delta[k] >= top) if variant == "ties_high" else (delta[k] > top):
                s, top = k, delta[k]
    if variant in CHUNK_VARIANTS:
        return delta, back, walk_back(back, s, variant)
    states = np.zeros(T, np.int32)
    states[T - 1] = s
    for t in range(T - 1, 0, -1):
        s = int(back[t - 1 if variant == "shifted_backptr" else t][s])
        states[t - 1] = s
    return delta, back, states


TRACE_ROWS = 1024   # HMM_TRACE_ROWS of csrc/hmm.hip: the frames of back pointers per chunk of the walk back
CHUNK_VARIANTS = ("chunk_repeat", "chunk_drop")  # wrong walks back that only more than one chunk shows (not in VARIANTS: T <= 6 there)


def chunks(T, rows=TRACE_ROWS, step=None):
    """The (lo, n) of every chunk of the kernel's walk back over T frames, last chunk first: hi = T - 1, lo = max(hi - (rows - 1), 0),
    n = hi - lo + 1, then hi -= rows (``step``: what a wrong kernel subtracts instead)."""
    out, hi = [], T - 1
    while hi >= 0:
        lo = max(hi - (rows - 1), 0)
        out.append((lo, hi - lo + 1))
        hi -= rows if step is None else step
    return out


def walk_back(back, s, variant=None):
    """states [T] int32 by the kernel's chunked walk from the final state ``s``.  None: the definition, whatever the chunking.
    chunk_repeat: the next chunk starts ON the row the last one ended with (hi -= rows - 1), which is then followed twice;
    chunk_drop: it starts one row too low (hi -= rows + 1), and the row between is neither followed nor written (it reads 0)."""
    T = back.shape[0]
    states = np.zeros(T, np.int32)
    step = {None: None, "chunk_repeat": TRACE_ROWS - 1, "chunk_drop": TRACE_ROWS + 1}[variant]
    for lo, n in chunks(T, step=step):
        for r in range(n - 1, -1, -1):
            states[lo + r] = s
            s = int(back[lo + r][s])   # (row 0 of backptr holds each state's own index)
    return states


def _chain(values):
    """acc = acc + v from 0.0 in ascending order, one float64 addition each."""
    acc = 0.0
    for v in values.tolist():
        acc = acc + v
    return acc


def posterior(obs, trans, init, variant=None):
    """(gamma [T, S], scale [T]) float64 of maua_hmm_posterior_f64."""
    ob = np.asarray(obs, np.float32).astype(np.float64)
    tr = np.asarray(trans, np.float64)
    ini = np.asarray(init, np.float64)
    if variant == "transposed":
        tr = tr.T
    T, S = ob.shape
    gamma, scale = np.zeros((T, S)), np.zeros(T)
    with np.errstate(invalid="ignore", divide="ignore"):
        for t in range(T):
            if t == 0:
                a = ob[0].copy() if variant == "no_init" else ini * ob[0]
            else:
                p = np.zeros(S)
                for i in range(S):
                    p = p + gamma[t - 1, i] * tr[i]
                a = p * ob[t]
            c = _chain(a)
            scale[t] = c
            gamma[t] = a / np.float64(c)
        beta = np.ones(S)
        for t in range(T - 2, -1, -1):
            u = ob[t + 1] * beta
            q = np.zeros(S)
            for j in range(S):
                q = q + tr[:, j] * u[j]
            beta = q / scale[t + 1]
            gamma[t] = gamma[t] * beta
    return gamma, scale


# ------------------------------------------------------------------------------------------------ brute force (S^T paths)
def brute_force(logobs, log_trans, log_init):
    """(best log-score, the paths that reach it, marginals [T, S], log-likelihood) by enumerating every path: math.fsum per path, so
    the figures are exact to the last bit or two and owe nothing to the recursions."""
    lo, lt, li = np.asarray(logobs, np.float64), np.asarray(log_trans, np.float64), np.asarray(log_init, np.float64)
    T, S = lo.shape
    scores = {}
    for path in itertools.product(range(S), repeat=T):
        terms = [li[path[0]], lo[0, path[0]]]
        for t in range(1, T):
            terms += [lt[path[t - 1], path[t]], lo[t, path[t]]]
        scores[path] = math.fsum(terms) if all(np.isfinite(terms)) else -math.inf
    top = max(scores.values())
    best = [p for p, v in scores.items() if v == top]
    total = math.fsum(math.exp(v) for v in scores.values())
    marg = np.zeros((T, S))
    for t in range(T):
        for s in range(S):
            marg[t, s] = math.fsum(math.exp(v) for p, v in scores.items() if p[t] == s) / total
    return top, best, marg, math.log(total)


# ------------------------------------------------------------------------------------------------ shared cases of the GPU test
STATES = (1, 2, 25, 64, 97, 128)
FRAMES = (1, 2, 3, 257, 2000)
VITERBI_KINDS = ("random", "integer", "neginf", "nan")
POSTERIOR_KINDS = ("random", "integer", "zeros", "nan", "zero_row")
LONG_CASE = dict(S=25, T=20000, kind="random", seed=77)


def cases(kinds):
    return [dict(S=S, T=T, kind=kind, seed=1000 * n + 10 * m + k) for k, kind in enumerate(kinds) for n, S in enumerate(STATES)
            for m, T in enumerate(FRAMES)]


def case_id(case):
    return f"{case['kind']}-S{case['S']}-T{case['T']}"


# (S, T) pairs, not a cross, on the edges the kernels compute: T = 1024 is one exactly full chunk of the walk back, 1025 leaves a last
# chunk of one row, 2048 is two full chunks, 2049 two and a row, 1023 and 2047 one row short of each; S = 63 / 65 put one dead / one
# live lane in the second wave, 127 is the largest S whose S | 1 stride equals S, 3 / 4 / 5 lie either side of the unroll-by-4 remainder.
# Both parities of T: the posterior's backward sweep alternates two buffers by frame parity.
EDGE_CASES = ((3, 1023), (4, 1024), (5, 1025), (63, 2047), (64, 1023), (65, 2048), (127, 2049), (128, 1024), (128, 1025), (128, 2048))
EDGE_VITERBI_KINDS = ("integer", "random")
EDGE_POSTERIOR_KINDS = ("integer", "zeros")
SWEEP_STATES = (1, 2, 3, 4, 5, 63, 64, 65, 127, 128)   # the wave and unroll edges the random-shape tests mix into their draws


def edge_cases(kinds):
    return [dict(S=S, T=T, kind=kind, seed=5000 + 10 * n + k) for k, kind in enumerate(kinds) for n, (S, T) in enumerate(EDGE_CASES)]


def _stochastic(rng, S):
    m = rng.random((S, S)) + 0.05
    m[np.arange(S), np.arange(S)] += 2.0
    return m / m.sum(1, keepdims=True)


def viterbi_operands(case):
    """(logobs float32 [T, S], log_trans float64 [S, S], log_init float64 [S]).  random: a sticky stochastic matrix and Gaussian
    log-likelihoods; integer: small integers everywhere, so every column holds ties and every sum is exact; neginf: a third of the
    transitions (never the diagonal) and of the initial states forbidden; nan: one NaN in the middle frame."""
    rng = np.random.default_rng(case["seed"])
    S, T, kind = case["S"], case["T"], case["kind"]
    if kind == "integer":
        return (rng.integers(-2, 1, (T, S)).astype(np.float32), rng.integers(-2, 1, (S, S)).astype(np.float64),
                rng.integers(-1, 1, S).astype(np.float64))
    logobs = (2.0 * rng.standard_normal((T, S))).astype(np.float32)
    log_trans = np.log(_stochastic(rng, S))
    init = rng.random(S) + 0.1
    log_init = np.log(init / init.sum())
    if kind == "neginf":
        forbid = rng.random((S, S)) < 1 / 3
        forbid[np.arange(S), np.arange(S)] = False
        log_trans[forbid] = -np.inf
        barred = rng.random(S) < 1 / 3
        barred[rng.integers(S)] = False
        log_init[barred] = -np.inf
    if kind == "nan":
        logobs[T // 2, S // 2] = np.nan
    return logobs, log_trans, log_init


def posterior_operands(case):
    """(obs float32 [T, S] >= 0, trans float64 [S, S], init float64 [S]).  random: likelihoods exp(2 N(0,1)) scaled to a row maximum
    of 1; integer: small integers (every product exact, the quotients are not); zeros: a third of the transitions (never the diagonal)
    zero — the counterpart of the -inf of the Viterbi cases; nan: one NaN in the middle frame; zero_row: the middle frame all zero."""
    rng = np.random.default_rng(case["seed"])
    S, T, kind = case["S"], case["T"], case["kind"]
    if kind == "integer":
        trans = rng.integers(0, 3, (S, S)).astype(np.float64)
        trans[np.arange(S), np.arange(S)] += 1.0
        return rng.integers(1, 4, (T, S)).astype(np.float32), trans, rng.integers(1, 3, S).astype(np.float64)
    logobs = 2.0 * rng.standard_normal((T, S))
    obs = np.exp(logobs - logobs.max(1, keepdims=True)).astype(np.float32)
    trans = _stochastic(rng, S)
    init = rng.random(S) + 0.1
    init = init / init.sum()
    if kind == "zeros":
        forbid = rng.random((S, S)) < 1 / 3
        forbid[np.arange(S), np.arange(S)] = False
        trans[forbid] = 0.0
        trans = trans / trans.sum(1, keepdims=True)
    if kind == "nan":
        obs[T // 2, S // 2] = np.nan
    if kind == "zero_row":
        obs[T // 2] = 0.0
    return obs, trans, init


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def same_bits_or_nan(a, b):
    """Bit for bit, except that a NaN matches any NaN: the payload and sign of a NaN that a division produces are not part of the
    definition (IEEE 754 leaves them open; the device's division sequence and the host's instruction choose differently)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    nan_a, nan_b = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(nan_a, nan_b)) and same_bits(np.where(nan_a, 0.0, a), np.where(nan_b, 0.0, b))


# ------------------------------------------------------------------------------------------------ chord clips (the feature tests)
SR = 22050
HOP = 512
NOTE = {"C": 0, "C#": 1, "D": 2, "D#": 3, "E": 4, "F": 5, "F#": 6, "G": 7, "G#": 8, "A": 9, "A#": 10, "B": 11}
QUALITIES = {"maj": (0, 4, 7), "min": (0, 3, 7), "7": (0, 4, 7, 10), "maj7": (0, 4, 7, 11), "min7": (0, 3, 7, 10), "dim": (0, 3, 6),
             "aug": (0, 4, 8), "sus4": (0, 5, 7)}
TRIAD_CLIP = (("C", "maj"), ("A", "min"), ("F", "maj"), ("G", "maj"), ("E", "min"), ("D", "min"))
SEVENTH_CLIP = (("C", "maj7"), ("A", "min7"), ("D", "min7"), ("G", "7"), ("B", "dim"), ("C", "sus4"))
CHORD_SECONDS, TAIL_SECONDS = 2.0, 1.0
EXEMPT_CHANGE, EXEMPT_START, TAIL_AFTER = 0.25, 0.1, 0.3
MAX_EXEMPT_SHARE = 0.25


def chord_clip(chords, transpose=0, clicks=True, tail=TAIL_SECONDS, seed=0):
    """The clip of the chord tests: every chord CHORD_SECONDS long, the notes of octave 3 (C3 = 130.81 Hz upwards from the root's pitch
    class) plus the root an octave below at 1.2 x amplitude, every note six partials at 0.6^h with a 20 ms attack and exp(-0.7 t)
    decay; ``tail`` seconds of silence behind; 10 ms noise clicks of amplitude 2.0 every 0.5 s."""
    n_chord = int(CHORD_SECONDS * SR)
    t = np.arange(n_chord) / SR
    env = np.minimum(t / 0.02, 1.0) * np.exp(-0.7 * t)
    c3 = 440.0 * 2.0 ** (-21 / 12)
    parts = []
    for root, quality in chords:
        pc = (NOTE[root] + transpose) % 12
        tones = [(c3 * 2.0 ** (((pc + step) % 12) / 12), 1.0) for step in QUALITIES[quality]] + [(c3 * 2.0 ** (pc / 12) / 2, 1.2)]
        y = np.zeros(n_chord)
        for f, amp in tones:
            for h in range(1, 7):
                y += amp * 0.6 ** h * np.sin(2 * np.pi * f * h * t)
        parts.append(y * env)
    y = np.concatenate(parts + [np.zeros(int(tail * SR))])
    if clicks:
        rng = np.random.default_rng(seed)
        width = SR // 100
        for at in np.arange(0.0, len(chords) * CHORD_SECONDS, 0.5):
            k = int(round(at * SR))
            y[k: k + width] += 2.0 * rng.standard_normal(width)
    return (y / np.abs(y).max() * 0.9).astype(np.float32)


def chord_truth(chords, names, transpose=0, tail=TAIL_SECONDS):
    """(want int [T], judged bool [T], tail bool [T]): the label every frame should have (N in the silence behind the chords), the
    frames that are judged — further than EXEMPT_CHANGE from a change, the end of the sound included, and past EXEMPT_START — and the
    frames later than TAIL_AFTER into the silence."""
    n = int((len(chords) * CHORD_SECONDS + tail) * SR)
    times = np.arange(1 + n // HOP) * HOP / SR
    end = len(chords) * CHORD_SECONDS
    which = np.minimum((times / CHORD_SECONDS).astype(int), len(chords) - 1)
    label = np.array([names.index(f"{list(NOTE)[(NOTE[r] + transpose) % 12]}:{q}") for r, q in chords])
    want = np.where(times < end, label[which], len(names) - 1)
    changes = np.arange(1, len(chords) + 1) * CHORD_SECONDS
    judged = (times >= EXEMPT_START) & (np.abs(times[:, None] - changes[None, :]).min(1) > EXEMPT_CHANGE)
    return want, judged, times > end + TAIL_AFTER


def rotate_labels(labels, n_states, by):
    """Chord labels (root-major blocks of 12, N last) with every root moved up ``by`` semitones."""
    labels = np.asarray(labels)
    chord = labels < n_states - 1
    return np.where(chord, labels // 12 * 12 + (labels % 12 + by) % 12, labels)
