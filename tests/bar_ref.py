"""Reference for the bar-pointer decoder (csrc/bar.hip: maua_bar_viterbi_f64; ar.bar_viterbi, ar.raw_bars): the definition in
include/maua_hip.h ("Bar-pointer model") restated in numpy float64, operation for operation in the defined order — the prefix sums
are Python chains, the source walk of an entry (k' ascending) is a Python loop, only the independent lanes (k, b) of one frame are
a numpy vector, which changes no operation and no order.  Five deliberately wrong variants that the host test must tell apart on the
GPU test's own case list, the expansion of a model to the dense matrix of hmm_ref.viterbi, that case list, and the click envelopes
and clips of the known-answer and feature tests."""
import numpy as np

import pulse_ref

MAX_FRAMES, MAX_TEMPI, MAX_BEATS, MAX_INTERVAL, MAX_MODELS, MAX_LANES = 1 << 22, 128, 8, 1024, 8, 1024   # include/maua_hip.h
LDS_LIMIT = 160 * 1024
VARIANTS = ("ring_off", "j_le_width", "no_wrap", "ties_high", "unclipped")   # each one a plausible wrong kernel; None is the definition


def lds_bytes(n_tempi, max_beats, max_interval):
    """maua_bar_lds_bytes restated: the matrix at a row stride of K | 1 doubles, two buffers of exit values, a ring of max_interval
    entry values per lane; 0 where that is more than one CU has."""
    if not (1 <= n_tempi <= MAX_TEMPI and 1 <= max_beats <= MAX_BEATS and 1 <= max_interval <= MAX_INTERVAL and n_tempi * max_beats <= MAX_LANES):
        return 0
    lanes = n_tempi * max_beats
    n = 8 * (n_tempi * (n_tempi | 1) + 2 * lanes + lanes * max_interval)
    n = (n + 15) // 16 * 16
    return n if n <= LDS_LIMIT else 0


def prefix_sums(logobs):
    """P [3, T + 1] float64: P[c][0] = 0, P[c][n + 1] = P[c][n] + logobs[n][c], one addition each in ascending n."""
    lo = np.asarray(logobs, np.float32).astype(np.float64)
    T = lo.shape[0]
    P = np.zeros((3, T + 1))
    with np.errstate(invalid="ignore"):
        for c in range(3):
            acc = 0.0
            col = lo[:, c].tolist()
            for n in range(T):
                acc = acc + col[n]
                P[c, n + 1] = acc
    return P


def _pick(P, c, at, lo0, unclipped):
    """P[c][at] for index vectors; ``unclipped``: an index below 0 is not clipped but read as if frame 0 repeated before the clip."""
    if not unclipped:
        return P[c, np.maximum(at, 0)]
    return np.where(at < 0, at * lo0[c], P[c, np.maximum(at, 0)])


def _segment(P, e, width, col, end, lo0, variant):
    """The observations of a beat entered at frame e (per lane) over the frames [max(e, 0), end): (P_c[a1] - P_c[a0]) + (P_0[end] -
    P_0[a1]) with a0 = max(e, 0), a1 = min(max(e + width, 0), end)."""
    unclipped = variant == "unclipped"
    a0 = e if unclipped else np.maximum(e, 0)
    a1 = np.minimum(e + width if unclipped else np.maximum(e + width, 0), end)
    with np.errstate(invalid="ignore"):
        beat = _pick(P, col, a1, lo0, unclipped) - _pick(P, col, a0, lo0, unclipped)
        rest = P[0, end] - _pick(P, np.zeros_like(col), a1, lo0, unclipped)
        return beat + rest


def viterbi(logobs, interval, width, log_change, beats, variant=None):
    """(score float64, path [T, 3] int32) of one model of maua_bar_viterbi_f64."""
    lo = np.asarray(logobs, np.float32).astype(np.float64)
    I = np.asarray(interval, np.int64)
    W = np.asarray(width, np.int64)
    if variant == "j_le_width":
        W = np.minimum(W + 1, I)   # the beat columns for j = 0 .. width, where the beat is that long
    lc = np.asarray(log_change, np.float64)
    T, K, B = lo.shape[0], len(I), int(beats)
    L = K * B
    P = prefix_sums(lo)
    lo0 = lo[0]
    kk, bb = np.repeat(np.arange(K), B), np.tile(np.arange(B), K)          # lane = k * B + b
    Il, Wl = I[kk], W[kk]
    col = np.where(bb == 0, 2, 1)
    src_b = bb - 1 if variant == "no_wrap" else (bb - 1) % B              # (no_wrap: lane index k' * B - 1 for b = 0)
    V = np.zeros((T + 1, L))                                               # V[e] for e >= 1; every entry at a frame <= 0 is worth 0
    back = np.zeros((T, L), np.uint8)
    shift = 1 if variant == "ring_off" else 0
    with np.errstate(invalid="ignore"):
        for t in range(1, T):
            e = t - Il
            X = np.where(e + shift >= 1, V[np.clip(e + shift, 0, T), np.arange(L)], 0.0) + _segment(P, e, Wl, col, t, lo0, variant)
            best = X[(0 * B + src_b) % L] + lc[0][kk]
            arg = np.zeros(L, np.uint8)
            for k in range(1, K):
                cand = X[(k * B + src_b) % L] + lc[k][kk]
                take = cand >= best if variant == "ties_high" else cand > best
                best = np.where(take, cand, best)
                arg[take] = k
            V[t] = best
            back[t] = arg
        # the last frame: every state (k, b, j), entered at e = T - 1 - j; the first maximum in ascending (k, b, j), from -inf
        top, final = -np.inf, (0, 0, 0)
        for lane in range(L):
            k, b = int(kk[lane]), int(bb[lane])
            j = np.arange(I[k])
            e = T - 1 - j
            vals = np.where(e >= 1, V[np.clip(e, 0, T), lane], 0.0) + _segment(P, e, np.full(len(j), Wl[lane]), np.full(len(j), col[lane]), T, lo0, variant)
            for jj, v in enumerate(vals.tolist()):
                if (v >= top and variant == "ties_high") or v > top:
                    top, final = v, (k, b, jj)
    path = np.zeros((T, 3), np.int32)
    k, b, j = final
    t = T - 1
    while True:
        e = t - j
        for f in range(max(e, 0), t + 1):
            path[f] = (k, b, f - e)
        if e <= 0:
            break
        k = int(back[e, k * B + b])
        b = (b - 1) % B
        j = int(I[k]) - 1
        t = e - 1
    return np.float64(top), path


def decode(logobs, interval, width, log_change, beats_per_bar, variant=None):
    """(score [n_models], path [n_models, T, 3]) of one call."""
    out = [viterbi(logobs, interval, width, log_change, B, variant) for B in beats_per_bar]
    return np.array([s for s, _ in out], np.float64), np.stack([p for _, p in out])


# ------------------------------------------------------------------------------------------------ the dense model
def expand(interval, width, log_change, beats):
    """(log_trans [S, S], log_init [S], column [S], states [S, 3]) of the model with every state (k, b, j) written out in ascending
    (k, b, j): the operands of hmm_ref.viterbi, whose observations are logobs[:, column]."""
    I, W, lc = np.asarray(interval, np.int64), np.asarray(width, np.int64), np.asarray(log_change, np.float64)
    states = [(k, b, j) for k in range(len(I)) for b in range(beats) for j in range(I[k])]
    index = {s: n for n, s in enumerate(states)}
    S = len(states)
    lt = np.full((S, S), -np.inf)
    for (k, b, j), n in index.items():
        if j > 0:
            lt[index[(k, b, j - 1)], n] = 0.0
        else:
            for k2 in range(len(I)):
                lt[index[(k2, (b - 1) % beats, int(I[k2]) - 1)], n] = lc[k2, k]
    column = np.array([(2 if b == 0 else 1) if j < W[k] else 0 for k, b, j in states])
    return lt, np.zeros(S), column, np.array(states, np.int32)


def dense_score(logobs, lt, column, states, path):
    """(the path's log-probability under the dense model by a plain chain, the sum of the magnitudes of its terms)."""
    lo = np.asarray(logobs, np.float32).astype(np.float64)
    index = {tuple(s): n for n, s in enumerate(states.tolist())}
    seq = [index[tuple(p)] for p in np.asarray(path).tolist()]
    acc, mag = lo[0, column[seq[0]]], abs(lo[0, column[seq[0]]])
    for t in range(1, len(seq)):
        for term in (lt[seq[t - 1], seq[t]], lo[t, column[seq[t]]]):
            acc, mag = acc + term, mag + abs(term)
    return acc, mag


# ------------------------------------------------------------------------------------------------ cases
DENSE_CASES = [([2, 3], 2, 1), ([2, 3], 2, 2), ([2, 3], 2, 40), ([3, 4, 5, 7], 3, 1), ([3, 4, 5, 7], 3, 5), ([3, 4, 5, 7], 3, 97),
               ([5], 1, 23), ([4, 9], 4, 64), ([1, 2], 3, 30), ([6, 7, 8], 5, 200)]


def random_operands(intervals, T, seed=0, widths="random", matrix="dirichlet", obs="normal"):
    """(logobs fp32 [T, 3], interval, width, log_change) of a case: random widths in 1 .. interval, Dirichlet rows with an occasional
    -inf, observations 3 N(0, 1) rounded to fp32; ``matrix`` / ``obs`` name the other kinds below."""
    rng = np.random.default_rng(seed)
    I = np.asarray(intervals, np.int32)
    K = len(I)
    W = np.array([rng.integers(1, i + 1) for i in I], np.int32)
    if widths == "full":
        W = I.copy()
    rows = rng.dirichlet(np.ones(K), K)
    with np.errstate(divide="ignore"):
        lc = np.log(rows)
        if K > 1:
            lc[rng.random((K, K)) < 0.1] = -np.inf
            lc[np.arange(K), np.arange(K)] = np.log(rows[np.arange(K), np.arange(K)])
    if matrix == "uniform":
        lc = np.zeros((K, K))
    if matrix == "forbidden_column":
        lc[:, K // 2] = -np.inf
    lo = (3.0 * rng.standard_normal((T, 3))).astype(np.float32)
    if obs == "zeros":
        lo[:] = 0
    if obs == "integer":
        lo = rng.integers(-2, 1, (T, 3)).astype(np.float32)
    if obs == "nan":
        lo[T // 2, 1] = np.nan
    if obs == "inf":
        lo[T // 3, 2] = np.inf
    if matrix == "integer":   # small integers: with obs="integer" every sum is exact, whatever its order (drawn last: the other kinds keep their draws)
        lc = rng.integers(-3, 1, (K, K)).astype(np.float64)
    return lo, I, W, lc


def default_model(fr=pulse_ref.FR):
    from maua_stylegan2_amd.audioreactive import bars

    return bars.bar_model(fr)


def _case(name, intervals, beats, T, **kw):
    return dict(name=name, intervals=None if intervals is None else list(intervals), beats=tuple(beats), T=T, kw=kw)


def gpu_cases():
    """The case list of tests/test_bar_gpu.py (and of the variant test of tests/test_bar_host.py)."""
    cases = [_case(f"dense-{'_'.join(map(str, iv))}-B{B}-T{T}", iv, (B,), T) for iv, B, T in DENSE_CASES]
    edge = [5, 6, 9]                                 # interval[0] - 1 = 4, interval[-1] = 9, interval[-1] + 1 = 10 (the first ring wrap)
    cases += [_case(f"edge-T{T}", edge, (3,), T, seed=T) for T in (1, 2, 4, 9, 10)]
    cases += [_case("K1-B1", [4], (1,), 37, seed=3), _case("interval-1", [1, 2, 4], (2,), 50, seed=4),
              _case("only-interval-1", [1], (3,), 20, seed=14),
              _case("width-full", [3, 5, 6], (3,), 60, seed=5, widths="full"),
              _case("lanes-63", range(2, 11), (7,), 70, seed=6), _case("lanes-64", range(2, 10), (8,), 70, seed=7),
              _case("lanes-65", range(2, 15), (5,), 70, seed=8),
              _case("forbidden-column", [3, 4, 5, 6, 7], (4,), 120, seed=9, matrix="forbidden_column"),
              _case("all-ties", [2, 3, 4, 5], (4,), 60, seed=10, matrix="uniform", obs="zeros"),
              _case("integer-ties", [2, 3, 4, 5], (3,), 90, seed=15, matrix="uniform", obs="integer"),
              _case("nan", [3, 4, 5], (3,), 40, seed=11, obs="nan"), _case("inf", [3, 4, 5], (3,), 40, seed=12, obs="inf"),
              _case("three-models", [3, 4, 6, 7], (1, 4, 8), 150, seed=13),
              _case("default-40s", None, (3, 4), 1723, seed=16),
              _case("limit-tempi", range(1, 101), (1,), 120, seed=17),       # K = 100, B = 1: 158.6 KiB, the most tempi one CU holds
              _case("limit-beats", range(1, 41), (8,), 90, seed=18)]         # 320 lanes, B = 8: 120 KiB
    return cases


def case_operands(case):
    if case["intervals"] is None:
        interval, width, lc = default_model()
        lo = random_operands([1], case["T"], case["kw"].get("seed", 0))[0]
        return lo, interval.astype(np.int32), width.astype(np.int32), lc
    return random_operands(case["intervals"], case["T"], **case["kw"])


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


# ------------------------------------------------------------------------------------------------ envelopes and clips
FR = pulse_ref.FR
KNOWN_CLIPS = [(120.0, 4), (90.0, 3), (133.0, 4), (171.0, 3), (70.0, 4)]     # 20 s each, the accent on every B-th click


def observations(beat_act, down_act, observation_lambda=16):
    """float64 restatement of ar.bar_observations, rounded to fp32 once."""
    a = np.clip(np.asarray(beat_act, np.float64), 1e-3, 1 - 1e-3)
    d = np.clip(np.asarray(down_act, np.float64), 0.05, 0.95)
    return np.stack([np.log((1 - a) / (observation_lambda - 1)), np.log(a * (1 - d)), np.log(a * d)], 1).astype(np.float32)


def accented_envelope(times, every, duration, fr=FR, first=0):
    """(beat_act, down_act, n): the click envelope of ``times`` with its peak scaled to 0.9, and a downbeat activation of 0.8 on the two
    frames round every ``every``-th click (from click ``first``), 0.2 round the other clicks, 0.5 elsewhere."""
    n = 1 + int(duration * pulse_ref.SR) // pulse_ref.HOP
    env = pulse_ref.click_envelope(times, n, fr).astype(np.float64)
    env = env / env.max() * 0.9
    d = np.full(n, 0.5)
    for i, t in enumerate(times):
        lo = int(np.floor(t * fr))
        d[max(lo, 0): lo + 2] = 0.8 if (i - first) % every == 0 else 0.2
    return env, d, n


def accented_clip(times, every, duration, seed=0, sr=pulse_ref.SR):
    """Audio: 10 ms bursts of white noise at ``times`` in silence (the clip of tests/test_pulse_features_gpu.py); every ``every``-th
    one, from the first, also starts a 60 Hz thump that decays with exp(-t / 50 ms) over 0.25 s."""
    rng = np.random.default_rng(seed)
    y = np.zeros(int(duration * sr), np.float64)
    t = np.arange(int(0.25 * sr)) / sr
    thump = 0.8 * np.sin(2 * np.pi * 60.0 * t) * np.exp(-t / 0.05)
    for i, at_s in enumerate(times):
        at = int(round(at_s * sr))
        n = min(sr // 100, len(y) - at)
        y[at: at + n] += 0.5 * rng.standard_normal(n)
        if i % every == 0:
            n = min(len(thump), len(y) - at)
            y[at: at + n] += thump[:n]
    return y.astype(np.float32)


AUDIO_CLIPS = {"120-4": (120.0, 4, 20.0), "90-3": (90.0, 3, 20.0), "switch-4": (None, 4, 40.0)}   # name -> (BPM, accent every, seconds)


def audio_clip(name):
    """(audio, click times, accent every, seconds, clear) of a clip of the feature tests; ``clear`` marks the clicks that are judged:
    further than 1 s from both ends of the clip and from the tempo switch."""
    bpm, every, seconds = AUDIO_CLIPS[name]
    times = pulse_ref.click_times(bpm, seconds) if bpm else np.concatenate(pulse_ref.switch_times(seconds, seconds / 2))
    clear = (times > 1.0) & (times < seconds - 1.0) & ((np.abs(times - seconds / 2) > 1.0) if bpm is None else True)
    return accented_clip(times, every, seconds), times, every, seconds, clear


def rank_percentile(x, p):
    ordered = np.sort(np.asarray(x).reshape(-1))
    return ordered[round(0.01 * p * (len(ordered) - 1))]


def activations_from_power(power, mel, edges_hz, lag_pad=3):
    """float64 restatement of the activations of ar.raw_bars from a power spectrogram [bins, N], a mel filterbank [128, bins] and the
    centre frequencies of its bands: (beat_act, down_act)."""
    def flux(fb, floor):
        db = 10 * np.log10(np.maximum(1e-10, fb @ power))
        db = np.maximum(db, db.max() - floor)
        return np.maximum(db[:, 1:] - db[:, :-1], 0)

    n = power.shape[1]
    onset = np.concatenate([np.zeros(lag_pad), np.median(flux(mel, 80.0), axis=0)])[:n]
    cue = np.concatenate([np.zeros(lag_pad), flux(mel[edges_hz < 200.0], 40.0).sum(0)])[:n]
    a = np.clip(onset / rank_percentile(onset[onset > 0], 90), 0, 1)
    pad = np.concatenate([cue[:1], cue, cue[-1:]])
    cue = np.maximum(np.maximum(pad[:-2], pad[1:-1]), pad[2:])
    return a, 0.05 + 0.9 * np.clip(cue / rank_percentile(cue[a > 0.1], 90), 0, 1)


def judge_events(beats, downs, clicks, every, clear, tol):
    """(every clear click has exactly one beat within tol and no other beat lies between the clear clicks' neighbours, worst beat
    offset, every clear accent has exactly one downbeat within tol and every downbeat near a clear click is on an accent, worst
    downbeat offset) in seconds."""
    beats, downs, clicks = np.asarray(beats), np.asarray(downs), np.asarray(clicks)
    accents, accent_clear = clicks[::every], clear[::every]
    worst = worst_down = 0.0
    beats_ok = downs_ok = True
    for t in clicks[clear]:
        near = np.abs(beats - t)
        beats_ok &= int((near <= tol).sum()) == 1
        worst = max(worst, float(near.min()) if len(near) else np.inf)
    for t in accents[accent_clear]:
        near = np.abs(downs - t)
        downs_ok &= int((near <= tol).sum()) == 1
        worst_down = max(worst_down, float(near.min()) if len(near) else np.inf)
    for t in downs:   # a downbeat on a clear click that is not an accent is a wrong bar line
        owner = int(np.abs(clicks - t).argmin())
        if clear[owner] and abs(clicks[owner] - t) <= tol:
            downs_ok &= owner % every == 0
    for t in beats:   # a beat whose nearest click is a clear one lies on it: no extra beats between the clicks
        owner = int(np.abs(clicks - t).argmin())
        if clear[owner]:
            beats_ok &= abs(clicks[owner] - t) <= tol
    return bool(beats_ok), worst, bool(downs_ok), worst_down


def path_events(path, fr=FR):
    """(beat times, downbeat times) in seconds of a decoded path: the frames with j == 0, and those of them with b == 0, over fr."""
    path = np.asarray(path)
    beat = np.flatnonzero(path[:, 2] == 0)
    return beat / fr, beat[path[beat, 1] == 0] / fr


def match(found, truth):
    """(count of truths with exactly one found event nearest to them, worst offset in seconds) of two time lists."""
    found, truth = np.asarray(found, np.float64), np.asarray(truth, np.float64)
    if len(found) == 0:
        return 0, np.inf
    owner = np.abs(found[:, None] - truth[None, :]).argmin(1)
    exactly_one = sum(int((owner == i).sum() == 1) for i in range(len(truth)))
    worst = max(np.abs(found - truth[owner]).max(), np.abs(found[:, None] - truth[None, :]).min(0).max())
    return exactly_one, float(worst)
