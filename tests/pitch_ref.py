"""Reference for the pitch tracker (csrc/pitch.hip, maua_yin_f32): the definition in include/maua_hip.h restated in float64 numpy, an
all-float32 emulation of it (every operand and intermediate rounded to fp32, the running sum included, one lag summed over j in order),
the comparison helper the GPU test uses, the shared case lists, and the host side of ``ar.pitch`` (steps 4-8) in numpy.

    PYTHONPATH=. python tests/pitch_ref.py

prints, without a GPU, the emulation's worst error against float64 over the GPU case list — one figure per output — from which the
tolerances below are derived (4 x the figure, rounded up to two digits; never taken from the kernel)."""
import math

import numpy as np

# Measured by `python tests/pitch_ref.py`: the fp32 emulation against float64 over gpu_cases(), lag / aperiodicity on the unambiguous
# frames.  Tolerance = 4 x the figure, rounded up to two digits.  Main list (frame > tau_max), absolute:
CMNDF_TOL = 2.7e-5           # 4 x 6.54e-6   worst |d' fp32 - d' fp64|
LAG_TOL = 1.7e-3             # 4 x 4.19e-4   samples (a 694-sample period under a broad minimum: 0.004 cents)
APERIODICITY_TOL = 2.3e-6    # 4 x 5.61e-7
# SHORT_WINDOW cases (frame <= tau_max, exact signals): d' and aperiodicity errors divided by max(1, |reference|)
SHORT_CMNDF_TOL = 2.4e-7     # 4 x 5.85e-8
SHORT_LAG_TOL = 1.3e-5       # 4 x 3.17e-6
SHORT_APERIODICITY_TOL = 1.5e-7  # 4 x 3.69e-8
# ar.pitch on the arpeggio, every stage (YIN and steps 4-8) in fp32 against float64:
PIPELINE_HEIGHT_TOL = 1.7e-7   # 4 x 4.24e-8
PIPELINE_VOICING_TOL = 2.4e-6  # 4 x 5.97e-7

# known answers (tests/test_pitch_host.py): worst error of the float64 definition over tone_cases(), interior frames
REF_WORST_CENTS = 1.937      # measured, on the 1318.5 Hz sine (aperiodicity <= 0.0073); the fp32 emulation gives the same 1.937
CENTS_BOUND = 2.91           # 1.5 x 1.937, rounded up (the margin is for a different libm)
APERIODICITY_BOUND = 0.011   # 1.5 x 0.0073, the worst aperiodicity measured on the same frames
TONE_SR, TONE_FRAME, TONE_HOP, TONE_TAU_MIN, TONE_TAU_MAX, TONE_THRESHOLD = 22050, 2048, 512, 10, 340, 0.1
TONE_FREQS = (70.0, 82.41, 110.0, 220.0, 261.63, 440.0, 659.25, 880.0, 1318.5)
TONE_KINDS = ("sine", "harmonics", "missing_fundamental")
TONE_SKIP = 4                # frames skipped at each end


# ------------------------------------------------------------------------------------------------ the definition
def frame_matrix(y, frame, hop, tau_max, dtype=np.float64):
    """[n_frames, L] frames of L = frame + tau_max samples starting at t * hop - L // 2, zeros outside the signal."""
    y = np.asarray(y)
    n = y.shape[0]
    span = frame + tau_max
    n_frames = 1 + n // hop
    idx = np.arange(n_frames, dtype=np.int64)[:, None] * hop - span // 2 + np.arange(span, dtype=np.int64)[None, :]
    inside = (idx >= 0) & (idx < n)
    return np.where(inside, y[np.clip(idx, 0, n - 1)], 0).astype(dtype)


def difference(x, frame, tau_max):
    """d [n_frames, tau_max + 1] in the dtype of ``x``: d(0) = 0, d(tau) = sum_j (x[j] - x[j + tau])^2 summed over j in ascending order
    (in float32 every product and every partial sum is rounded to float32)."""
    d = np.zeros((x.shape[0], tau_max + 1), x.dtype)
    acc = d[:, 1:]
    for j in range(frame):
        diff = x[:, j:j + 1] - x[:, j + 1:j + 1 + tau_max]
        acc += diff * diff
    return d


def cmndf(d):
    """d' : d'(0) = 1, d'(tau) = d(tau) tau / sum_{k <= tau} d(k) where the sum is > 0, else 1 (sequential running sum in d's dtype)."""
    run = np.cumsum(d[:, 1:], axis=1, dtype=d.dtype)
    tau = np.arange(1, d.shape[1], dtype=d.dtype)[None, :]
    out = np.ones_like(d)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = (d[:, 1:] * tau) / run
    out[:, 1:] = np.where(run > 0, q, np.ones_like(q))
    return out


def pick(dp, tau_min, tau_max, threshold, descend=True, exact=False):
    """(tau_int, margin): the picked lag of one frame's d' and the smallest margin of any comparison the pick made (against the threshold,
    the descent steps, the arg-min gap).  A tie between two values that are both exactly 0 or both exactly 1 is no ambiguity: d' is
    exactly 0 where d is (a sum of squares vanishes only with every term, in any precision) and exactly 1 where the running sum is 0, so
    every implementation of the definition ties there too — the zero padding of the edge frames produces whole runs of both.  ``exact``
    (signals whose d is the same number in fp32 and fp64): no exact tie is an ambiguity."""
    thr = dp.dtype.type(threshold)
    margins = []

    def note(m, value=None):
        if m == 0 and (exact or value in (0, 1)):
            return
        margins.append(abs(float(m)))

    window = dp[tau_min:tau_max + 1]
    below = np.nonzero(window < thr)[0]
    if below.size:
        tau = tau_min + int(below[0])
        for m in window[:below[0] + 1] - thr:
            note(m)
        while descend and tau + 1 <= tau_max:
            note(dp[tau + 1] - dp[tau], dp[tau])
            if not dp[tau + 1] < dp[tau]:
                break
            tau += 1
    else:
        for m in window - thr:
            note(m)
        best = int(np.argmin(window))
        rest = np.delete(window, best)
        if rest.size:
            note(rest.min() - window[best], window[best])
        tau = tau_min + best
    return tau, (min(margins) if margins else math.inf)


def refine(dp, tau, tau_max, clamp=True):
    """(lag, aperiodicity) of one frame in dp's dtype."""
    f = dp.dtype.type
    b = dp[tau]
    if tau - 1 >= 1 and tau + 1 <= tau_max:
        a, c = dp[tau - 1], dp[tau + 1]
        curv = (a - f(2) * b) + c
        if curv > 0:
            shift = f(0.5) * (a - c) / curv
            shift = min(max(shift, f(-0.5)), f(0.5))
            ap = b - f(0.25) * (a - c) * shift
            return f(tau) + shift, (max(f(0), ap) if clamp else ap)
    return f(tau), b


def yin(y, frame, hop, tau_min, tau_max, threshold, dtype=np.float64, exact=False, normalise=True, lag_offset=0, descend=True, clamp=True):
    """The whole definition -> dict(cmndf [T, tau_max + 1], tau_int [T], lag [T], aperiodicity [T], margin [T]) in ``dtype``.  The four
    switches build the deliberately wrong variants of tests/test_pitch_host.py."""
    x = frame_matrix(y, frame, hop, tau_max, dtype)
    d = difference(x, frame, tau_max)
    dp = cmndf(d) if normalise else np.concatenate([np.ones_like(d[:, :1]), d[:, 1:]], axis=1)
    n_frames = x.shape[0]
    tau_int = np.zeros(n_frames, np.int32)
    lag = np.zeros(n_frames, dtype)
    ap = np.zeros(n_frames, dtype)
    margin = np.zeros(n_frames, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        for t in range(n_frames):
            tau, margin[t] = pick(dp[t], tau_min, tau_max, threshold, descend=descend, exact=exact)
            tau = min(max(tau + lag_offset, tau_min), tau_max)
            tau_int[t] = tau
            lag[t], ap[t] = refine(dp[t], tau, tau_max, clamp=clamp)
    return {"cmndf": dp, "tau_int": tau_int, "lag": lag, "aperiodicity": ap, "margin": margin}


# ------------------------------------------------------------------------------------------------ comparison
def unambiguous(ref, cmndf_tol=CMNDF_TOL):
    """Frames whose pick is decided in float64 by more than twice the d' tolerance at every comparison it makes."""
    return ref["margin"] > 2 * cmndf_tol


def _errors(got, ref, key, scaled):
    e = np.abs(np.asarray(got[key], np.float64) - ref[key])
    return e / np.maximum(1.0, np.abs(ref[key])) if scaled else e


def compare(got, ref, cmndf_tol=CMNDF_TOL, lag_tol=LAG_TOL, ap_tol=APERIODICITY_TOL, scaled=False):
    """List of complaints (empty = ``got`` agrees with the float64 ``ref``): every d' element at its tolerance, none exempt; tau_int
    exactly, lag and aperiodicity at theirs on every frame whose pick is unambiguous in ``ref``.  ``scaled`` (the SHORT_WINDOW cases):
    the errors of d' and of the aperiodicity are divided by max(1, |reference|)."""
    bad = []
    err = _errors(got, ref, "cmndf", scaled)
    if not np.all(err <= cmndf_tol):  # (a NaN fails too)
        bad.append(f"cmndf: worst {np.nanmax(err):.3g} > {cmndf_tol:.3g} ({int((~(err <= cmndf_tol)).sum())} elements)")
    ok = unambiguous(ref, cmndf_tol)
    tau = np.asarray(got["tau_int"])
    if not np.array_equal(tau[ok], ref["tau_int"][ok]):
        where = np.nonzero(ok & (tau != ref["tau_int"]))[0]
        bad.append(f"tau_int differs on unambiguous frames {where[:8].tolist()}: {tau[where[:8]].tolist()} != {ref['tau_int'][where[:8]].tolist()}")
    for key, tol in (("lag", lag_tol), ("aperiodicity", ap_tol)):
        e = _errors(got, ref, key, scaled and key == "aperiodicity")[ok]
        if e.size and not np.all(e <= tol):
            bad.append(f"{key}: worst {np.nanmax(e):.3g} > {tol:.3g}")
    return bad


def worst(got, ref, cmndf_tol=CMNDF_TOL, scaled=False):
    """(cmndf, lag, aperiodicity) worst errors as compare() measures them; lag / aperiodicity over the unambiguous frames."""
    ok = unambiguous(ref, cmndf_tol)
    e = [float(np.max(_errors(got, ref, "cmndf", scaled)))]
    for key in ("lag", "aperiodicity"):
        v = _errors(got, ref, key, scaled and key == "aperiodicity")[ok]
        e.append(float(v.max()) if v.size else 0.0)
    return tuple(e)


# ------------------------------------------------------------------------------------------------ the GPU case list
FRAMES = (16, 63, 64, 65, 1000, 2048, 4096)
# the issue's pairs + the pairs around this kernel's own steps: 4 lags per lane (4 | 5), 64 / 128 / 256 lanes per workgroup
# (tau_max 256 | 257 and 512 | 513), a second lag group per lane (1024 | 1025), the last lag (2047, 2048)
TAU_PAIRS = ((1, 2), (2, 17), (10, 340), (63, 64), (64, 65), (255, 256), (256, 257), (1, 2048),
             (1, 4), (2, 5), (3, 512), (3, 513), (500, 1024), (500, 1025), (2047, 2048))
HOPS = (1, 7, 512, "n+3")
N_SAMPLES = ("1", "2", "hop-1", "hop", "hop+1", "L-1", "L", "L+1", "3L+5")
EXACT_SIGNALS = ("zeros", "constant", "impulse", "square")
NOISY_SIGNALS = ("tone40", "tone20", "tone6", "glide")
MAX_FRAMES = 64
MAX_COST = 6e7  # n_frames * frame * tau_max of one case: keeps the float64 reference of the whole list at a few seconds


def _resolve(hop, ns, span):
    """(hop, n_samples) for the symbolic choices, or None where the combination does not exist / is too long."""
    base = {"1": 1, "2": 2, "L-1": span - 1, "L": span, "L+1": span + 1, "3L+5": 3 * span + 5}
    if hop == "n+3":
        if ns not in base:
            return None
        n = base[ns]
        return n + 3, n
    n = base.get(ns)
    if n is None:
        n = {"hop-1": hop - 1, "hop": hop, "hop+1": hop + 1}[ns]
    if n < 1 or 1 + n // hop > MAX_FRAMES:
        return None
    return hop, n


# Which frame lengths a lag pair meets.  In the main list the analysis window is longer than the lag range (frame > tau_max), as in any
# sensible use: then d' stays of order 1 and ONE absolute tolerance means something.  With frame <= tau_max the first frames see nothing
# but padding in x[0 .. frame) and d'(tau) = tau at the first lag that reaches the signal — d' in the hundreds, whose fp32 rounding
# (relative, 6e-8) would swamp an absolute tolerance sized for the rest.  Those combinations are real kernel shapes (a j loop of a few
# steps under two lag groups per lane): SHORT_WINDOW keeps them as additional cases, on exact signals, with the d' tolerance scaled by
# max(1, d') — see compare().
PAIRING = (((1, 2), (16, 64)), ((2, 17), (63, 2048)), ((10, 340), (1000, 2048)), ((63, 64), (65, 1000)), ((64, 65), (1000, 4096)),
           ((255, 256), (1000, 2048)), ((256, 257), (1000, 4096)), ((1, 2048), (4096,)), ((1, 4), (16, 65)), ((2, 5), (63, 64)),
           ((3, 512), (1000, 4096)), ((3, 513), (1000, 2048)), ((500, 1024), (2048, 4096)), ((500, 1025), (2048, 4096)),
           ((2047, 2048), (4096,)))
SHORT_WINDOW = (((1, 2048), 16), ((2047, 2048), 64), ((10, 340), 63), ((64, 65), 65), ((500, 1025), 1000), ((3, 513), 16))


def gpu_cases():
    """The pruned cross of FRAMES x TAU_PAIRS x HOPS x N_SAMPLES x signals: every lag pair with the frame lengths of PAIRING, hop and
    n_samples rotating through their sets (the next admissible combination where one does not exist, exceeds MAX_FRAMES frames or
    MAX_COST), one exact and one noisy signal per combination (two exact ones below 64 samples, where a tone is a click, and in the
    SHORT_WINDOW cases).  Deterministic: host test, GPU test and the tolerance run iterate the same list."""
    cases = []
    c = 0
    combos = [(pair, frame, False) for pair, frames in PAIRING for frame in frames] + [(pair, frame, True) for pair, frame in SHORT_WINDOW]
    assert {p for p, _, _ in combos} == set(TAU_PAIRS) and {f for _, f, _ in combos} == set(FRAMES)
    for (tau_min, tau_max), frame, short in combos:
        assert short == (frame <= tau_max)
        span = frame + tau_max
        for step in range(len(HOPS) * len(N_SAMPLES)):
            k = c + step
            got = _resolve(HOPS[k % len(HOPS)], N_SAMPLES[k % len(N_SAMPLES)], span)
            if got and (1 + got[1] // got[0]) * frame * tau_max <= MAX_COST:
                break
        else:
            raise AssertionError((frame, tau_min, tau_max))
        hop, n = got
        noisy = n >= 64 and not short
        second = NOISY_SIGNALS[(c // 2) % len(NOISY_SIGNALS)] if noisy else EXACT_SIGNALS[(c + 1) % len(EXACT_SIGNALS)]
        for signal in (EXACT_SIGNALS[c % len(EXACT_SIGNALS)], second):
            cases.append({"frame": frame, "tau_min": tau_min, "tau_max": tau_max, "hop": hop, "n_samples": n, "signal": signal,
                          "threshold": 0.1, "seed": 1000 + len(cases), "short": short})
        c += 1
    return cases


def case_id(case):
    return "f{frame}-t{tau_min}_{tau_max}-h{hop}-n{n_samples}-{signal}".format(**case)


def is_exact(case):
    """d of these signals is a sum of exactly representable squares (0, 0.25, 1, 4): the same number in fp32 and fp64, so d' differs
    from float64 by the rounding of one product and one quotient only."""
    return case["signal"] in EXACT_SIGNALS


def make_signal(case):
    """float32 samples of a case (built in float64, rounded once)."""
    n, tau_min, tau_max = case["n_samples"], case["tau_min"], case["tau_max"]
    i = np.arange(n, dtype=np.float64)
    kind = case["signal"]
    if kind == "zeros":
        y = np.zeros(n)
    elif kind == "constant":
        y = np.full(n, 0.5)
    elif kind == "impulse":
        y = np.zeros(n)
        y[n // 2] = 1.0
    elif kind == "square":  # integer period: d is exactly 0 at every multiple of it
        period = 2 * max(1, (tau_min + 2) // 2)
        y = np.where((np.arange(n) % period) < period // 2, 1.0, -1.0)
    else:
        # a band-limited sawtooth (harmonics h <= period / 4, at most 40, amplitudes 1 / h): its d' has a SHARP minimum at the period, so
        # that neighbouring lags differ by more than the ambiguity margin even at periods of many hundred samples (a sine's minimum is
        # as flat as (2 pi / period)^2); the period sits 0.07 samples above an integer lag
        rng = np.random.default_rng(case["seed"])
        period = float(round(tau_min + (tau_max - tau_min) / 2.7)) + 0.07
        harmonics = np.arange(1, max(1, min(40, int(period / 4))) + 1, dtype=np.float64)
        if kind == "glide":  # the same tone gliding up a tenth of an octave over the clip, next to a weaker one a fifth above it
            phase = 2 * np.pi * np.cumsum(2.0 ** (i / max(n, 1) / 10.0)) / period
            saw = (np.sin(harmonics[None, :] * phase[:, None]) / harmonics[None, :]).sum(1)
            y = 0.3 * saw + 0.05 * np.sin(1.5 * phase + 0.3) + 0.002 * rng.standard_normal(n)
        else:
            saw = (np.sin(harmonics[None, :] * (2 * np.pi * i[:, None] / period + 0.2)) / harmonics[None, :]).sum(1)
            y = 0.3 * saw
            y = y + np.sqrt(np.mean(y * y)) * 10 ** (-float(kind[4:]) / 20) * rng.standard_normal(n)
    return y.astype(np.float32)


def reference(case, dtype=np.float64):
    r = yin(make_signal(case), case["frame"], case["hop"], case["tau_min"], case["tau_max"], case["threshold"], dtype=dtype,
            exact=is_exact(case))
    if is_exact(case):  # nothing is exempt: tests/test_pitch_host.py shows that fp32 rounding of these d' moves no pick
        r["margin"][:] = np.inf
    return r


def tolerances(case):
    """(cmndf, lag, aperiodicity) tolerances of a case, in compare()'s argument order."""
    if case["short"]:
        return SHORT_CMNDF_TOL, SHORT_LAG_TOL, SHORT_APERIODICITY_TOL
    return CMNDF_TOL, LAG_TOL, APERIODICITY_TOL


def max_exempt(n_frames):
    """At most 2 % of the frames of a case may be exempt as ambiguous, at most one in a case of fewer than 50."""
    return 1 if n_frames < 50 else int(0.02 * n_frames)


# ------------------------------------------------------------------------------------------------ known answers
def tone(kind, freq, seconds=1.0, sr=TONE_SR):
    """float32 test tone: a sine, harmonics 1-3 with 1/h amplitudes, or harmonics 2, 3, 4 without the fundamental."""
    t = np.arange(int(seconds * sr), dtype=np.float64) / sr
    harmonics = {"sine": (1,), "harmonics": (1, 2, 3), "missing_fundamental": (2, 3, 4)}[kind]
    y = sum(np.sin(2 * np.pi * h * freq * t) / h for h in harmonics)
    return (0.5 * y / len(harmonics)).astype(np.float32)


def tone_cases():
    return [(kind, f) for kind in TONE_KINDS for f in TONE_FREQS]


def cents(f0, freq):
    return 1200.0 * np.abs(np.log2(np.asarray(f0, np.float64) / freq))


def tone_errors(dtype=np.float64, **variant):
    """(worst cents, worst aperiodicity) over tone_cases(), interior frames, of the definition in ``dtype``."""
    worst_c, worst_ap = 0.0, 0.0
    for kind, freq in tone_cases():
        r = yin(tone(kind, freq, seconds=0.5), TONE_FRAME, TONE_HOP, TONE_TAU_MIN, TONE_TAU_MAX, TONE_THRESHOLD, dtype=dtype, **variant)
        inner = slice(TONE_SKIP, -TONE_SKIP)
        worst_c = max(worst_c, float(cents(TONE_SR / r["lag"][inner].astype(np.float64), freq).max()))
        worst_ap = max(worst_ap, float(r["aperiodicity"][inner].max()))
    return worst_c, worst_ap


# ------------------------------------------------------------------------------------------------ ar.pitch, steps 4-8, on the host
def height(f0, fmin, fmax, dtype=np.float64):
    f0 = np.asarray(f0, dtype)
    return np.clip(np.log2(f0 / dtype(fmin)) / dtype(math.log2(fmax / fmin)), 0, 1).astype(dtype)


def hold_fill(values, voiced):
    """Unvoiced frames take the previous voiced value, leading ones the first voiced value; None when nothing is voiced."""
    voiced = np.asarray(voiced, bool)
    if not voiced.any():
        return None
    idx = np.where(voiced, np.arange(len(voiced)), -1)
    idx = np.maximum.accumulate(idx)
    idx[idx < 0] = int(np.argmax(voiced))
    return np.asarray(values)[idx]


def median5(x):
    """5-tap median along time with symmetric reflection (d c b a | a b c d | d c b a) — maua_median_filter_f32's boundary."""
    n = len(x)
    q = np.arange(-2, n + 2)
    q = np.mod(q, 2 * n)
    q = np.where(q >= n, 2 * n - 1 - q, q)
    padded = np.asarray(x)[q]
    return np.median(np.stack([padded[k:k + n] for k in range(5)]), axis=0).astype(np.asarray(x).dtype)


def lerp_resize(x, num, dtype=np.float64):
    """Linear interpolation of x[n] at the ``num`` positions i (n - 1) / (num - 1) (end points kept)."""
    x = np.asarray(x, dtype)
    n = len(x)
    if n == 1 or num == 1:
        return np.full(num, x[0], dtype)
    pos = np.arange(num, dtype=dtype) * dtype((n - 1) / (num - 1))
    lo = np.minimum(np.floor(pos).astype(np.int64), n - 2)
    frac = (pos - lo.astype(dtype)).astype(dtype)
    return (x[lo] * (dtype(1) - frac) + x[lo + 1] * frac).astype(dtype)


def gaussian_smooth(x, sigma, smf=1, dtype=np.float64):
    """The circular Gaussian FIR of ar.gaussian_filter (radius int(4 sigma smf), capped at 3 n; circular inside one wrap, zero beyond)."""
    x = np.asarray(x, dtype)
    n = len(x)
    radius = min(int(sigma * 4 * smf), 3 * n)
    k = np.arange(-radius, radius + 1, dtype=np.float32)
    taps = np.exp(np.float32(-0.5 / sigma ** 2) * k * k).astype(np.float32)
    taps = (taps / taps.sum(dtype=np.float32)).astype(dtype)
    out = np.zeros(n, dtype)
    for j, w in enumerate(taps):
        i = np.arange(n) + j - radius
        inside = (i >= -n) & (i < 2 * n)
        out = out + w * np.where(inside, x[np.mod(i, n)], dtype(0))
    return out


def pitch_pipeline(f0, confidence, n_frames, fmin, fmax, voicing=0.5, smooth=2, dtype=np.float64):
    """Steps 4-8 of ar.pitch on raw f0 / confidence -> (height [n_frames], voicing envelope [n_frames]) in ``dtype``."""
    conf = np.asarray(confidence, dtype)
    h = hold_fill(height(f0, fmin, fmax, dtype), conf >= dtype(voicing))
    h = np.zeros(len(conf), dtype) if h is None else median5(h)
    return (gaussian_smooth(lerp_resize(h, n_frames, dtype), smooth, dtype=dtype),
            gaussian_smooth(lerp_resize(conf, n_frames, dtype), smooth, dtype=dtype))


def arpeggio(sr=22050, notes=(110.0, 164.81, 220.0, 329.63), note_s=0.25, gap_s=0.2):
    """4 notes of 0.25 s (harmonics 1-3) with silences between them (0.2 s: longer than the 2388 samples a frame reads, so some frames see nothing else) -> (float32 samples, [(start, stop, freq)] in samples)."""
    parts, spans, pos = [], [], 0
    for f in notes:
        t = np.arange(int(note_s * sr), dtype=np.float64) / sr
        parts.append(0.4 * sum(np.sin(2 * np.pi * h * f * t) / h for h in (1, 2, 3)))
        spans.append((pos, pos + len(t), f))
        pos += len(t)
        gap = np.zeros(int(gap_s * sr))
        parts.append(gap)
        pos += len(gap)
    return np.concatenate(parts).astype(np.float32), spans


ARPEGGIO_FRAMES, ARPEGGIO_FMIN, ARPEGGIO_FMAX = 40, 65.0, 2100.0  # video frames of the arpeggio test; ar.pitch's default band


def arpeggio_reference(dtype=np.float64):
    """(height, voicing envelope, raw f0, raw confidence) of ar.pitch(margin=None) on the arpeggio, every stage in ``dtype``."""
    y, _ = arpeggio()
    r = yin(y, TONE_FRAME, TONE_HOP, TONE_TAU_MIN, TONE_TAU_MAX, TONE_THRESHOLD, dtype=dtype)
    f0 = dtype(TONE_SR) / r["lag"]
    conf = dtype(1) - np.minimum(r["aperiodicity"], dtype(1))
    return pitch_pipeline(f0, conf, ARPEGGIO_FRAMES, ARPEGGIO_FMIN, ARPEGGIO_FMAX, dtype=dtype) + (f0, conf)


def pipeline_emulation_error():
    """Worst |fp32 - float64| of the height and of the voicing envelope of the arpeggio, YIN included in both."""
    h64, v64, _, _ = arpeggio_reference(np.float64)
    h32, v32, _, _ = arpeggio_reference(np.float32)
    return float(np.abs(h32.astype(np.float64) - h64).max()), float(np.abs(v32.astype(np.float64) - v64).max())


def main():
    figures = {False: [0.0, 0.0, 0.0], True: [0.0, 0.0, 0.0]}
    exempt = 0
    cases = gpu_cases()
    for case in cases:
        ref = reference(case)
        emu = reference(case, np.float32)
        # (ambiguity is judged with the d' tolerance above, which this run is there to derive: run it again after changing the constant)
        e = worst(emu, ref, scaled=case["short"])
        exempt += int((~unambiguous(ref)).sum())
        figures[case["short"]] = [max(a, b) for a, b in zip(figures[case["short"]], e)]
    print(f"{len(cases)} cases, {exempt} ambiguous frames")
    for short, name in ((False, "frame > tau_max (absolute)"), (True, "SHORT_WINDOW (d', aperiodicity / max(1, |ref|))")):
        w = figures[short]
        print(f"fp32 emulation against float64, {name}: cmndf {w[0]:.3g}   lag {w[1]:.3g} samples   aperiodicity {w[2]:.3g}")
    c64, a64 = tone_errors(np.float64)
    c32, a32 = tone_errors(np.float32)
    print(f"known answers: float64 worst {c64:.3f} cents, aperiodicity <= {a64:.4f};  fp32 emulation worst {c32:.3f} cents, <= {a32:.4f}")
    e = pipeline_emulation_error()
    print(f"ar.pitch (YIN and steps 4-8) in fp32 against float64 on the arpeggio: height {e[0]:.3g}   voicing {e[1]:.3g}")


if __name__ == "__main__":
    main()
