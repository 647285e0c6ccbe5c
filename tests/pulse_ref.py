"""The predominant local pulse (Grosche & Mueller 2011) in numpy: the definition behind csrc/pulse.hip and audioreactive/beat.py.

Two forms of each entry of include/maua_hip.h ("Predominant local pulse"): float64 on the same float32 table / window / (bin, phase)
the kernel reads, and an emulation with float32 accumulation in the kernel's summation order (ascending k, one chain per element, fused
multiply-add emulated through float64).  The emulation is not compared with the kernel: its distance from float64 is the measured size of
float32 rounding, and the tolerance of a test is four times that, asserted to lie under the derived ceiling:

  entry A  eps_F = (W + 3) 2^-24 sum_k |x[k]| |tab[b][k]| on each component of F; 2 |F| eps_F + eps_F^2 (times p[b]) on S; on the phase
           asin(min(1, eps_F / |F|)) plus the float32 atan2 term (the emulation's float32 arctan2 against float64 on the same operands).
           Tolerances are the ceiling scaled by 4 x the emulation's worst fraction of it (a fraction under 1/4 keeps them below).
  entry B  two ulps of the largest argument W omega_max + pi plus (W + 2) 2^-24: num / den is a weighted mean of cosines.

bin must be exact except on the frames where the reference's two best scores lie within twice the S ceiling of each other (decided here,
before a kernel runs, capped at 2 % of a case's frames); there phase and power are compared with the reference at the kernel's bin.

Also here: beat picking and the beat-phase mapping as plain numpy, the case lists of the GPU tests, and four deliberately wrong variants
(``variant=``) that tests/test_pulse_host.py feeds to the comparison functions."""
import functools
import math

import numpy as np

SR = 22050
HOP = 512
FR = SR / HOP
WIN = 384
TILE = 64    # frames per workgroup of maua_tempogram_peak_f32
BLOCK = 128  # output samples per workgroup of maua_pulse_synth_f32
U = 2.0 ** -24
EXEMPT_CAP = 0.02


# ------------------------------------------------------------------------------------------------ tables
def tempo_grid(tempo_min=30.0, tempo_max=300.0, tempo_step=1.0):
    return tempo_min + tempo_step * np.arange(int(math.floor((tempo_max - tempo_min) / tempo_step + 1e-9)) + 1, dtype=np.float64)


def omega_of(grid_bpm, fr=FR):
    return 2.0 * np.pi * np.asarray(grid_bpm, np.float64) / (60.0 * fr)


def hann(win):
    return 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(win) / win)  # periodic


def make_table(window, omega):
    """tab[b][k] = w[k] (cos(omega_b k), -sin(omega_b k)) in float64, rounded to float32 once."""
    k = np.arange(len(window), dtype=np.float64)
    arg = np.asarray(omega, np.float64)[:, None] * k[None, :]
    w = np.asarray(window, np.float64)[None, :]
    return np.stack([w * np.cos(arg), -w * np.sin(arg)], axis=-1).astype(np.float32)


def lognormal_prior(grid_bpm, start_bpm=120.0):
    return np.exp(-0.5 * np.log2(np.asarray(grid_bpm, np.float64) / start_bpm) ** 2).astype(np.float32)


def frame_matrix(env, win, centre_shift=0):
    """x[t][k] = env[t - win // 2 + k], zero outside."""
    n = len(env)
    idx = np.arange(n)[:, None] - win // 2 + np.arange(win)[None, :] + centre_shift
    ok = (idx >= 0) & (idx < n)
    return np.where(ok, np.asarray(env)[np.clip(idx, 0, n - 1)], 0).astype(env.dtype)


# ------------------------------------------------------------------------------------------------ entry A
def walk_peak(S, ties_high=False):
    """best = 0, bin = -1; walking b upwards, take b when S > best (a NaN never compares greater)."""
    clean = np.where(np.isnan(S), -np.inf, S)
    if ties_high:
        bins = S.shape[1] - 1 - np.argmax(clean[:, ::-1], axis=1)
    else:
        bins = np.argmax(clean, axis=1)
    best = clean[np.arange(len(S)), bins]
    ok = best > 0
    return np.where(ok, bins, -1).astype(np.int32), np.where(ok, best, 0.0)


def tempogram_peak(env, table, prior=None, variant=None, exact=False):
    """Entry A in float64 on the float32 operands, with the per-element ceilings and the frames exempt from an exact bin.  ``exact``: the
    caller has shown float32 to be exact on these operands (small integers), so no frame is exempt: ties are the definition's to settle."""
    env = np.asarray(env, np.float32)
    tab = np.asarray(table, np.float64)
    if variant == "phase_sign":
        tab = tab * np.array([1.0, -1.0])
    B, W, _ = tab.shape
    X = frame_matrix(env.astype(np.float64), W, centre_shift=1 if variant == "centre" else 0)
    cos_t, sin_t = np.ascontiguousarray(tab[:, :, 0].T), np.ascontiguousarray(tab[:, :, 1].T)
    re, im = X @ cos_t, X @ sin_t
    p = np.ones(B) if prior is None else np.asarray(prior, np.float64)
    S = (re * re + im * im) * p[None, :]
    bins, power = walk_peak(S, ties_high=variant == "ties_high")
    mag = np.hypot(re, im)
    with np.errstate(invalid="ignore"):
        eps_f = (W + 3) * U * (np.abs(X) @ np.hypot(cos_t, sin_t))
        ceil_s = (2.0 * mag * eps_f + eps_f ** 2) * p[None, :]
        ceil_ph = np.arcsin(np.minimum(1.0, np.where(mag > 0, eps_f / np.where(mag > 0, mag, 1.0), 1.0)))
    rows = np.arange(len(env))
    at = np.maximum(bins, 0)
    phase = np.where(bins >= 0, np.arctan2(im[rows, at], re[rows, at]), 0.0)
    # the second best score, and whether it lies within twice the ceiling of the best
    clean = np.where(np.isnan(S), -np.inf, S)
    exempt = np.zeros(len(env), bool)
    if B > 1 and not exact:
        rest = clean.copy()
        rest[rows, at] = -np.inf
        second_at = np.argmax(rest, axis=1)
        second = rest[rows, second_at]
        c = np.maximum(ceil_s[rows, at], ceil_s[rows, second_at])
        with np.errstate(invalid="ignore"):
            exempt = (bins >= 0) & (c > 0) & (power - second <= 2.0 * c)
    return dict(bin=bins, phase=phase, power=power, S=S, re=re, im=im, ceil_s=ceil_s, ceil_ph=ceil_ph, exempt=exempt)


def emulate_peak(env, table, prior=None, frames=None):
    """Entry A with float32 accumulation in the kernel's order on the frames ``frames`` (all by default): (re, im, S, phase32 - phase64
    of the float32 operands)."""
    env = np.asarray(env, np.float32)
    tab = np.asarray(table, np.float32)
    B, W, _ = tab.shape
    X = frame_matrix(env, W)
    if frames is not None:
        X = X[frames]
    re = np.zeros((len(X), B), np.float32)
    im = np.zeros((len(X), B), np.float32)
    for k in range(W):
        xk = X[:, k, None].astype(np.float64)
        re = (xk * tab[None, :, k, 0].astype(np.float64) + re).astype(np.float32)  # a float32 product is exact in float64: one rounding
        im = (xk * tab[None, :, k, 1].astype(np.float64) + im).astype(np.float32)
    S = re * re + im * im
    if prior is not None:
        S = S * np.asarray(prior, np.float32)[None, :]
    with np.errstate(invalid="ignore"):
        atan_term = np.abs(np.arctan2(im, re).astype(np.float64) - np.arctan2(im.astype(np.float64), re.astype(np.float64)))
    return re, im, S, atan_term


def peak_tolerances(env, table, prior, ref, max_frames=192):
    """(rho_S, rho_phase, atan_term): the emulation's worst error as a fraction of the ceilings (S; the phase's asin part) and its worst
    float32 atan2 error, on at most ``max_frames`` evenly spread frames.  The tests use 4 x these."""
    n = len(ref["bin"])
    frames = np.unique(np.linspace(0, n - 1, min(n, max_frames)).round().astype(int))
    re, im, S, atan_term = emulate_peak(env, table, prior, frames)
    ok = np.isfinite(ref["S"][frames])
    with np.errstate(invalid="ignore", divide="ignore"):
        frac = np.abs(S.astype(np.float64) - ref["S"][frames]) / ref["ceil_s"][frames]
    frac = np.where(ok & (ref["ceil_s"][frames] > 0), frac, 0.0)
    assert np.all(S[ok & (ref["ceil_s"][frames] == 0)] == 0)
    rho_s = float(frac.max()) if frac.size else 0.0
    d = angle_diff(np.arctan2(im.astype(np.float64), re.astype(np.float64)), np.arctan2(ref["im"][frames], ref["re"][frames]))
    with np.errstate(invalid="ignore", divide="ignore"):
        fr_ph = np.where(ok & (ref["ceil_ph"][frames] > 0) & (np.hypot(ref["re"][frames], ref["im"][frames]) > 0), d / ref["ceil_ph"][frames], 0.0)
    rho_ph = float(np.nan_to_num(fr_ph).max()) if fr_ph.size else 0.0
    a = float(np.nan_to_num(atan_term).max()) if atan_term.size else 0.0
    return rho_s, rho_ph, max(a, U)


def angle_diff(a, b):
    return np.abs((np.asarray(a, np.float64) - np.asarray(b, np.float64) + np.pi) % (2.0 * np.pi) - np.pi)


def compare_peak(got, ref, tol):
    """Problems (strings) of entry A outputs ``got`` (bin, phase, power and optionally tgram) against ``ref`` = tempogram_peak(...) under
    ``tol`` = peak_tolerances(...): [] when all is well."""
    rho_s, rho_ph, atan_term = tol
    assert 4 * rho_s < 1 and 4 * rho_ph < 1, f"4 x the emulation's error ({rho_s:.3g}, {rho_ph:.3g} of the ceilings) is not under the ceiling"
    problems = []
    n, B = ref["S"].shape
    rows = np.arange(n)
    gb = np.asarray(got["bin"]).astype(np.int64)
    if np.any((gb < -1) | (gb >= B)):
        return [f"bin outside [-1, {B})"]
    wrong = (gb != ref["bin"]) & ~ref["exempt"]
    if wrong.any():
        t = int(np.flatnonzero(wrong)[0])
        problems.append(f"bin: {int(wrong.sum())} frames differ outside the exempt set, first t={t}: got {gb[t]}, want {ref['bin'][t]}")
    lost = (gb < 0) & (ref["bin"] >= 0) & ref["exempt"]
    if lost.any():
        problems.append(f"bin: {int(lost.sum())} exempt frames came back without a tempo")
    at = np.maximum(gb, 0)
    has = gb >= 0
    tol_s = 4 * rho_s * ref["ceil_s"]
    want_power = np.where(has, ref["S"][rows, at], 0.0)
    gp = np.asarray(got["power"], np.float64)
    with np.errstate(invalid="ignore"):
        bad = ~(np.abs(gp - want_power) <= np.where(has, tol_s[rows, at], 0.0))
    if bad.any():
        t = int(np.flatnonzero(bad)[0])
        problems.append(f"power: {int(bad.sum())} frames out of tolerance, first t={t}: got {gp[t]!r}, want {want_power[t]!r}")
    want_phase = np.where(has, np.arctan2(ref["im"][rows, at], ref["re"][rows, at]), 0.0)
    tol_ph = np.where(has, 4 * rho_ph * ref["ceil_ph"][rows, at] + 4 * atan_term, 0.0)
    with np.errstate(invalid="ignore"):
        bad = ~(angle_diff(got["phase"], want_phase) <= tol_ph)
    if bad.any():
        t = int(np.flatnonzero(bad)[0])
        problems.append(f"phase: {int(bad.sum())} frames out of tolerance, first t={t}: got {float(got['phase'][t])!r}, want {want_phase[t]!r} +- {tol_ph[t]:.3g}")
    if got.get("tgram") is not None:
        g = np.asarray(got["tgram"], np.float64)
        nan_ref = np.isnan(ref["S"])
        if not np.array_equal(np.isnan(g), nan_ref):
            problems.append("tgram: NaN where the reference has none, or the reverse")
        with np.errstate(invalid="ignore"):
            bad = ~nan_ref & ~(np.abs(g - ref["S"]) <= tol_s)
        if bad.any():
            t, b = (int(v[0]) for v in np.nonzero(bad))
            problems.append(f"tgram: {int(bad.sum())} elements out of tolerance, first [{t}, {b}]: got {g[t, b]!r}, want {ref['S'][t, b]!r} +- {tol_s[t, b]:.3g}")
    return problems


# ------------------------------------------------------------------------------------------------ entry B
def pulse_synth(bins, phase, window, omega, dtype=np.float64, variant=None):
    """Entry B: float64 on the float32 operands, or (dtype=np.float32) every operation in float32 in the kernel's order."""
    bins = np.asarray(bins).astype(np.int64)
    n, W, B = len(bins), len(window), len(omega)
    f = dtype
    valid = (bins >= 0) & (bins < B)
    om = np.where(valid, np.asarray(omega, np.float32)[np.clip(bins, 0, B - 1)], 0).astype(f)
    ph = np.asarray(phase, np.float32).astype(f)
    w = np.asarray(window, np.float32).astype(f)
    num, den = np.zeros(n, f), np.zeros(n, f)
    m = np.arange(n)
    for k in range(W):
        t = m + W // 2 - k
        inside = (t >= 0) & (t < n)
        tc = np.clip(t, 0, n - 1)
        den = np.where(inside, den + w[k], den).astype(f)
        arg = (om[tc] * f(k)).astype(f) + ph[tc]
        c = np.cos(arg.astype(np.float64)).astype(f)
        num = np.where(inside & valid[tc], num + (w[k] * c).astype(f), num).astype(f)
    if variant == "den_const":
        den = np.full(n, w.sum(dtype=f), f)
    with np.errstate(invalid="ignore", divide="ignore"):
        r = num / den
    return np.where((den > 0) & (r > 0), r, 0).astype(f)


def synth_ceiling(win, omega):
    largest = win * float(np.max(np.abs(omega))) + math.pi
    return 2.0 * 2.0 ** (math.floor(math.log2(largest)) - 23) + (win + 2) * U


def synth_tolerance(bins, phase, window, omega, ref=None):
    """4 x the float32 emulation's worst distance from float64, asserted under the ceiling."""
    ref = pulse_synth(bins, phase, window, omega) if ref is None else ref
    worst = float(np.abs(pulse_synth(bins, phase, window, omega, np.float32).astype(np.float64) - ref).max())
    tol = 4.0 * max(worst, U)
    assert tol < synth_ceiling(len(window), omega), (tol, synth_ceiling(len(window), omega))
    return tol


def compare_pulse(got, ref, tol):
    got = np.asarray(got, np.float64)
    with np.errstate(invalid="ignore"):
        bad = ~(np.abs(got - ref) <= tol)
    bad |= (ref == 0) & (got != 0) & (np.abs(got) > tol)
    if bad.any():
        m = int(np.flatnonzero(bad)[0])
        return [f"pulse: {int(bad.sum())} samples out of tolerance {tol:.3g}, first m={m}: got {got[m]!r}, want {ref[m]!r}"]
    return []


# ------------------------------------------------------------------------------------------------ beats and beat phase
def pick_beats(pulse, fr=FR, threshold=0.1):
    """Maxima P[m] > P[m-1], P[m] >= P[m+1], P[m] > threshold of the interior samples, refined by the three-point parabola: seconds."""
    p = np.asarray(pulse, np.float64)
    if len(p) < 3:
        return np.zeros(0)
    a, b, c = p[:-2], p[1:-1], p[2:]
    at = np.flatnonzero((b > a) & (b >= c) & (b > threshold))
    curv = a[at] - 2 * b[at] + c[at]
    delta = np.where(curv < 0, 0.5 * (a[at] - c[at]) / np.where(curv < 0, curv, 1.0), 0.0)
    return (at + 1 + np.clip(delta, -0.5, 0.5)) / fr


def beat_phase_from_times(times, duration, n_frames, division=1.0):
    """float64 restatement of audioreactive.beat.beat_phase_from_times (zeros for fewer than two beats)."""
    times = np.asarray(times, np.float64)
    if len(times) < 2:
        return np.zeros(n_frames)
    tau = np.arange(n_frames) * (duration / n_frames)
    i = np.clip(np.searchsorted(times, tau, side="right") - 1, 0, len(times) - 2)
    count = i + (tau - times[i]) / (times[i + 1] - times[i])
    x = division * count
    return x - np.floor(x)


def plp(env, grid_bpm, fr=FR, win=WIN, prior=None):
    """The whole pipeline in float64 on a float32 envelope: (pulse, tempo in BPM with NaN where there is none, power)."""
    om = omega_of(grid_bpm, fr)
    w = hann(win)
    a = tempogram_peak(env, make_table(w, om), prior)
    pulse = pulse_synth(a["bin"], a["phase"].astype(np.float32), w.astype(np.float32), om.astype(np.float32))
    tempo = np.where(a["bin"] >= 0, np.asarray(grid_bpm)[np.maximum(a["bin"], 0)], np.nan)
    return pulse, tempo, a["power"]


def detrend(env, win):
    """env minus its moving average over ``win`` frames (centred, zero-padded sums over the true count), clamped at 0."""
    env = np.asarray(env, np.float64)
    n = len(env)
    c = np.concatenate([[0.0], np.cumsum(env)])
    lo = np.clip(np.arange(n) - win // 2, 0, n)
    hi = np.clip(np.arange(n) - win // 2 + win, 0, n)
    return np.maximum(env - (c[hi] - c[lo]) / win, 0.0)


# ------------------------------------------------------------------------------------------------ envelopes
def click_times(bpm, duration, start=0.5):
    return np.arange(start, duration - 1e-9, 60.0 / bpm)


def click_envelope(times, n, fr=FR):
    """A unit click at every time, split linearly between the two nearest frames."""
    env = np.zeros(n, np.float32)
    pos = np.asarray(times) * fr
    lo = np.floor(pos).astype(int)
    for i, f in zip(lo, pos - lo):
        if 0 <= i < n:
            env[i] += 1 - f
        if 0 <= i + 1 < n:
            env[i + 1] += f
    return env


def switch_times(duration=60.0, at=30.0, first=100.0, second=150.0):
    a = np.arange(0.6, at - 1e-9, 60.0 / first)
    b = np.arange(at, duration - 1e-9, 60.0 / second)
    return a, b


def make_env(case):
    """The envelope of a case.  "random": pulses at one of the case's own tempi with random heights over a floor of noise (a random
    envelope with a tempo: white noise has no predominant pulse, and at win 384 with 271 tempi its two best scores lie within twice
    the ceiling on 3.7 % of the frames, over the cap);
    "click": unit clicks at that tempo, split between frames; "integer": small non-negative integers; "zero"; "nan": random with one NaN."""
    n, kind = case["n"], case["kind"]
    rng = np.random.RandomState(case["seed"])
    om = case_omega(case)
    o = float(om[(len(om) * 2) // 5])
    t = np.arange(n)
    if kind == "zero":
        return np.zeros(n, np.float32)
    if kind == "integer":
        return rng.randint(0, 8, n).astype(np.float32)
    if kind == "click":
        return click_envelope(np.arange(0.3, n, 2 * np.pi / o), n, fr=1.0)
    env = (np.maximum(np.cos(o * t + 0.7), 0) ** 4 * (0.5 + 0.5 * rng.random_sample(n)) + 0.05 * rng.random_sample(n)).astype(np.float32)
    if kind == "nan":
        env[case.get("nan_at", n // 2)] = np.nan
    return env


def case_omega(case):
    """The grid of a case in radians per frame: the default 30 .. 300 BPM in 1 BPM steps for 271 tempi at win 384, otherwise ``n_tempi``
    equal steps from 0.15 to 3.0 (0.9 for a single tempo)."""
    B, W = case["n_tempi"], case["win"]
    if case.get("grid") == "integer":
        return np.array([0.0, np.pi / 2] * B)[:B]
    if B == 271 and W == WIN:
        return omega_of(tempo_grid())
    return np.linspace(0.15, 3.0, B) if B > 1 else np.array([0.9])


def case_window(case):
    if case.get("window") == "ones":
        return np.ones(case["win"])
    if case.get("window") == "zero_ends":
        w = hann(case["win"])
        w[: case["win"] // 4] = 0
        w[-(case["win"] // 4):] = 0
        return w
    if case.get("window") == "zero_middle":
        w = hann(case["win"])
        w[case["win"] // 4: case["win"] - case["win"] // 4] = 0
        return w
    return hann(case["win"])


def case_table(case):
    om = case_omega(case)
    if case.get("grid") == "integer":  # cos / sin of multiples of pi / 2, exactly
        k = np.arange(case["win"])
        quarter = np.array([[1, 0], [0, -1], [-1, 0], [0, 1]], np.float32)
        tab = np.stack([np.tile(np.array([[1.0, 0.0]], np.float32), (case["win"], 1)) if o == 0 else quarter[k % 4] for o in om])
        return tab.astype(np.float32) + 0.0  # (+ 0.0: no negative zeros)
    return make_table(case_window(case), om)


def case_prior(case):
    if not case.get("prior"):
        return None
    return (0.25 + 0.75 * np.random.RandomState(case["seed"] + 1000).random_sample(case["n_tempi"])).astype(np.float32)


def max_exempt(n):
    return int(math.floor(EXEMPT_CAP * n))


def _case(n, win, n_tempi, kind, seed, **kw):
    return dict(n=n, win=win, n_tempi=n_tempi, kind=kind, seed=seed, **kw)


def a_cases():
    """n: 1, W - 1, W, W + 1, one tile, two tiles + 5, 20 000; W: 2, 3, 33, 384, 2048; B: 1, 2, 63, 64, 65, 271, 1024 and, round the
    48 tempi of one round of the waves, 3, 4, 47, 48, 49, 97; random, click and
    zero envelopes, with and without prior and tgram.  (A frame whose window holds one non-zero sample scores the same on every tempo up
    to rounding: the cases with one-sample windows have one tempo, or few enough such frames for the cap.)"""
    return [
        _case(1, 384, 1, "random", 1, tgram=True),
        _case(1, 2, 1, "random", 2, window="ones"),
        _case(2, 2, 1, "random", 3, window="ones", tgram=True),
        _case(3, 2, 1, "random", 4, window="ones", prior=True),
        _case(TILE, 3, 2, "random", 5, window="ones", tgram=True),
        _case(2, 3, 1, "random", 6),
        _case(3, 3, 1, "random", 23, prior=True),
        _case(4, 3, 1, "random", 7, tgram=True),
        _case(32, 33, 2, "random", 8, tgram=True),
        _case(33, 33, 2, "random", 9, prior=True),
        _case(34, 33, 2, "random", 10, tgram=True, prior=True),
        _case(TILE, 33, 63, "random", 11, tgram=True),
        _case(2 * TILE + 5, 33, 64, "random", 12, prior=True, tgram=True),
        _case(2 * TILE + 5, 33, 65, "random", 13),
        _case(383, 384, 271, "random", 14),
        _case(384, 384, 271, "click", 15, tgram=True),
        _case(385, 384, 271, "random", 16, prior=True),
        _case(2 * TILE + 5, 384, 271, "zero", 17, tgram=True, prior=True),
        _case(2 * TILE + 5, 2048, 65, "random", 18, tgram=True),
        _case(2047, 2048, 1, "random", 24, tgram=True),
        _case(2048, 2048, 2, "random", 25, prior=True),
        _case(2049, 2048, 2, "random", 19),
        _case(2 * TILE + 5, 384, 1024, "random", 20, prior=True),
        _case(TILE, 384, 1024, "click", 21, tgram=True),
        # the kernel hands three tempi at a time to sixteen waves, 48 a round: a part round, one short of a round, a round, one over, two and one
        _case(65, 33, 3, "random", 26, prior=True),
        _case(65, 33, 4, "random", 27, tgram=True),
        _case(65, 33, 47, "random", 28, prior=True, tgram=True),
        _case(65, 33, 48, "random", 29, tgram=True),
        _case(65, 33, 49, "random", 30, prior=True),
        _case(65, 33, 97, "random", 31, prior=True, tgram=True),
    ]


LONG_CASE = _case(20000, 384, 271, "click", 22, tgram=True)


def case_id(case):
    extra = "".join(f"-{k}" for k in ("prior", "tgram") if case.get(k)) + "".join(f"-{case[k]}" for k in ("window", "grid") if case.get(k))
    return f"n{case['n']}-W{case['win']}-B{case['n_tempi']}-{case['kind']}{extra}"


@functools.lru_cache(maxsize=None)
def _a_reference(key):
    case = dict(key)
    env, table, prior = make_env(case), case_table(case), case_prior(case)
    ref = tempogram_peak(env, table, prior)
    assert int(ref["exempt"].sum()) <= max_exempt(case["n"]), (case_id(case), int(ref["exempt"].sum()))
    return env, table, prior, ref, peak_tolerances(env, table, prior, ref)


def a_reference(case):
    """(env, table, prior, reference, tolerances) of a case, computed once; asserts the exempt cap with the reference alone."""
    return _a_reference(tuple(sorted(case.items())))


def b_operands(case):
    """Host-built (bin, phase, window, omega) of an entry-B case.  kinds: "random" bins with runs of -1, "none" all -1, "wild" with bins
    outside [-1, n_tempi), "steady" one tempo with coherent phases."""
    n, W, B = case["n"], case["win"], case["n_tempi"]
    rng = np.random.RandomState(case["seed"])
    om = case_omega(case).astype(np.float32)
    w = case_window(case).astype(np.float32)
    bins = rng.randint(0, B, n).astype(np.int32)
    phase = rng.uniform(-np.pi, np.pi, n).astype(np.float32)
    kind = case["kind"]
    if kind == "steady":
        bins[:] = B // 2
        phase = ((((np.arange(n) - W // 2) * float(om[B // 2])) + np.pi) % (2 * np.pi) - np.pi).astype(np.float32)
    if kind in ("random", "wild", "steady") and n >= 8:
        lo = n // 3
        bins[lo: lo + max(1, n // 5)] = -1
        bins[rng.randint(0, n, max(1, n // 10))] = -1
    if kind == "none":
        bins[:] = -1
    if kind == "wild":
        bins[rng.randint(0, n, max(1, n // 4))] = rng.choice([-2, -1000, B, B + 7, 2 ** 30, -2 ** 31], max(1, n // 4))
    return bins, phase, w, om


def b_cases():
    return [
        _case(1, 384, 271, "random", 31),
        _case(1, 2, 1, "steady", 32, window="ones"),
        _case(3, 2, 2, "random", 33),
        _case(4, 3, 2, "wild", 34),
        _case(32, 33, 63, "random", 35),
        _case(33, 33, 64, "steady", 36),
        _case(34, 33, 65, "wild", 37),
        _case(BLOCK, 384, 271, "steady", 38),
        _case(2 * BLOCK + 5, 384, 271, "random", 39),
        _case(383, 384, 271, "wild", 40),
        _case(385, 384, 1024, "none", 41),
        _case(2 * BLOCK + 5, 2048, 65, "random", 42),
        _case(2049, 2048, 1024, "steady", 43),
        _case(96, 384, 271, "random", 44, window="zero_ends"),    # n < W: only the taps around W / 2 are reached, den > 0 everywhere
        _case(150, 384, 271, "random", 45, window="zero_middle"),  # den = 0 where every reachable tap lies in the zero middle, > 0 elsewhere
        _case(20, 384, 271, "random", 47, window="zero_middle"),   # den = 0 everywhere
        _case(20000, 384, 271, "random", 46),
    ]
