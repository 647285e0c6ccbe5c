"""Reference for probabilistic YIN (csrc/pyin.hip: maua_pyin_candidates_f32, maua_pyin_viterbi_f64; ar.raw_pyin, ar.pitch(method="pyin")):
the definitions in include/maua_hip.h restated in numpy — stage A (d' rows -> per-bin voiced mass) in float32, every operation as
defined, and in float64; stage B (the Viterbi decoder) in float64 with the exact operation order, once as a scalar loop that defines
every corner (NaN included) and once vectorised over the bins for long inputs (the host test shows that they agree bit for bit) — the
host construction of the tables, the shared case lists, the comparison helpers and the known-answer inputs.

    PYTHONPATH=tests python tests/pyin_ref.py

prints, without a GPU, the figures the tolerances below are derived from (never taken from the kernel)."""
import math

import numpy as np
import scipy.stats

import pitch_ref as pr

# limits of include/maua_hip.h
MAX_BINS, MAX_THRESHOLDS, MAX_WIDTH = 1024, 256, 128

# Measured by `python tests/pyin_ref.py` over a_cases(): the float32 restatement of stage A against the float64 one.
PERIOD_FIGURE = 5.81e-8          # worst |period fp32 - period fp64| / period fp64 (half an ulp: the rows are well conditioned, see make_rows)
PERIOD_TOL = 4 * PERIOD_FIGURE   # relative
# ar.pitch(method="pyin") on the arpeggio, steps 4-8 in fp32 against float64 on the same raw outputs:
PIPELINE_HEIGHT_FIGURE = 5.81e-8
PIPELINE_VOICING_FIGURE = 2.25e-7
PIPELINE_HEIGHT_TOL = 4 * PIPELINE_HEIGHT_FIGURE
PIPELINE_VOICING_TOL = 4 * PIPELINE_VOICING_FIGURE
# known answers: worst error of the reference (float64 YIN d' rounded to fp32, stage A in fp32, stage B) on the interior frames
NOISY_CASES = ((220.0, 6.0), (440.0, 6.0), (220.0, 3.0), (440.0, 3.0))   # (Hz, dB SNR), harmonics 1-3 + white noise, seed 5
NOISY_WORST_CENTS = (30.5, 14.6, 48.7, 24.8)  # measured, one per case; the bound of the tests is 100 cents (the right note)
NOISY_BOUND_CENTS = 100.0
NOISY_YIN_WRONG = 0.40           # plain YIN is off by more than 50 cents on at least this share of the same frames
ARPEGGIO_WORST_CENTS = 0.19      # measured on the frames that lie inside a note
ARPEGGIO_BOUND_CENTS = 0.29      # 1.5 x 0.19, rounded up
FLT_MIN = float(np.finfo(np.float32).tiny)


# ------------------------------------------------------------------------------------------------ host tables
def threshold_prior(n_thr=100, beta=(2, 18)):
    """cum_prior [n_thr + 1] fp32: the running sum (float64, rounded once) of the Beta prior over the thresholds k / n_thr."""
    prior = np.diff(scipy.stats.beta.cdf(np.arange(n_thr + 1, dtype=np.float64) / n_thr, *beta))
    return np.concatenate([[0.0], np.cumsum(prior)]).astype(np.float32)


def pitch_bins(fmin, fmax, bins_per_semitone):
    return int(math.floor(12 * bins_per_semitone * math.log2(fmax / fmin))) + 1


def transition_width(max_transition_rate, hop, sr, bins_per_semitone):
    return int(round(max_transition_rate * 12 * hop / sr)) * bins_per_semitone // 2


def bin_edges(sr, fmin, bins_per_semitone, n_bins):
    """bin_edge_period [n_bins + 1] fp32: sr / (fmin 2^((b - 0.5) / (12 B))), float64 rounded once."""
    b = np.arange(n_bins + 1, dtype=np.float64)
    return (sr / (fmin * 2.0 ** ((b - 0.5) / (12 * bins_per_semitone)))).astype(np.float32)


def bin_centres(fmin, bins_per_semitone, n_bins):
    return fmin * 2.0 ** (np.arange(n_bins, dtype=np.float64) / (12 * bins_per_semitone))


def transition_tables(n_bins, width):
    """(log_tri [2 W + 1], log_norm [P]) in float64: the triangular weights W + 1 - |d| and each source bin's sum of them over the
    targets inside [0, P - 1]."""
    d = np.arange(-width, width + 1)
    tri = (width + 1 - np.abs(d)).astype(np.float64)
    norm = np.array([tri[(d + i >= 0) & (d + i <= n_bins - 1)].sum() for i in range(n_bins)], np.float64)
    return np.log(tri), np.log(norm)


# ------------------------------------------------------------------------------------------------ stage A
def thr_index(x, n_thr):
    """idx(x) of the header on fp32 values: clamp((int)floorf(x * (float)n_thr), 0, n_thr), NaN and +inf -> n_thr."""
    with np.errstate(invalid="ignore", over="ignore"):
        v = np.floor(np.asarray(x, np.float32) * np.float32(n_thr))
    out = np.zeros(v.shape, np.int64)
    top = (v >= n_thr) | np.isnan(v)
    mid = ~top & (v > 0)
    out[top] = n_thr
    out[mid] = v[mid].astype(np.int64)
    return out


def trough_mask(cmndf, tau_min, tau_max):
    """[T, tau_max + 1] bool: fp32 compares of the given values, +inf left of tau_min, tau_max never."""
    r = np.asarray(cmndf, np.float32)
    mask = np.zeros(r.shape, bool)
    with np.errstate(invalid="ignore"):
        left = r[:, tau_min - 1:tau_max - 1].copy()
        left[:, 0] = np.inf
        mid, right = r[:, tau_min:tau_max], r[:, tau_min + 1:tau_max + 1]
        mask[:, tau_min:tau_max] = (mid < left) & (mid <= right)
    return mask


def refine_period(r, tau, dtype):
    """The parabola of maua_yin_f32 on one trough in ``dtype`` (fmaxf / fminf semantics for the clamp)."""
    f = dtype
    if tau - 1 >= 1:
        a, b, c = f(r[tau - 1]), f(r[tau]), f(r[tau + 1])
        with np.errstate(invalid="ignore", over="ignore", divide="ignore"):
            curv = (a - f(2) * b) + c
            if curv > 0:
                shift = (f(0.5) * (a - c)) / curv
                return f(tau) + np.fmin(np.fmax(shift, f(-0.5)), f(0.5))
    return f(tau)


def find_bin(edges, lag):
    """The first bin whose lower edge lies below the period, the last bin when none does (compares in the dtype of ``edges``)."""
    below = np.nonzero(edges[1:] < lag)[0]
    return int(below[0]) if below.size else len(edges) - 2


def candidates(cmndf, tau_min, tau_max, cum_prior, n_thr, no_trough_prob, edges, dtype=np.float32, first_only=True):
    """Stage A -> dict(obs [T, P], period [T, P], voiced_prob [T], count [T, P] summands per element, cands: per frame the list of
    (tau, p, lag, bin) with p > 0).  dtype float32: every operation as the header defines it.  float64: the same decisions (compares and
    idx are exact by definition on the given fp32 values) with the table differences, the parabola and the sums in float64.
    ``first_only=False`` is the deliberate defect of the host test: every trough takes every threshold it lies under."""
    f = dtype
    r = np.asarray(cmndf, np.float32)
    n_frames, n_bins = r.shape[0], len(edges) - 1
    cum, edg = np.asarray(cum_prior, np.float32).astype(f), np.asarray(edges, np.float32).astype(f)
    obs, period, best = np.zeros((n_frames, n_bins), f), np.zeros((n_frames, n_bins), f), np.zeros((n_frames, n_bins), f)
    count = np.zeros((n_frames, n_bins), np.int64)
    vp = np.zeros(n_frames, f)
    cands = []
    mask = trough_mask(r, tau_min, tau_max)
    for t in range(n_frames):
        taus = np.nonzero(mask[t])[0]
        h = r[t, taus]
        found = []
        if taus.size:
            before = np.concatenate([[np.float32(np.inf)], np.minimum.accumulate(h)[:-1]]).astype(np.float32)
            if first_only:
                rec = h < before
            else:
                rec, before = np.ones(len(h), bool), np.full(len(h), np.inf, np.float32)
            taus, h, before = taus[rec], h[rec], before[rec]
            p = cum[thr_index(before, n_thr)] - cum[thr_index(h, n_thr)]
            last = int(np.nonzero(h == h.min())[0][0])  # the first trough of smallest height
            p[last] = p[last] + f(f(no_trough_prob) * cum[thr_index(h[last], n_thr)])
            total = f(0)
            for tau, pk in zip(taus.tolist(), p):
                if not pk > 0:
                    continue
                lag = refine_period(r[t], tau, f)
                b = find_bin(edg, lag)
                obs[t, b] = obs[t, b] + pk
                count[t, b] += 1
                total = total + pk
                if pk > best[t, b]:
                    best[t, b], period[t, b] = pk, lag
                found.append((tau, float(pk), float(lag), b))
            vp[t] = min(f(1), total)
        cands.append(found)
    return {"obs": obs, "period": period, "voiced_prob": vp, "count": count, "cands": cands}


def near_edge_frames(ref, edges, tol=PERIOD_TOL):
    """Frames with a candidate whose refined period lies within twice the (relative) period tolerance of a bin edge: their bins are
    not compared."""
    e = np.asarray(edges, np.float64)[1:-1]  # (the outermost edges decide nothing: the bins beyond them are clamped to)
    out = np.zeros(len(ref["cands"]), bool)
    for t, found in enumerate(ref["cands"]):
        for _, _, lag, _ in found:
            if np.any(np.abs(e - lag) <= 2 * tol * abs(lag)):
                out[t] = True
    return out


def compare_candidates(got, ref, edges):
    """Complaints (empty = agreement) of stage-A outputs against the float32 restatement ``ref``: voiced_prob and obs within
    n 2^-24 1.01 (n = the summands of the element; non-negative fp32 terms with a total <= 1 + no_trough_prob, in any order), obs bit
    for bit where n <= 1, period within PERIOD_TOL (relative); obs / period are skipped on the frames of near_edge_frames()."""
    bad = []
    unit = 2.0 ** -24 * 1.01
    n_frame = np.array([len(c) for c in ref["cands"]])
    err = np.abs(np.asarray(got["voiced_prob"], np.float64) - ref["voiced_prob"].astype(np.float64))
    if not np.all(err <= n_frame * unit):
        bad.append(f"voiced_prob: worst {np.nanmax(err):.3g}")
    keep = ~near_edge_frames(ref, edges)
    g_obs, r_obs, n = np.asarray(got["obs"])[keep], ref["obs"][keep], ref["count"][keep]
    err = np.abs(g_obs.astype(np.float64) - r_obs.astype(np.float64))
    if not np.all(err <= n * unit):
        bad.append(f"obs: worst {np.nanmax(err):.3g} on {int((~(err <= n * unit)).sum())} elements")
    single = n <= 1
    if not np.array_equal(np.ascontiguousarray(g_obs[single]).view(np.int32), np.ascontiguousarray(r_obs[single]).view(np.int32)):
        bad.append("obs: an element of at most one summand differs in bits")
    g_per, r_per = np.asarray(got["period"], np.float64)[keep], ref["period"][keep].astype(np.float64)
    if not np.array_equal(g_per > 0, r_per > 0):
        bad.append("period: set in other bins")
    err = np.abs(g_per - r_per)
    if not np.all(err <= PERIOD_TOL * np.abs(r_per)):
        bad.append(f"period: worst {np.nanmax(err):.3g}")
    return bad


# ------------------------------------------------------------------------------------------------ stage A: the GPU case list
A_TAU_PAIRS = ((1, 2), (2, 5), (10, 340), (63, 64), (255, 256), (256, 257), (1, 2048))
A_BINS = (1, 2, 63, 64, 65, 602, 1024)
A_FRAMES = (1, 2, 65)
A_THRESHOLDS = (1, 100, 256)
A_KINDS = ("equal", "increasing", "decreasing", "alternating", "zeros", "multiples", "random", "nonfinite")


def a_cases():
    """The pruned cross: every lag pair meets every row kind; n_bins, n_frames and n_thr rotate through their sets with co-prime
    strides, so that every value of each meets every lag pair.  Deterministic: host test, GPU test and the tolerance run share it."""
    cases = []
    for i, (tau_min, tau_max) in enumerate(A_TAU_PAIRS):
        for k, kind in enumerate(A_KINDS):
            c = len(cases)
            cases.append({"tau_min": tau_min, "tau_max": tau_max, "kind": kind, "n_bins": A_BINS[(k + i) % len(A_BINS)],
                          "n_frames": A_FRAMES[(k + i) % len(A_FRAMES)], "n_thr": A_THRESHOLDS[(k // 3 + k + i) % len(A_THRESHOLDS)],
                          "no_trough_prob": (0.01, 0.0, 1.0)[c % 3], "seed": 7300 + c})
    for key, values in (("n_bins", A_BINS), ("n_frames", A_FRAMES), ("n_thr", A_THRESHOLDS)):
        for pair in A_TAU_PAIRS:
            assert {c[key] for c in cases if (c["tau_min"], c["tau_max"]) == pair} == set(values), (key, pair)
    return cases


def a_case_id(case):
    return "t{tau_min}_{tau_max}-{kind}-b{n_bins}-f{n_frames}-k{n_thr}".format(**case)


def make_rows(case):
    """fp32 d' rows [n_frames, tau_max + 1] of a case.  The random kinds draw multiples of 2^-10 in [0, 1.25]: a - 2 b + c and a - c of
    the parabola are then exact in fp32 as in float64, the refined period is decided by one division and one addition, and the
    float32-against-float64 figure (and with it the width of the exempt strip around every bin edge) stays at half an ulp instead of
    being set by one shallow trough whose curvature cancels."""
    rng = np.random.default_rng(case["seed"])
    shape = (case["n_frames"], case["tau_max"] + 1)
    n_thr = case["n_thr"]
    kind = case["kind"]
    lagi = np.arange(shape[1], dtype=np.float64)[None, :]
    if kind == "equal":
        r = np.full(shape, 0.25)
    elif kind == "increasing":
        r = 0.01 + lagi / shape[1] + np.zeros(shape)
    elif kind == "decreasing":  # (one trough at tau_max - 1 only when the last step rises: the last element is lifted)
        r = 1.0 - lagi / (shape[1] + 1) + np.zeros(shape)
        r[:, -1] = 2.0
    elif kind == "alternating":  # the maximum number of troughs, descending heights: every one a record
        low = np.linspace(0.9, 0.0, shape[1])[None, :] * rng.integers(1, 1024, (shape[0], 1)) / 1024
        r = np.where(lagi % 2 == (case["tau_min"] % 2), low, 1.0 + 0 * low)
    elif kind == "zeros":
        r = np.where(rng.random(shape) < 0.5, 0.0, rng.integers(0, 1280, shape) / 1024)
    elif kind == "multiples":
        r = (rng.integers(0, n_thr + 2, shape).astype(np.float32) / np.float32(n_thr)).astype(np.float64)
    else:
        r = rng.integers(0, 1281, shape) / 1024
        if kind == "nonfinite":
            r = np.where(rng.random(shape) < 0.1, rng.choice([np.nan, np.inf, -np.inf], shape), r)
    r = r.astype(np.float32)
    r[:, 0] = 1.0
    return r


def case_tables(case):
    """(cum_prior, bin_edge_period) of a stage-A case: the Beta(2, 18) prior, edges geometric from tau_max + 0.5 down to tau_min - 0.5."""
    hi, lo, n = case["tau_max"] + 0.5, case["tau_min"] - 0.5, case["n_bins"]
    edges = (hi * (lo / hi) ** (np.arange(n + 1, dtype=np.float64) / n)).astype(np.float32)
    assert np.all(np.diff(edges) < 0)
    return threshold_prior(case["n_thr"]), edges


def a_reference(case, dtype=np.float32):
    cum, edges = case_tables(case)
    return candidates(make_rows(case), case["tau_min"], case["tau_max"], cum, case["n_thr"], case["no_trough_prob"], edges, dtype=dtype)


def max_exempt(n_frames):
    return pr.max_exempt(n_frames)


# ------------------------------------------------------------------------------------------------ stage B
def viterbi_loop(lov, lou, width, log_tri, log_norm, log_init, log_stay, log_switch, tie_high=False, add_first=False, normalise=True):
    """The decoder, operation by operation as the header states it, one scalar at a time: the definition (NaN included).  Returns
    (delta_last [2 P], backptr [T, 2 P] uint16, states [T] int32).  The three switches build the deliberately wrong variants of the
    host test: ties to the higher index, the voicing constant added before the arg-max, the normaliser dropped."""
    lov = np.asarray(lov, np.float32).astype(np.float64)
    lou = np.asarray(lou, np.float32).astype(np.float64)
    T, P = lov.shape
    W = width
    better = (lambda c, b: c >= b) if tie_high else (lambda c, b: c > b)
    delta = np.concatenate([lov[0] + log_init, np.full(P, lou[0] + log_init)])
    back = np.zeros((T, 2 * P), np.uint16)
    back[0] = np.arange(2 * P)
    with np.errstate(invalid="ignore"):
        for t in range(1, T):
            norm = log_norm if normalise else np.zeros(P)
            e_v, e_u = delta[:P] - norm, delta[P:] - norm
            new = np.empty(2 * P)
            for j in range(P):
                for target, (c_v, c_u), o in ((j, (log_stay, log_switch), lov[t, j]), (P + j, (log_switch, log_stay), lou[t])):
                    first = True
                    for i in range(max(0, j - W), min(P - 1, j + W) + 1):
                        cv, cu = e_v[i] + log_tri[j - i + W], e_u[i] + log_tri[j - i + W]
                        if add_first:
                            cv, cu = cv + c_v, cu + c_u
                        if first:
                            bv, iv, bu, iu, first = cv, i, cu, i, False
                        else:
                            if better(cv, bv):
                                bv, iv = cv, i
                            if better(cu, bu):
                                bu, iu = cu, i
                    a, b = (bv, bu) if add_first else (bv + c_v, bu + c_u)
                    if better(b, a) if tie_high else b > a:
                        a, iv = b, P + iu
                    new[target] = o + a
                    back[t, target] = iv
            delta = new
        best, s = delta[0], 0
        for k in range(1, 2 * P):
            if better(delta[k], best):
                best, s = delta[k], k
    states = np.zeros(T, np.int32)
    states[T - 1] = s
    for t in range(T - 1, 0, -1):
        states[t - 1] = back[t, states[t]]
    return delta, back, states


def viterbi(lov, lou, width, log_tri, log_norm, log_init, log_stay, log_switch, reach=None):
    """The same decoder vectorised over the target bins (a frame at a time, both voicings at once).  np.argmax returns the first
    maximum, which is the scan's rule while no NaN is involved; a window of nothing but -inf keeps its first element.  A NaN among the
    observations follows the scalar rule in vector form — a NaN is never strictly greater and nothing is strictly greater than one, so a
    window whose first candidate is a NaN keeps it and a NaN further on is passed over; a NaN in a table goes through the scalar loop
    (tests/test_pyin_host.py and tests/test_decoders_host.py hold the two together bit for bit).  ``reach`` (None: the definition) is the deliberate defect of tests/test_decoders_host.py: the
    kernel's scan clamp — it walks the offsets -reach .. reach, the definition's being min(W, P - 1) — set to another value (no NaN)."""
    lov32, lou32 = np.asarray(lov, np.float32), np.asarray(lou, np.float32)
    if np.isnan(log_tri).any() or np.isnan(log_norm).any():
        return viterbi_loop(lov32, lou32, width, log_tri, log_norm, log_init, log_stay, log_switch)
    lov, lou = lov32.astype(np.float64), lou32.astype(np.float64)
    T, P = lov.shape
    W = width
    delta = np.concatenate([lov[0] + log_init, np.full(P, lou[0] + log_init)])
    back = np.zeros((T, 2 * P), np.uint16)
    back[0] = np.arange(2 * P)
    pad = np.full((2, P + 2 * W), -np.inf)
    # window element k of target j is source i = j - W + k with weight log_tri[j - i + W] = log_tri[2 W - k]
    win = np.lib.stride_tricks.sliding_window_view(pad, 2 * W + 1, axis=1)  # [2, P, 2 W + 1], a view
    tri = np.ascontiguousarray(log_tri[::-1])
    j = np.arange(P)
    i0 = np.maximum(0, j - W)
    valid = (j[:, None] - W + np.arange(2 * W + 1)[None, :] >= 0) & (j[:, None] - W + np.arange(2 * W + 1)[None, :] <= P - 1)
    masked = not np.isfinite(log_tri).all()  # (-inf + a finite weight stays -inf outside the window; any other table entry must not leak in)
    if reach is not None:
        valid, masked = valid & (np.abs(np.arange(2 * W + 1) - W) <= reach)[None, :], True
    buf = np.empty((2, P, 2 * W + 1))
    for t in range(1, T):
        pad[0, W:W + P] = delta[:P] - log_norm
        pad[1, W:W + P] = delta[P:] - log_norm
        np.add(win, tri, out=buf)
        if masked:
            buf[:, ~valid] = -np.inf
        stuck = None
        if np.isnan(pad).any():  # the window's first candidate (element i0 - j + W) decides; every other NaN loses like -inf
            stuck = np.isnan(np.take_along_axis(buf, np.broadcast_to((i0 - j + W)[None, :, None], (2, P, 1)), axis=2)[:, :, 0])
            buf[np.isnan(buf)] = -np.inf
        k = buf.argmax(axis=2)
        best = np.take_along_axis(buf, k[:, :, None], axis=2)[:, :, 0]
        idx = j[None, :] - W + k
        idx = np.where(best == -np.inf, i0[None, :], idx)
        if stuck is not None:
            best, idx = np.where(stuck, np.nan, best), np.where(stuck, i0[None, :], idx)
        bv, bu, iv, iu = best[0], best[1], idx[0], idx[1]
        a, b = bv + log_stay, bu + log_switch
        sw = b > a
        back[t, :P] = np.where(sw, P + iu, iv)
        voiced = lov[t] + np.where(sw, b, a)
        a, b = bv + log_switch, bu + log_stay
        sw = b > a
        back[t, P:] = np.where(sw, P + iu, iv)
        delta = np.concatenate([voiced, lou[t] + np.where(sw, b, a)])
    s = 0 if np.isnan(delta[0]) or (delta == -np.inf).all() else int(np.argmax(np.where(np.isnan(delta), -np.inf, delta)))
    states = np.zeros(T, np.int32)
    states[T - 1] = s
    for t in range(T - 1, 0, -1):
        states[t - 1] = back[t, states[t]]
    return delta, back, states


def path_score(path, lov, lou, width, log_tri, log_norm, log_init, log_stay, log_switch):
    """The score of one state path by the recursion's own operations in its own order (None: a step wider than the window)."""
    lov = np.asarray(lov, np.float32).astype(np.float64)
    lou = np.asarray(lou, np.float32).astype(np.float64)
    P = lov.shape[1]
    o = lambda t, s: lov[t, s] if s < P else lou[t]  # noqa: E731
    score = o(0, path[0]) + log_init
    for t in range(1, len(path)):
        i, j = path[t - 1] % P, path[t] % P
        if abs(j - i) > width:
            return None
        c = (score - log_norm[i]) + log_tri[j - i + width]
        score = o(t, path[t]) + (c + (log_stay if (path[t - 1] < P) == (path[t] < P) else log_switch))
    return score


# Stage B: the GPU case list
B_BINS = (1, 2, 3, 64, 65, 602, 1024)
B_WIDTHS = (0, 1, 50, 128)
B_FRAMES = (1, 2, 3, 257)
B_KINDS = ("random", "integer", "inf_rows", "inf_frame", "nan")


def b_cases():
    """Every (P, W) pair; T and the input kind rotate (the NaN kind never meets T = 1, where there is no frame before it)."""
    cases = []
    for i, P in enumerate(B_BINS):
        for k, W in enumerate(B_WIDTHS):
            c = len(cases)
            T = B_FRAMES[(c + i) % len(B_FRAMES)]
            kind = B_KINDS[(c + 2 * i) % len(B_KINDS)]
            if kind == "nan" and T < 3:
                T = 3
            cases.append({"n_bins": P, "width": W, "n_frames": T, "kind": kind, "seed": 9000 + c})
    assert {c["n_frames"] for c in cases} == set(B_FRAMES) and {c["kind"] for c in cases} == set(B_KINDS)
    return cases


LONG_CASE = {"n_bins": 602, "width": 50, "n_frames": 20000, "kind": "random", "seed": 9999}


def b_case_id(case):
    return "P{n_bins}-W{width}-T{n_frames}-{kind}".format(**case)


def make_logobs(case):
    """(logobs_voiced [T, P] fp32, logobs_unvoiced [T] fp32) of a stage-B case."""
    rng = np.random.default_rng(case["seed"])
    T, P, kind = case["n_frames"], case["n_bins"], case["kind"]
    if kind == "integer":
        lov, lou = -rng.integers(0, 4, (T, P)).astype(np.float32), -rng.integers(0, 4, T).astype(np.float32)
    elif kind == "corners":  # all voiced mass in bin 0 on the even frames and in bin P - 1 on the odd ones: where W >= P - 1 the best
        lov, lou = np.full((T, P), -40.0, np.float32), np.full(T, -30.0, np.float32)  # path takes the widest step there is, every frame
        lov[np.arange(T), np.where(np.arange(T) % 2 == 0, 0, P - 1)] = -rng.integers(0, 2, T).astype(np.float32)
    else:
        lov, lou = np.log(rng.random((T, P)) + 1e-6).astype(np.float32), np.log(rng.random(T) * 0.5 + 1e-6).astype(np.float32)
    if kind == "inf_rows":  # bins that never carry mass, frames without any voiced mass, frames that cannot be unvoiced
        lov[:, rng.random(P) < 0.5] = -np.inf
        lov[rng.random(T) < 0.3] = -np.inf
        lou[rng.random(T) < 0.3] = -np.inf
    elif kind == "inf_frame":
        lov[T // 2], lou[T // 2] = -np.inf, -np.inf
    elif kind == "nan":
        lov[T // 2, P // 2] = np.nan
    return lov, lou


def b_constants(case):
    """(log_tri, log_norm, log_init, log_stay, log_switch) as ar.raw_pyin builds them (switch_prob 0.01)."""
    tri, norm = transition_tables(case["n_bins"], case["width"])
    return tri, norm, -math.log(2 * case["n_bins"]), math.log(1 - 0.01), math.log(0.01)


def b_reference(case):
    lov, lou = make_logobs(case)
    return viterbi(lov, lou, case["width"], *b_constants(case))


# (P, W) pairs, not a cross, on the clamp reach = min(W, P - 1) of the kernel's scan: W = P - 2, P - 1 and >= P with one wave (P = 63,
# 64), across the 64 / 65 boundary (P = 65) and with two waves and the first lane of a third (P = 127, 128, 129).
EDGE_CASES = ((63, 62), (64, 63), (64, 64), (65, 63), (65, 64), (65, 65), (127, 126), (127, 128), (128, 127), (128, 128), (129, 128),
              (64, 62), (128, 126))   # (the last two: W = P - 2 with one full wave and with two, which the pairs before them lack)
EDGE_FRAMES = (2, 3, 257)
EDGE_KINDS = ("integer", "random", "corners")   # (with the first two alone a scan one offset short goes unnoticed: the far source never wins)


def edge_cases():
    """Every pair with every kind; T rotates, so that every pair meets all three lengths."""
    return [{"n_bins": P, "width": W, "n_frames": EDGE_FRAMES[(n + k) % len(EDGE_FRAMES)], "kind": kind, "seed": 9500 + 3 * n + k}
            for n, (P, W) in enumerate(EDGE_CASES) for k, kind in enumerate(EDGE_KINDS)]


def integer_constants(n_bins, width):
    """(log_tri, log_norm, log_init, log_stay, log_switch), all integer-valued: with the integer kind of make_logobs every sum of the
    recursion is exact, so ties are real ties and two orders of the same additions give the same bits."""
    d = np.arange(-width, width + 1)
    return -np.abs(d).astype(np.float64), np.arange(n_bins, dtype=np.float64) % 2, -1.0, 0.0, -1.0


def expand(n_bins, width, log_tri, log_norm, log_init, log_stay, log_switch):
    """(log_trans [2 P, 2 P], log_init [2 P]) of the model with every state written out, voiced 0 .. P - 1 then unvoiced P .. 2 P - 1:
    the operands of hmm_ref.viterbi, whose observations are [lov | lou repeated P times].  Entry (i, j) is (-log_norm[i % P] +
    log_tri[(j % P) - (i % P) + W]) + (log_stay within a voicing, log_switch across), -inf where the bins lie further than W apart."""
    P, W = n_bins, width
    tri, norm = np.asarray(log_tri, np.float64), np.asarray(log_norm, np.float64)
    lt = np.full((2 * P, 2 * P), -np.inf)
    for i in range(2 * P):
        for j in range(2 * P):
            d = j % P - i % P
            if abs(d) <= W:
                lt[i, j] = (-norm[i % P] + tri[d + W]) + (log_stay if (i < P) == (j < P) else log_switch)
    return lt, np.full(2 * P, np.float64(log_init))


def dense_observations(lov, lou):
    lov, lou = np.asarray(lov, np.float32), np.asarray(lou, np.float32)
    return np.concatenate([lov, np.repeat(lou[:, None], lov.shape[1], axis=1)], axis=1)


# ------------------------------------------------------------------------------------------------ the whole tracker on the host
def pyin(y, sr, fmin=65.0, fmax=2100.0, frame_length=2048, hop=512, bins_per_semitone=10, max_transition_rate=35.92, switch_prob=0.01,
         no_trough_prob=0.01, beta=(2, 18), n_thresholds=100, first_only=True, decoder=None):
    """ar.raw_pyin on the host: the float64 YIN d' of pitch_ref rounded to fp32 (what the device kernel hands over), stage A in fp32,
    the logarithms in fp32, stage B -> dict(f0, voiced_flag, voiced_prob, states, obs, period, logobs_voiced, logobs_unvoiced)."""
    tau_min, tau_max = int(math.floor(sr / fmax)), int(math.ceil(sr / fmin))
    dp = pr.yin(y, frame_length, hop, tau_min, tau_max, 0.1)["cmndf"].astype(np.float32)
    return pyin_from_cmndf(dp, sr, tau_min, tau_max, fmin, fmax, hop, bins_per_semitone, max_transition_rate, switch_prob, no_trough_prob,
                           beta, n_thresholds, first_only, decoder)


def pyin_from_cmndf(dp, sr, tau_min, tau_max, fmin=65.0, fmax=2100.0, hop=512, bins_per_semitone=10, max_transition_rate=35.92,
                    switch_prob=0.01, no_trough_prob=0.01, beta=(2, 18), n_thresholds=100, first_only=True, decoder=None):
    P = pitch_bins(fmin, fmax, bins_per_semitone)
    W = transition_width(max_transition_rate, hop, sr, bins_per_semitone)
    a = candidates(dp, tau_min, tau_max, threshold_prior(n_thresholds, beta), n_thresholds, no_trough_prob,
                   bin_edges(sr, fmin, bins_per_semitone, P), first_only=first_only)
    tiny = np.float32(FLT_MIN)
    lov = np.log(np.maximum(a["obs"], tiny))
    lou = np.log(np.maximum((np.float32(1) - a["voiced_prob"]) / np.float32(P), tiny))
    tri, norm = transition_tables(P, W)
    _, _, states = (decoder or viterbi)(lov, lou, W, tri, norm, -math.log(2 * P), math.log(1 - switch_prob), math.log(switch_prob))
    out = decode(states, a["period"], sr, fmin, bins_per_semitone, P)
    out.update(voiced_prob=a["voiced_prob"], states=states, obs=a["obs"], period=a["period"], logobs_voiced=lov, logobs_unvoiced=lou)
    return out


def decode(states, period, sr, fmin, bins_per_semitone, n_bins):
    """f0 = sr / period[t, bin] where a candidate sits in the decoded bin, the bin's centre frequency otherwise; voiced = state < P."""
    states = np.asarray(states, np.int64)
    b = states % n_bins
    per = np.asarray(period, np.float64)[np.arange(len(states)), b]
    with np.errstate(divide="ignore"):
        f0 = np.where(per > 0, sr / per, bin_centres(fmin, bins_per_semitone, n_bins)[b])
    return {"f0": f0, "voiced_flag": states < n_bins}


def noisy_tone(freq, snr_db, seed=5):
    """pitch_ref.tone("harmonics", freq, 1 s) + white noise of RMS = tone RMS x 10^(-SNR / 20), fp32."""
    y = pr.tone("harmonics", freq, seconds=1.0).astype(np.float64)
    rng = np.random.default_rng(seed)
    noise = rng.standard_normal(len(y)) * np.sqrt(np.mean(y * y)) * 10 ** (-snr_db / 20)
    return (y + noise).astype(np.float32)


INTERIOR = slice(4, -4)


def yin_f0(y, sr=pr.TONE_SR):
    r = pr.yin(y, pr.TONE_FRAME, pr.TONE_HOP, pr.TONE_TAU_MIN, pr.TONE_TAU_MAX, pr.TONE_THRESHOLD)
    return sr / r["lag"]


def arpeggio_frame_sets(hop=512, frame=2048, tau_max=340):
    """(inside [(frame index, note frequency)], silent [frame index]): frames whose L = frame + tau_max samples lie inside one note, and
    frames that read nothing but silence (or padding)."""
    y, spans = pr.arpeggio()
    span = frame + tau_max
    inside, silent = [], []
    for t in range(1 + len(y) // hop):
        lo, hi = t * hop - span // 2, t * hop - span // 2 + span
        for a, b, f in spans:
            if lo >= a and hi <= b:
                inside.append((t, f))
        if all(hi <= a or lo >= b for a, b, _ in spans):
            silent.append(t)
    return inside, silent


def pyin_pipeline(f0, voiced_flag, voiced_prob, n_frames, fmin, fmax, smooth=2, dtype=np.float64):
    """Steps after raw_pyin of ar.pitch(method="pyin"): log height, hold-fill on the voiced flag, linear interpolation, Gaussian
    smoothing (no median) -> (height, voicing envelope)."""
    h = pr.hold_fill(pr.height(f0, fmin, fmax, dtype), voiced_flag)
    h = np.zeros(len(f0), dtype) if h is None else h
    return (pr.gaussian_smooth(pr.lerp_resize(h, n_frames, dtype), smooth, dtype=dtype),
            pr.gaussian_smooth(pr.lerp_resize(np.asarray(voiced_prob, dtype), n_frames, dtype), smooth, dtype=dtype))


def main():
    worst_rel, exempt, frames = 0.0, 0, 0
    cases = a_cases()
    for case in cases:
        _, edges = case_tables(case)
        r32, r64 = a_reference(case), a_reference(case, np.float64)
        both = (r32["period"] > 0) & (r64["period"] > 0)
        if both.any():
            worst_rel = max(worst_rel, float(np.max(np.abs(r32["period"][both].astype(np.float64) - r64["period"][both]) / r64["period"][both])))
        n = int(near_edge_frames(r32, edges).sum())
        assert n <= max_exempt(case["n_frames"]), (a_case_id(case), n)
        exempt += n
        frames += case["n_frames"]
    print(f"stage A, {len(cases)} cases, {frames} frames, {exempt} exempt (a period within 2 x the tolerance of a bin edge)")
    print(f"period, fp32 against float64: worst relative error {worst_rel:.3g}")
    for (freq, snr), quoted in zip(NOISY_CASES, NOISY_WORST_CENTS):
        y = noisy_tone(freq, snr)
        got = pyin(y, pr.TONE_SR)
        c = pr.cents(got["f0"][INTERIOR], freq)
        wrong = float(np.mean(pr.cents(yin_f0(y)[INTERIOR], freq) > 50))
        print(f"{freq:.0f} Hz at {snr:.0f} dB: pYIN worst {c.max():.1f} cents (quoted {quoted}), {int((c > 50).sum())} frames over 50 cents, "
              f"{int((~got['voiced_flag'][INTERIOR]).sum())} unvoiced of {len(c)};  YIN over 50 cents on {100 * wrong:.0f} %")
    y, _ = pr.arpeggio()
    got = pyin(y, pr.TONE_SR)
    inside, silent = arpeggio_frame_sets()
    c = max(float(pr.cents(got["f0"][t], f)) for t, f in inside)
    print(f"arpeggio: {len(inside)} frames inside a note, all voiced {all(got['voiced_flag'][t] for t, _ in inside)}, worst {c:.3f} cents;  "
          f"{len(silent)} silent frames, all unvoiced {not any(got['voiced_flag'][t] for t in silent)}, "
          f"voiced probability <= {max(float(got['voiced_prob'][t]) for t in silent):.3f}")
    h64, v64 = pyin_pipeline(got["f0"], got["voiced_flag"], got["voiced_prob"], pr.ARPEGGIO_FRAMES, pr.ARPEGGIO_FMIN, pr.ARPEGGIO_FMAX)
    h32, v32 = pyin_pipeline(got["f0"].astype(np.float32), got["voiced_flag"], got["voiced_prob"], pr.ARPEGGIO_FRAMES, pr.ARPEGGIO_FMIN,
                             pr.ARPEGGIO_FMAX, dtype=np.float32)
    print(f"ar.pitch(method='pyin') steps in fp32 against float64 on the arpeggio: height {np.abs(h32 - h64).max():.3g}   "
          f"voicing {np.abs(v32 - v64).max():.3g}")


if __name__ == "__main__":
    main()
