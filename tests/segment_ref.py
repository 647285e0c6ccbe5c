"""CPU restatement of laplacian_segmentation (numpy / scipy, fp64), stage by stage, for the tests of audioreactive/segment.py.

Written from the recipe (librosa 0.8's beat tracker, recurrence matrix, time-lag filter and Laplacian segmentation as the
reference calls them), not from the device code: loops are plain Python where that is the clearest statement."""
import math

import numpy as np
import scipy.ndimage
import scipy.signal

from oracle import signal_oracle as so

HOP = 512


def np_median(x, axis=None):
    return np.median(x, axis=axis)


# ------------------------------------------------------------------------------------------------ 1. onset envelope
def onset_envelope(y, sr):
    power = so.stft_power(y, 2048, HOP)
    db = so.power_to_db(so.mel_filterbank(sr, 2048, 128) @ power)
    flux = np.median(np.maximum(0.0, np.diff(db, axis=1)), axis=0)
    return np.concatenate([np.zeros(3), flux])[: db.shape[1]], power


# ------------------------------------------------------------------------------------------------ 2. tempo
def tempogram_mean(env, win):
    env = np.asarray(env, dtype=np.float64)
    n = env.size
    padded = np.pad(env, win // 2, mode="linear_ramp", end_values=0)
    window = scipy.signal.get_window("hann", win, fftbins=True)
    total = np.zeros(win)
    for t in range(n):
        f = padded[t: t + win] * window
        ac = np.array([np.dot(f[: win - lag], f[lag:]) for lag in range(win)])
        peak = np.abs(ac).max()
        total += ac / peak if peak >= np.finfo(np.float32).tiny else ac
    return total / n


def tempo(tg, sr):
    bpm = np.full(tg.size, np.inf)
    bpm[1:] = 60.0 * sr / (HOP * np.arange(1, tg.size))
    with np.errstate(divide="ignore"):
        prior = -0.5 * (np.log2(bpm) - np.log2(120.0)) ** 2
    first = int(np.flatnonzero(bpm < 320.0)[0])
    prior[:first] = -np.inf
    return bpm[np.argmax(np.log1p(1e6 * np.asarray(tg, np.float64)) + prior)]


# ------------------------------------------------------------------------------------------------ 3. beats
def localscore(env, period, normalise=True):
    """The envelope over its sample std (``normalise``; left alone when already normalised by the caller) convolved with the Gaussian
    taps, scipy's 'same': n values for every n, also where the 2 period + 1 taps are longer than the envelope (np.convolve's "same"
    returns max(n, taps) values there)."""
    x = np.asarray(env, dtype=np.float64)
    if normalise and x.size > 1:
        sd = x.std(ddof=1)
        if sd > 0:
            x = x / sd
    taps = np.exp(-0.5 * (np.arange(-period, period + 1) * 32.0 / period) ** 2)
    return np.convolve(x, taps, mode="full")[period: period + x.size]


def beat_dp_margins(ls, period):
    """beat_dp with two measurements of how unambiguous its decisions are: ``min_gap``, the smallest difference between the best and
    the second-best candidate over all frames, and ``min_threshold_gap``, the smallest |ls[i] - 0.01 max ls| over the frames
    before the first beat (those whose backlink is -1).  inf where nothing is decided."""
    ls = np.asarray(ls, dtype=np.float64)
    n = ls.size
    offsets = np.arange(-2 * period, -int(np.round(period / 2)) + 1)
    weight = -100.0 * np.log(-offsets / period) ** 2
    thr = 0.01 * ls.max()
    cum = np.zeros(n)
    back = np.zeros(n, dtype=np.int64)
    started = False
    min_gap = min_thr = np.inf
    for i in range(n):
        prev = i + offsets
        score = weight + np.where(prev >= 0, cum[np.maximum(prev, 0)], 0.0)
        best = int(np.argmax(score))
        if score.size > 1:
            top = np.partition(score, score.size - 2)[-2:]
            min_gap = min(min_gap, float(top[1] - top[0]))
        cum[i] = ls[i] + score[best]
        if not started and ls[i] < thr:
            back[i] = -1
            min_thr = min(min_thr, float(thr - ls[i]))
        else:
            back[i] = prev[best]
            started = True
    return cum, back, min_gap, min_thr


def beat_dp(ls, period):
    cum, back, _, _ = beat_dp_margins(ls, period)
    return cum, back


def beats_from_dp(ls, cum, back):
    padded = np.concatenate([cum[:1], cum, cum[-1:]])
    peak = (cum > padded[:-2]) & (cum >= padded[2:])
    med = np.median(cum[peak])
    last = np.flatnonzero(cum * peak * 2 > med).max()
    path = [last]
    while back[path[-1]] >= 0:
        path.append(back[path[-1]])
    beats = np.array(path[::-1])
    smooth = scipy.signal.convolve(ls[beats], scipy.signal.windows.hann(5), "same")
    valid = np.flatnonzero(smooth > 0)
    return beats[valid.min(): valid.max()]


def beat_track(env, sr):
    win = int(8.0 * sr) // HOP
    bpm = tempo(tempogram_mean(env, win), sr)
    period = int(round(60.0 * sr / HOP / bpm))
    ls = localscore(env, period)
    cum, back = beat_dp(ls, period)
    return bpm, period, ls, cum, back, beats_from_dp(ls, cum, back)


# ------------------------------------------------------------------------------------------------ 4-5. features, sync
def features(y, sr, power):
    tuning = so.estimate_tuning(y, sr, bins_per_octave=36)
    cqt = so.cqt_magnitude(y, sr, fmin=32.70319566257483 * 2.0 ** (tuning / 36))
    c = 20.0 * np.log10(np.maximum(1e-5, cqt)) - 20.0 * np.log10(max(1e-5, cqt.max()))
    c = np.maximum(c, c.max() - 80.0)
    db = so.power_to_db(so.mel_filterbank(sr, 2048, 128) @ power)
    n = db.shape[0]
    basis = np.array([[math.cos(math.pi * q * (2 * m + 1) / (2 * n)) for m in range(n)] for q in range(20)]) * math.sqrt(2.0 / n)
    basis[0] *= math.sqrt(0.5)
    return c, basis @ db


def sync_spans(beats, n_frames):
    edges = np.unique(np.clip(np.concatenate([[0], beats, [n_frames]]), 0, n_frames)).astype(int)
    return list(zip(edges[:-1], edges[1:]))


def sync(x, spans, how):
    return np.stack([how(x[:, a:b], axis=1) for a, b in spans], axis=1)


def clamp_bounds(bounds, n_frames):
    """The bounds table as the header reads it: every bound inside [0, n_frames] and none below the one before it."""
    return np.maximum.accumulate(np.clip(np.asarray(bounds, dtype=np.int64), 0, n_frames))


def beat_sync_ref(x, bounds, median):
    """out[r][s] over x[r][b[s] .. b[s + 1]) with b = clamp_bounds(bounds): the float32 median (the middle element of the sorted span,
    or the float32 mean of the two middle ones), or the float64 mean rounded to float32; NaN for an empty span."""
    x = np.asarray(x, dtype=np.float32)
    b = clamp_bounds(bounds, x.shape[1])
    out = np.full((x.shape[0], len(b) - 1), np.nan, dtype=np.float32)
    for s, (lo, hi) in enumerate(zip(b[:-1], b[1:])):
        n = int(hi - lo)
        if n == 0:
            continue
        if median:
            srt = np.sort(x[:, lo:hi], axis=1)
            with np.errstate(invalid="ignore"):  # (inf + -inf in a span that holds both)
                out[:, s] = srt[:, n // 2] if n & 1 else (srt[:, n // 2 - 1] + srt[:, n // 2]) * np.float32(0.5)
        else:
            with np.errstate(invalid="ignore"):
                out[:, s] = x[:, lo:hi].astype(np.float64).mean(axis=1).astype(np.float32)
    return out


# ------------------------------------------------------------------------------------------------ 6. recurrence
def knn_k(n, width=3):
    return int(2 * math.ceil(math.sqrt(n - 2 * width + 1))) if n > 2 * width + 1 else 2


def pair_distances(x):
    """fp32 Euclidean distances, squares summed feature by feature in fp32 (x [D, S])."""
    x = np.asarray(x, dtype=np.float32)
    d = np.zeros((x.shape[1], x.shape[1]), dtype=np.float32)
    for f in range(x.shape[0]):
        diff = x[f][:, None] - x[f][None, :]
        d = (d + diff * diff).astype(np.float32)
    return np.sqrt(d)


def knn_sets(dist, k, width=3):
    """Row i -> the k columns j with |i - j| >= width of smallest distance, ties to the lower j."""
    s = dist.shape[0]
    out = []
    for i in range(s):
        cand = [j for j in range(s) if abs(i - j) >= width]
        cand.sort(key=lambda j: (dist[i, j], j))
        out.append(set(cand[:k]))
    return out


def pair_distances_rows(x, rows):
    """pair_distances for the rows ``rows`` only: [len(rows), S]."""
    x = np.asarray(x, dtype=np.float32)
    d = np.zeros((len(rows), x.shape[1]), dtype=np.float32)
    for f in range(x.shape[0]):
        diff = x[f][rows, None] - x[f][None, :]
        d = (d + diff * diff).astype(np.float32)
    return np.sqrt(d)


def knn_links_exact(x, k, width, rows=None, block=512):
    """The link matrix itself, float32 [S, S] (or [len(rows), S] for the rows asked for): the fp32 distances of pair_distances, the band
    |i - j| < width set to +inf, a stable argsort per row (ties to the lower j), the first min(k, columns outside the band) columns
    keep their distance, every other cell is -1.  Computed ``block`` rows at a time."""
    x = np.asarray(x, dtype=np.float32)
    s = x.shape[1]
    rows = np.arange(s) if rows is None else np.asarray(rows, dtype=np.int64)
    out = np.full((len(rows), s), -1.0, dtype=np.float32)
    cols = np.arange(s)
    for a in range(0, len(rows), block):
        r = rows[a: a + block]
        dist = pair_distances_rows(x, r)
        band = np.abs(r[:, None] - cols[None, :]) < width
        order = np.argsort(np.where(band, np.float32(np.inf), dist), axis=1, kind="stable")
        n_valid = s - band.sum(axis=1)
        keep = np.arange(s)[None, :] < np.minimum(k, n_valid)[:, None]  # by rank
        ri = np.broadcast_to(np.arange(len(r))[:, None], order.shape)
        out[a + ri[keep], order[keep]] = dist[ri[keep], order[keep]]
    return out


def affinity_from_links(links, bandwidth):
    """rec (fp64) of a link matrix (distance on a link, negative elsewhere): exp(-d / bandwidth) where i links j AND j links i, else 0."""
    links = np.asarray(links)
    mutual = (links >= 0) & (links.T >= 0)
    return np.where(mutual, np.exp(-np.where(mutual, links, 0).astype(np.float64) / float(bandwidth)), 0.0)


def affinity(dist, sets):
    s = dist.shape[0]
    linked = np.zeros((s, s), dtype=bool)
    for i, js in enumerate(sets):
        linked[i, list(js)] = True
    mutual = linked & linked.T
    rowmax = [dist[i][mutual[i]].max() for i in range(s) if mutual[i].any()]
    bw = float(np.median(rowmax))
    rec = np.where(mutual, np.exp(-dist.astype(np.float64) / bw), 0.0)
    return rec, bw, linked


def timelag_median_formula(rec):
    s = rec.shape[0]
    out = np.zeros_like(rec)
    for i in range(s):
        for j in range(s):
            vals = []
            for sh in range(-3, 4):
                jp = j + sh
                jp = -jp - 1 if jp < 0 else (2 * s - jp - 1 if jp >= s else jp)
                r = i - j + jp
                vals.append(rec[r, jp] if 0 <= r < s else 0.0)
            out[i, j] = sorted(vals)[3]  # the median of seven
    return out


def timelag_median_literal(rec):
    """The lag-matrix route itself: pad S zero rows, shear columns by -j, median filter (1, 7) in 'reflect' mode, shear back."""
    s = rec.shape[0]
    padded = np.concatenate([rec, np.zeros_like(rec)], axis=0)
    lag = np.stack([np.roll(padded[:, j], -j) for j in range(s)], axis=1)
    lag = scipy.ndimage.median_filter(lag, size=(1, 7), mode="reflect")
    back = np.stack([np.roll(lag[:, j], j) for j in range(s)], axis=1)
    return back[:s]


# ------------------------------------------------------------------------------------------------ 8. Laplacian embedding
def embedding(rf, msync, k):
    pd = np.sum(np.diff(msync.astype(np.float64), axis=1) ** 2, axis=0)
    path = np.exp(-pd / np.median(pd))
    r_path = np.diag(path, 1) + np.diag(path, -1)
    deg_path, deg_rec = r_path.sum(1), rf.sum(1)
    mu = deg_path.dot(deg_path + deg_rec) / np.sum((deg_path + deg_rec) ** 2)
    a = mu * rf + (1 - mu) * r_path
    import scipy.sparse.csgraph

    lap = scipy.sparse.csgraph.laplacian(a, normed=True)
    _, evecs = np.linalg.eigh(lap)
    evecs = scipy.ndimage.median_filter(evecs, size=(9, 1), mode="reflect")
    cnorm = np.cumsum(evecs ** 2, axis=1) ** 0.5
    return evecs[:, :k] / cnorm[:, k - 1: k]


def lloyd(x, k, seed=0, n_init=10):
    """Plain k-means++ (one candidate per centre) + Lloyd iterations, best of n_init by inertia."""
    rng = np.random.default_rng(seed)
    best, best_inertia = None, np.inf
    for _ in range(n_init):
        centers = [x[rng.integers(len(x))]]
        for _c in range(1, k):
            d2 = np.min([((x - c) ** 2).sum(1) for c in centers], axis=0)
            centers.append(x[rng.choice(len(x), p=d2 / d2.sum())] if d2.sum() > 0 else x[rng.integers(len(x))])
        centers = np.array(centers)
        for _it in range(300):
            lab = np.argmin(((x[:, None] - centers[None]) ** 2).sum(2), axis=1)
            new = np.array([x[lab == c].mean(0) if (lab == c).any() else centers[c] for c in range(k)])
            if np.allclose(new, centers):
                break
            centers = new
        inertia = ((x - centers[lab]) ** 2).sum()
        if inertia < best_inertia:
            best, best_inertia = lab, inertia
    return best


def first_appearance(seg):
    seen = {}
    return np.array([seen.setdefault(v, len(seen)) for v in seg.tolist()])


def segment(y, sr, k):
    """Whole recipe: (times, labels, per-column partition, beats)."""
    env, power = onset_envelope(y, sr)
    _, _, _, _, _, beats = beat_track(env, sr)
    c, m = features(y, sr, power)
    spans = sync_spans(beats, c.shape[1])
    csync = sync(c.astype(np.float32), spans, np.median)
    msync = sync(m.astype(np.float32), spans, np.mean)
    dist = pair_distances(csync)
    rec, _, _ = affinity(dist, knn_sets(dist, knn_k(len(spans))))
    rf = timelag_median_formula(rec)
    seg = first_appearance(lloyd(embedding(rf, msync, k), k))
    bound = np.concatenate([[0], 1 + np.flatnonzero(seg[:-1] != seg[1:])])
    bound = bound[bound < len(beats)]
    frames = np.concatenate([beats[bound], [c.shape[1] - 1]])
    times = frames * HOP / sr
    times[0] = 0.0
    return list(times), list(seg[bound]), seg, beats


# ------------------------------------------------------------------------------------------------ synthetic tracks
def click_track(bpm, seconds, sr=22050, seed=0):
    rng = np.random.default_rng(seed)
    y = 1e-3 * rng.standard_normal(int(seconds * sr))
    step = 60.0 / bpm
    click = np.exp(-np.arange(int(0.03 * sr)) / (0.004 * sr)) * np.sin(2 * np.pi * 1500 * np.arange(int(0.03 * sr)) / sr)
    t = 0.25
    while t < seconds - 0.05:
        a = int(t * sr)
        y[a: a + click.size] += click[: y.size - a]
        t += step
    return y.astype(np.float32)


def noise_burst_track(seconds, sr=22050, seed=0):
    rng = np.random.default_rng(seed)
    y = 1e-3 * rng.standard_normal(int(seconds * sr))
    t = 0.1
    while t < seconds - 0.2:
        a = int(t * sr)
        n = int(rng.uniform(0.02, 0.08) * sr)
        y[a: a + n] += rng.uniform(0.2, 1.0) * rng.standard_normal(n) * np.exp(-np.arange(n) / (0.3 * n))
        t += rng.uniform(0.2, 0.7)
    return y.astype(np.float32)


SECTION_CHORDS = {"A": (220.0, 277.18, 329.63), "B": (146.83, 185.0, 220.0), "C": (196.0, 246.94, 293.66)}


def sectioned_track(order="ABAC", beats_per_section=16, bpm=120, sr=22050, seed=0):
    """Sections of distinct harmonic content (a sustained chord, with a kick on every beat), seeded low-level noise throughout."""
    rng = np.random.default_rng(seed)
    beat = 60.0 / bpm
    sec = beats_per_section * beat
    n = int(len(order) * sec * sr)
    t = np.arange(n) / sr
    y = 2e-3 * rng.standard_normal(n)
    for s, name in enumerate(order):
        a, b = int(s * sec * sr), int((s + 1) * sec * sr)
        for f in SECTION_CHORDS[name]:
            y[a:b] += 0.15 * np.sin(2 * np.pi * f * t[a:b]) + 0.05 * np.sin(2 * np.pi * 2 * f * t[a:b])
    kick_n = int(0.08 * sr)
    kick = np.sin(2 * np.pi * 60 * np.arange(kick_n) / sr) * np.exp(-np.arange(kick_n) / (0.02 * sr))
    for q in range(int(len(order) * beats_per_section)):
        a = int(q * beat * sr)
        y[a: a + kick_n] += 0.8 * kick[: max(0, min(kick_n, n - a))]
    return y.astype(np.float32)
