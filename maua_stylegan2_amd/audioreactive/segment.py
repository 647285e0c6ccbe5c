"""Structural segmentation of a track (the reference's ``audioreactive.signal.laplacian_segmentation``, librosa 0.8's Laplacian
segmentation recipe) on the MI355X.

Pipeline: beat tracking (median-aggregated onset envelope -> autocorrelation tempogram -> tempo -> dynamic-programming beat
search), beat-synchronous constant-Q dB and MFCC features, a k-nearest-neighbour recurrence graph with its time-lag median
filter, an MFCC path graph, the normalised Laplacian of their balanced sum, its eigenvectors, k-means.  The tempogram, the beat
search, the beat-synchronous aggregation, the neighbour search and the affinity / time-lag median are HIP kernels
(csrc/segment.hip); the STFT, mel / DCT projections and the constant-Q transform are the existing ones (csrc/signal.hip); eigh,
the Laplacian assembly and the small reductions are torch on the same device; k-means runs on the host over [beats, k].
"""
import math

import numpy as np
import torch as th

from .. import _lib
from . import signal as _sig

HOP = 512
N_FFT = 2048
WIDTH = 3  # recurrence band: links need |i - j| >= WIDTH


# ------------------------------------------------------------------------------------------------ host helpers
def np_median(x, dim=0):
    """np.median along ``dim`` of a tensor: the mean of the two middle values for an even count (torch.median takes the lower)."""
    v = x.sort(dim=dim).values
    n = v.shape[dim]
    return 0.5 * (v.narrow(dim, (n - 1) // 2, 1) + v.narrow(dim, n // 2, 1)).squeeze(dim)


def dct_matrix(n_out, n_in):
    """Orthonormal DCT-II rows [n_out, n_in] (scipy.fftpack.dct(type=2, norm='ortho'))."""
    k = np.arange(n_out)[:, None]
    n = np.arange(n_in)[None, :]
    m = np.cos(np.pi * k * (2 * n + 1) / (2.0 * n_in)) * np.sqrt(2.0 / n_in)
    m[0] /= np.sqrt(2.0)
    return m.astype(np.float32)


def tempo_from_tempogram(tg, sr, hop=HOP, start_bpm=120.0, max_tempo=320.0):
    """bpm of the argmax of log1p(1e6 tg) + a log-normal prior around ``start_bpm`` (librosa.beat.tempo)."""
    tg = np.asarray(tg, dtype=np.float64)
    bpm = np.empty(tg.shape[0])
    bpm[0] = np.inf
    bpm[1:] = 60.0 * sr / (hop * np.arange(1.0, tg.shape[0]))
    with np.errstate(divide="ignore", invalid="ignore"):
        logprior = -0.5 * (np.log2(bpm) - np.log2(start_bpm)) ** 2
    logprior[: int(np.argmax(bpm < max_tempo))] = -np.inf
    return float(bpm[int(np.argmax(np.log1p(1e6 * tg) + logprior))])


def last_beat(cumscore):
    """Last local maximum of the cumulative score above half the median of its local maxima (librosa.beat's __last_beat)."""
    x = np.asarray(cumscore)
    prev = np.concatenate([x[:1], x[:-1]])
    nxt = np.concatenate([x[1:], x[-1:]])
    maxes = (x > prev) & (x >= nxt)
    med = np.median(x[maxes])
    return int(np.flatnonzero(x * maxes * 2 > med).max())


def trim_beats(localscore, beats):
    """trim=False form of librosa.beat's __trim_beats: smooth localscore[beats] with the 5-point Hann [0, .5, 1, .5, 0] and keep
    beats[first positive : last positive] (the slice drops the last positive beat, as the reference does)."""
    if len(beats) == 0:
        return beats
    smooth = np.convolve(np.asarray(localscore)[beats], [0.0, 0.5, 1.0, 0.5, 0.0], mode="same")
    valid = np.flatnonzero(smooth > 0.0)
    if valid.size == 0:
        return beats[:0]
    return beats[valid.min(): valid.max()]


def sync_bounds(beats, n_frames):
    """[0] + beats + [n_frames], clipped, unique and sorted (librosa.util.fix_frames(pad=True)): spans of the sync columns."""
    return np.unique(np.clip(np.concatenate([[0], np.asarray(beats, dtype=np.int64), [n_frames]]), 0, n_frames))


def knn_count(n_cols, width=WIDTH):
    """librosa.segment.recurrence_matrix's default k."""
    return int(2 * math.ceil(math.sqrt(n_cols - 2 * width + 1))) if n_cols > 2 * width + 1 else 2


def check_arguments(sr, k):
    if not isinstance(k, (int, np.integer)) or isinstance(k, bool) or k < 1:
        raise ValueError(f"laplacian_segmentation: k must be a positive integer (got {k!r})")
    if not sr > 0:
        raise ValueError(f"laplacian_segmentation: sr must be positive (got {sr!r})")


def check_columns(n_cols, k, width=WIDTH):
    need = max(int(k), 2 * width + 1)
    if n_cols < need:
        raise ValueError(f"laplacian_segmentation: {n_cols} beat-synchronous columns, need at least {need} for k={k} — the track is too "
                         "short, silent or has too few beats to segment")


def kmeans(x, k, n_init=10, seed=0, max_iter=300, tol=1e-4):
    """Deterministic k-means (seeded greedy k-means++, ``n_init`` runs, lowest inertia) of the rows of ``x`` -> labels [n]."""
    x = np.asarray(x, dtype=np.float64)
    n = x.shape[0]
    rng = np.random.RandomState(seed)
    tol = tol * float(np.mean(np.var(x, axis=0)))
    trials = 2 + int(np.log(k))
    best, best_inertia = None, np.inf
    for _ in range(n_init):
        centers = np.empty((k, x.shape[1]))
        centers[0] = x[rng.randint(n)]
        d2 = ((x - centers[0]) ** 2).sum(1)
        for c in range(1, k):
            total = d2.sum()
            if total > 0:
                cand = np.searchsorted(np.cumsum(d2), rng.random_sample(trials) * total)
                cand = np.minimum(cand, n - 1)
            else:
                cand = rng.randint(n, size=trials)
            cd2 = np.minimum(d2[None, :], ((x[None, :, :] - x[cand][:, None, :]) ** 2).sum(2))
            pick = int(np.argmin(cd2.sum(1)))
            centers[c] = x[cand[pick]]
            d2 = cd2[pick]
        for _ in range(max_iter):
            dist = ((x[:, None, :] - centers[None, :, :]) ** 2).sum(2)
            labels = dist.argmin(1)
            new = np.array([x[labels == c].mean(0) if np.any(labels == c) else centers[c] for c in range(k)])
            shift = ((new - centers) ** 2).sum()
            centers = new
            if shift <= tol:
                break
        dist = ((x[:, None, :] - centers[None, :, :]) ** 2).sum(2)
        labels = dist.argmin(1)
        inertia = float(dist[np.arange(n), labels].sum())
        if inertia < best_inertia:
            best, best_inertia = labels, inertia
    return best


def relabel_first_appearance(seg):
    """Renumber cluster ids so that they appear as 0, 1, 2 ... along the sequence."""
    seg = np.asarray(seg)
    order = {}
    for v in seg.tolist():
        if v not in order:
            order[v] = len(order)
    return np.array([order[v] for v in seg.tolist()], dtype=np.int64)


def segment_boundaries(seg, beats, n_frames, sr, hop=HOP):
    """Step 9 of the recipe on the host: (times, labels) from the per-column cluster ids ``seg`` [S] and the beat frames.
    Boundaries are the first column and every column whose id differs from the previous one; a boundary column is used as an
    index into ``beats`` as the reference does, and one at or past len(beats) is dropped together with its label (the reference
    raises IndexError there).  The last time is the end of the track (frame n_frames - 1), the first is 0."""
    seg = relabel_first_appearance(seg)
    beats = np.asarray(beats, dtype=np.int64)
    bound = np.concatenate([[0], 1 + np.flatnonzero(seg[:-1] != seg[1:])]).astype(np.int64)
    bound = bound[bound < len(beats)]
    labels = [int(v) for v in seg[bound]]
    frames = np.clip(beats[bound], 0, n_frames - 1)
    frames = np.concatenate([frames, [n_frames - 1]])
    times = [float(f) * hop / float(sr) for f in frames]
    times[0] = 0.0
    return times, labels


# ------------------------------------------------------------------------------------------------ device stages
def onset_envelope(audio, sr, n_mels=128):
    """Onset strength for beat tracking: mel power -> dB (80 dB floor) -> positive first difference -> np.median over bands,
    3 leading zero frames (librosa.onset.onset_strength(aggregate=np.median))."""
    p = _sig.stft_power(audio, N_FFT, HOP)
    db = _sig.project(_sig.mel_filterbank(sr, N_FFT, n_mels), p, to_db=True)
    db = th.maximum(db, db.max() - 80.0)
    flux = np_median(th.clamp(db[:, 1:] - db[:, :-1], min=0), dim=0)
    pad = 1 + N_FFT // (2 * HOP)
    return th.cat([th.zeros(pad, device=flux.device), flux])[: db.shape[1]].contiguous(), p


def tempogram(env, win):
    """Mean autocorrelation tempogram tg[win] on the device of an onset envelope, a numpy array or a tensor on any device
    (maua_tempogram_f32)."""
    env = _sig._to_dev(env).reshape(-1)
    n = env.numel()
    ws = th.empty(_lib.load().maua_tempogram_ws_doubles(n, win), dtype=th.float64, device=env.device)
    tg = th.empty(win, dtype=th.float32, device=env.device)
    _lib.call("maua_tempogram_f32", env, n, win, ws, tg)
    return tg


def beat_dp(onset_norm, period):
    """(localscore, cumscore, backlink) device tensors of the beat search over a normalised envelope, a numpy array or a tensor on
    any device, computed in float64 (maua_beat_track_f64)."""
    x = _sig._to_dev(onset_norm, th.float64).reshape(-1)
    n = x.numel()
    ls, cs = th.empty_like(x), th.empty_like(x)
    bl = th.empty(n, dtype=th.int32, device=x.device)
    _lib.call("maua_beat_track_f64", x, n, int(period), ls, cs, bl)
    return ls, cs, bl


def beat_track(env, sr, hop=HOP):
    """(tempo, beat frames) of a device onset envelope (librosa.beat.beat_track(trim=False) with that envelope)."""
    if not bool((env != 0).any()):
        return 0.0, np.zeros(0, dtype=np.int64)
    win = int(8.0 * sr) // hop
    tempo = tempo_from_tempogram(tempogram(env, win).cpu().numpy(), sr, hop)
    period = int(round(60.0 * sr / hop / tempo))
    x = env.double()
    std = float(x.std(unbiased=True)) if x.numel() > 1 else 0.0
    if std > 0:
        x = x / std
    ls, cs, bl = beat_dp(x, period)
    ls, cs, bl = ls.cpu().numpy(), cs.cpu().numpy(), bl.cpu().numpy()
    beats = [last_beat(cs)]
    while bl[beats[-1]] >= 0:
        beats.append(int(bl[beats[-1]]))
    beats = np.array(beats[::-1], dtype=np.int64)
    return tempo, trim_beats(ls, beats)


def beat_sync(x, bounds, median):
    """[rows, len(bounds) - 1] np.median (``median``) or mean of x[rows, n_frames] over the spans (maua_beat_sync_f32), on the device.
    ``x`` and ``bounds`` are numpy arrays or tensors on any device (``bounds`` a list too).  ValueError: an ``x`` that is not a matrix,
    fewer than two bounds, a bound outside 0 .. n_frames."""
    if len(x.shape) != 2:
        raise ValueError(f"beat_sync: x must be [rows, n_frames] (got {tuple(x.shape)})")
    rows, n = x.shape
    edges = np.asarray(bounds.detach().cpu() if isinstance(bounds, th.Tensor) else bounds).reshape(-1)
    if len(edges) < 2 or int(edges.min()) < 0 or int(edges.max()) > n:
        raise ValueError(f"beat_sync: need at least two bounds inside 0 .. {n}, the frame count (got {edges.tolist()})")
    x = _sig._to_dev(x)
    b = _sig._to_dev(edges, th.int32)
    out = th.empty((rows, b.numel() - 1), dtype=th.float32, device=x.device)
    _lib.call("maua_beat_sync_f32", x, rows, n, b, b.numel() - 1, int(bool(median)), out)
    return out


def knn_links(x, k, width=WIDTH):
    """[S, S] links of the columns of x[D, S] (a numpy array or a tensor on any device): the distance where row i links column j, -1
    elsewhere (maua_knn_links_f32)."""
    if len(x.shape) != 2:
        raise ValueError(f"knn_links: x must be [D, S] (got {tuple(x.shape)})")
    x = _sig._to_dev(x)
    d, s = x.shape
    out = th.empty((s, s), dtype=th.float32, device=x.device)
    _lib.call("maua_knn_links_f32", x, d, s, int(k), int(width), out)
    return out


def link_bandwidth(links):
    """np.median over rows with at least one mutual link of the row's largest mutual link distance."""
    mutual = (links >= 0) & (links.t() >= 0)
    rowmax = th.where(mutual, links, th.full_like(links, -1.0)).amax(1)
    has = mutual.any(1)
    if not bool(has.any()):
        raise ValueError("laplacian_segmentation: the recurrence graph has no mutual links")
    return float(np_median(rowmax[has].double()))


def rec_affinity(links, bandwidth):
    """(R, Rf): mutual-link affinity exp(-d / bandwidth) and its time-lag median filter (maua_rec_affinity_f32) of the [S, S] links
    of :func:`knn_links`, a numpy array or a tensor on any device."""
    if len(links.shape) != 2 or links.shape[0] != links.shape[1]:
        raise ValueError(f"rec_affinity: links must be a square matrix [S, S] (got {tuple(links.shape)})")
    links = _sig._to_dev(links)
    s = links.shape[0]
    rec, filt = th.empty_like(links), th.empty_like(links)
    _lib.call("maua_rec_affinity_f32", links, s, float(bandwidth), rec, filt)
    return rec, filt


def spectral_embedding(rf, msync, k):
    """X [S, k] (fp64, device): balanced recurrence + MFCC path graph -> normalised Laplacian -> eigenvectors (ascending),
    median-filtered over 9 beats, cumulatively normalised."""
    m = msync.double()
    pd = ((m[:, 1:] - m[:, :-1]) ** 2).sum(0)
    path = th.exp(-pd / np_median(pd))
    r_path = th.diag(path, 1) + th.diag(path, -1)
    rf = rf.double()
    deg_path, deg_rec = r_path.sum(1), rf.sum(1)
    mu = float(deg_path.dot(deg_path + deg_rec) / ((deg_path + deg_rec) ** 2).sum())
    a = mu * rf + (1 - mu) * r_path
    a.fill_diagonal_(0.0)
    w = a.sum(0)
    isolated = w == 0
    w = th.where(isolated, th.ones_like(w), th.sqrt(w))
    lap = -(a / w) / w[:, None]
    lap.diagonal().copy_((~isolated).double())
    _, evecs = th.linalg.eigh(lap)
    ev32 = evecs.float().contiguous()
    filt = th.empty_like(ev32)
    s = ev32.shape[0]
    _lib.call("maua_median_filter_f32", ev32, filt, s, s, 9, 0)
    ev = filt.double()
    cnorm = th.sqrt((ev[:, :k] ** 2).sum(1))
    return ev[:, :k] / cnorm[:, None]


def features(audio, sr, power):
    """(C [252, n] constant-Q dB, M [20, n] MFCCs) on the device; ``power`` is the |STFT|^2 of the track."""
    tuning = _sig.estimate_tuning(audio, sr, bins_per_octave=36)
    cqt = _sig.cqt_magnitude(audio, sr, fmin=_sig.CQT_FMIN * 2.0 ** (tuning / 36))
    ref = max(float(cqt.max()), 1e-5)
    c = 20.0 * th.log10(th.clamp(cqt, min=1e-5)) - 20.0 * math.log10(ref)
    c = th.maximum(c, c.max() - 80.0)
    db = _sig.project(_sig.mel_filterbank(sr, N_FFT, 128), power, to_db=True)
    db = th.maximum(db, db.max() - 80.0)
    return c, _sig.project(dct_matrix(20, 128), db.contiguous())


def laplacian_segmentation(signal, sr, k=5, plot=False):
    """Section start times and one cluster label per section of a track (Laplacian structural segmentation, McFee & Ellis 2014,
    as the reference runs it with librosa 0.8).  ``signal``: mono float audio, numpy or torch on any device.  Returns
    (times, labels): Python floats (seconds, times[0] == 0, the last one the end of the track) and ints, len(times) ==
    len(labels) + 1.

    Deliberate differences from the reference:
      * labels are renumbered in order of first appearance (the first section is 0) and k-means is seeded, so a track gives the
        same answer on every run (the reference's unseeded sklearn KMeans numbers the clusters at random);
      * a boundary at the last beat-synchronous column, which has no beat frame, is dropped with its label (the reference raises
        IndexError);
      * times use the caller's ``sr`` (the reference's frames_to_time assumes 22050 Hz, the rate of everything load_audio returns);
      * k < 1, sr <= 0 and fewer than max(k, 7) beat-synchronous columns (silence, a clip of a few beats) raise ValueError.
    ``plot=True`` draws the constant-Q dB spectrogram with the sections shaded (workspace/laplacian_segmentation.png without a display).
    """
    check_arguments(sr, k)
    k = int(k)
    audio = signal.detach().float().reshape(-1) if isinstance(signal, th.Tensor) else np.ascontiguousarray(signal, dtype=np.float32).reshape(-1)
    env, power = onset_envelope(audio, sr)
    _, beats = beat_track(env, sr)
    c, mfcc = features(audio, sr, power)
    n_frames = c.shape[1]
    bounds = sync_bounds(beats, n_frames)
    check_columns(len(bounds) - 1, k)
    csync = beat_sync(c, bounds, median=True)
    msync = beat_sync(mfcc, bounds, median=False)
    links = knn_links(csync, knn_count(csync.shape[1]))
    _, rf = rec_affinity(links, link_bandwidth(links))
    x = spectral_embedding(rf, msync, k).cpu().numpy()
    times, labels = segment_boundaries(kmeans(x, k), beats, n_frames, sr)
    if plot:
        _plot(c, sr, times, labels, k)
    return times, labels


def _plot(c, sr, times, labels, k):
    from . import util

    plt = util._pyplot()
    if plt is None:
        return None
    fig, ax = plt.subplots(figsize=(16, 6))
    c = c.cpu().numpy()
    ax.imshow(c, origin="lower", aspect="auto", extent=(0.0, c.shape[1] * HOP / sr, 0, c.shape[0]), cmap="magma")
    colors = plt.get_cmap("Paired", k)
    for (start, stop), label in zip(zip(times, times[1:]), labels):
        ax.axvspan(start, stop, color=colors(label), alpha=0.5)
    ax.set_xlabel("time (s)")
    ax.set_ylabel("constant-Q bin (36 per octave from C1)")
    return util._finish(plt, "laplacian_segmentation")
