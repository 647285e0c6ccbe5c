"""Host: the inputs, references and comparisons of tests/test_segment_entries_gpu.py, checked on the CPU.

Every input of that module is built here and every precondition it states is asserted (a bad seed fails here, not on the GPU machine):
the gaps of the dynamic programme, both ends of its candidate window reached, the leading -1 backlinks, the integer exactness of the
neighbour search's squares, one-way and zero-distance links, the NaN spans.  Then a numpy stand-in of each kernel's arithmetic is put
through the very comparison the GPU test applies: the stand-in passes every case, and the same stand-in with one deliberate defect
fails at least one, so the comparisons are neither unsatisfiable nor slack.

One listed defect cannot be caught by construction, and the test says so instead of pretending: a dynamic programme that keeps the LAST
maximum differs from np.argmax's first maximum only on an exact tie of the two best candidates, and the inputs are required to keep
those >= 1e-8 apart on every frame.  test_beat_dp_last_maximum_is_indistinguishable_without_ties asserts exactly that."""
import numpy as np
import pytest
import scipy.signal

import segment_ref as ref
import test_segment_entries_gpu as se

F32, F64 = np.float32, np.float64


def fails(check, *args):
    try:
        check(*args)
    except AssertionError:
        return True
    return False


# ---------------------------------------------------------------------------------------------------------- tempogram
def tempogram_standin(env, win, hann="periodic", ramp=0):
    """The kernel's arithmetic: float32 envelope, fp64 ramp padding / window / direct autocorrelation, max-normalised unless below
    FLT_MIN, mean over frames, rounded to float32.  Defects: ``hann="symmetric"``; ``ramp=1`` (the right ramp one step late)."""
    e = env.astype(F32).astype(F64)
    n, pad = e.size, win // 2
    p = np.arange(n + 2 * pad + 1)  # (one spare sample: an odd window's last frame ends at n + 2 pad)
    k = p - pad
    padded = np.where(k < 0, p * (e[0] / pad), np.where(k >= n, (pad - 1 - (k - n) + ramp) * (e[-1] / pad), e[np.clip(k, 0, n - 1)]))
    window = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(win) / (win if hann == "periodic" else max(win - 1, 1)))
    total = np.zeros(win)
    for t in range(n):
        f = padded[t: t + win] * window
        ac = np.correlate(f, f, mode="full")[win - 1:]
        peak = np.abs(ac).max()
        total += ac / (1.0 if peak < se.TINY32 else peak)
    return (total / n).astype(F32)


def test_tempogram_runs_reach_the_stated_branches():
    runs = se.TEMPOGRAM_RUNS
    assert {(n, w) for n, w, _ in runs if _ != "tiny"} == set(se.TEMPOGRAM_CASES) and runs[-1] == (40, 64, "tiny")
    silent = [r for r in runs if r[2] == "lead0" and (se.tempogram_frame_energy(se.tempogram_env(r), r[1]) == 0).any()]
    assert silent, "no lead0 run has an all-zero frame"
    for r in runs:
        energy = se.tempogram_frame_energy(se.tempogram_env(r), r[1])
        if r[2] == "uniform":
            assert (energy >= se.TINY32).all(), r  # tg[0] == 1 is asserted on every uniform run
        if r[2] == "tiny":
            assert (energy < se.TINY32).all() and (energy > 0).all()
    assert any(n > 512 for n, _, _ in runs)  # the grid-stride trip over the 512 blocks


@pytest.mark.parametrize("run", se.TEMPOGRAM_RUNS, ids=se._ids)
def test_tempogram_standin_passes(run):
    se.check_tempogram(run, tempogram_standin(se.tempogram_env(run), run[1]))


@pytest.mark.parametrize("defect", [dict(hann="symmetric"), dict(ramp=1)], ids=["symmetric-hann", "late-ramp"])
def test_tempogram_defects_are_caught(defect):
    small = [r for r in se.TEMPOGRAM_RUNS if r[0] * r[1] * r[1] <= 3e7]
    caught = [r for r in small if fails(se.check_tempogram, r, tempogram_standin(se.tempogram_env(r), r[1], **defect))]
    print(f"tempogram {defect}: caught on {len(caught)} of {len(small)} runs")
    assert caught


# ---------------------------------------------------------------------------------------------------------- beat tracking
def localscore_standin(x, period, clip_at_n=False):
    """The kernel's clipped tap range per frame.  Defect ``clip_at_n``: the upper clip one frame late (reads x[n]; here a 1.0 beyond)."""
    n = x.size
    xp = np.concatenate([x, [1.0]])
    taps = np.exp(-0.5 * ((np.arange(2 * period + 1) - period) * 32.0 / period) ** 2)
    ls = np.zeros(n)
    last = n if clip_at_n else n - 1
    for i in range(n):
        lo = period - i if i - period < 0 else 0
        hi = period + (last - i) if i + period > last else 2 * period
        ls[i] = np.dot(xp[i - period + lo: i - period + hi + 1], taps[lo: hi + 1])
    return ls


def dp_standin(ls, period, half_up=False, short=False, last_max=False, sticky=False):
    """The kernel's dynamic programme.  Defects: ``half_up`` rounding of period / 2, ``short`` window from -2 period + 1, ``last_max``
    on ties, ``sticky``: the `first` flag never cleared."""
    n = ls.size
    w0 = -2 * period + (1 if short else 0)
    r = int(np.floor(period / 2 + 0.5)) if half_up else int(np.rint(period / 2))
    offsets = np.arange(w0, -r + 1)
    weight = -100.0 * np.log(-offsets / period) ** 2
    thr = 0.01 * ls.max()
    cum, back, first = np.zeros(n), np.zeros(n, np.int32), True
    for i in range(n):
        prev = i + offsets
        score = np.where(prev >= 0, weight + cum[np.maximum(prev, 0)], weight)
        best = score.size - 1 - int(np.argmax(score[::-1])) if last_max else int(np.argmax(score))
        cum[i] = ls[i] + score[best]
        none = first and ls[i] < thr
        back[i] = -1 if none else prev[best]
        first = first if sticky else none
    return cum, back


def beat_standin(run, clip_at_n=False, **dp):
    ls = localscore_standin(se.beat_onset(run), run[1], clip_at_n)
    return (ls,) + dp_standin(ls, run[1], **dp)


def test_localscore_has_n_values_and_is_scipys_same():
    rng = np.random.default_rng(0)
    for n, p in [(1, 2), (2, 2), (4, 2), (5, 2), (3, 7), (41, 21), (42, 21), (43, 21), (300, 344), (100, 20)]:
        x = rng.random(n)
        taps = np.exp(-0.5 * (np.arange(-p, p + 1) * 32.0 / p) ** 2)
        want = scipy.signal.convolve(x, taps, "same", method="direct")
        got = ref.localscore(x, p, normalise=False)
        assert got.shape == want.shape == (n,), (n, p)
        np.testing.assert_allclose(got, want, rtol=1e-13, atol=1e-15)
    x = rng.random(50)  # the normalising form is the same thing on x / std
    np.testing.assert_allclose(ref.localscore(x, 4), ref.localscore(x / x.std(ddof=1), 4, normalise=False), rtol=1e-14)


def test_beat_runs_cover_the_issue():
    assert {(n, p) for n, p, k in se.BEAT_RUNS if k == "uniform"} == set(se.BEAT_CASES)
    assert [p for _, p, k in se.BEAT_RUNS if k == "spikes"] == [2, 3, 5, 7, 21, 86]
    assert [se.round_half_even(p / 2) for p in (2, 3, 5, 7, 21, 86)] == [1, 2, 2, 4, 10, 43]  # 5 and 21 differ from half-up (3, 11)
    assert any(n < 2 * p + 1 for n, p, _ in se.BEAT_RUNS) and any(n > 256 for n, _, _ in se.BEAT_RUNS)
    w = 2 * 2000 - 1000 + 1
    assert w == 3001 <= 3072 and 2 * 2000 < 4096 < 4500  # the txwt slots; the ring wraps with predecessors 4000 frames back


@pytest.mark.parametrize("run", se.BEAT_RUNS, ids=se._ids)
def test_beat_preconditions_and_standin(run):
    se.beat_preconditions(run)
    gap, thr_gap = se.beat_want(run)[3:]
    print(f"beat {run}: top-two gap {gap:.3e}, threshold gap {thr_gap:.3e}")
    se.check_beat(run, *beat_standin(run))


BEAT_DEFECTS = {"clip-at-n": dict(clip_at_n=True), "half-up": dict(half_up=True), "short-window": dict(short=True),
                "first-never-cleared": dict(sticky=True)}


@pytest.mark.parametrize("name", BEAT_DEFECTS)
def test_beat_defects_are_caught(name):
    small = [r for r in se.BEAT_RUNS if r[0] <= 1200]
    caught = [r for r in small if fails(se.check_beat, r, *beat_standin(r, **BEAT_DEFECTS[name]))]
    print(f"beat {name}: caught on {len(caught)} of {len(small)} runs: {caught[:6]}")
    assert caught
    if name == "half-up":
        assert {r[1] for r in caught} >= {5, 21}


def test_beat_dp_last_maximum_is_indistinguishable_without_ties():
    """Keeping the last maximum changes a backlink only where the two best candidates tie exactly; the inputs keep them >= 1e-8 apart
    on every frame, so this defect passes every run (and only a tied input, which the unambiguity condition rules out, could show it)."""
    for run in [r for r in se.BEAT_RUNS if r[0] <= 1200]:
        assert se.beat_want(run)[3] >= se.MIN_GAP
        se.check_beat(run, *beat_standin(run, last_max=True))

# ---------------------------------------------------------------------------------------------------------- beat sync
def sync_standin(x, bounds, median, upper_only=False, unclamped=False):
    """The kernel's spans and ranks.  Defects: ``upper_only``, the rank L / 2 element alone for an even span; ``unclamped`` bounds
    (reads outside the row see zeros here)."""
    rows, n = x.shape
    bounds = np.asarray(bounds, np.int64)
    pad = int(np.abs(bounds).max()) + n
    xp = np.concatenate([np.zeros((rows, pad), F32), x, np.zeros((rows, pad), F32)], axis=1)
    out = np.zeros((rows, len(bounds) - 1), F32)
    for s in range(len(bounds) - 1):
        if unclamped:
            b0, b1 = int(bounds[s]), int(bounds[s + 1])
        else:
            b0 = min(max(0, int(bounds[: s + 1].max())), n)
            b1 = max(b0, min(int(bounds[s + 1]), n))
        L = b1 - b0
        if L <= 0:
            out[:, s] = np.nan
            continue
        span = xp[:, pad + b0: pad + b1]
        if median:
            srt = np.sort(span, axis=1)
            hi = srt[:, L // 2]
            with np.errstate(invalid="ignore"):
                out[:, s] = hi if (L & 1 or upper_only) else (srt[:, L // 2 - 1] + hi) * F32(0.5)
        else:
            with np.errstate(invalid="ignore"):
                out[:, s] = (span.astype(F64).sum(axis=1) / L).astype(F32)
    return out


def test_sync_tables_follow_the_header():
    assert np.diff(se.SYNC_BOUNDS).tolist() == se.SYNC_SPANS and se.SYNC_BOUNDS[-1] <= se.SYNC_FRAMES
    b = ref.clamp_bounds(se.SYNC_CLAMP_BOUNDS, se.SYNC_FRAMES)
    assert list(zip(b[:-1].tolist(), b[1:].tolist())) == se.SYNC_CLAMP_SPANS  # the restatement against the hand-written table
    x = se.sync_data(3)
    for median in (0, 1):
        want = ref.beat_sync_ref(x, se.SYNC_CLAMP_BOUNDS, median)
        assert np.isnan(want).all(axis=0).tolist() == [True, False, True, True, False, False, True, True]
        for rows in se.SYNC_ROWS:  # the span after the lowered bound tells [10, 4990) from [7, 4990) in every row
            xc, bc = se.sync_run(rows, "clamp")
            assert (ref.beat_sync_ref(xc, bc, median)[:, 4] != ref.beat_sync_ref(xc, [7, 4990], median)[:, 0]).all()
        assert np.isfinite(ref.beat_sync_ref(x, se.SYNC_BOUNDS, median)).all()
    xi = se.sync_data(3, inf=True)
    med, mean = ref.beat_sync_ref(xi, se.SYNC_BOUNDS, 1), ref.beat_sync_ref(xi, se.SYNC_BOUNDS, 0)
    assert (med[:, 2] == np.inf).all() and np.isfinite(med[:, [6, 8]]).all()
    assert (mean[:, [2, 6]] == np.inf).all() and (mean[:, 8] == -np.inf).all()
    # the reference's float32 median is numpy's
    for a, c in zip(se.SYNC_BOUNDS[:-1], se.SYNC_BOUNDS[1:]):
        assert np.array_equal(ref.beat_sync_ref(x, [a, c], 1)[:, 0], np.median(x[:, a:c], axis=1))
    # signed zeros sit on the middle ranks of the 64- and 65-frame spans, the equal run on those of the 128-frame span
    for span in (4, 5, 7):
        srt = np.sort(x[:, se.SYNC_BOUNDS[span]: se.SYNC_BOUNDS[span + 1]], axis=1)
        L = se.SYNC_SPANS[span]
        assert (srt[:, L // 2 - 1] == srt[:, L // 2]).all() and (srt[:, L // 2] == (F32(0.25) if span == 7 else 0)).all()


@pytest.mark.parametrize("median", [0, 1])
@pytest.mark.parametrize("rows", se.SYNC_ROWS)
def test_sync_standin_passes(rows, median):
    for kind in se.SYNC_KINDS:
        x, bounds = se.sync_run(rows, kind)
        se.check_sync(x, bounds, median, sync_standin(x, bounds, median))


def test_sync_defects_are_caught():
    x, bounds = se.sync_run(5, "spans")
    se.check_sync(x, bounds, 1, sync_standin(x, bounds, 1))
    assert fails(se.check_sync, x, bounds, 1, sync_standin(x, bounds, 1, upper_only=True))
    x, bounds = se.sync_run(5, "clamp")
    for median in (0, 1):
        assert fails(se.check_sync, x, bounds, median, sync_standin(x, bounds, median, unclamped=True))
    # a clamp of each span on its own (the span (7, 4990) kept as it is) is not the header's table clamp either
    per_span = sync_standin(x, np.array([-5, 0, 10, 10, 10, 4990, 5000, 5000, 5000]), 0)
    per_span[:, 4] = x[:, 7:4990].astype(F64).mean(axis=1).astype(F32)
    assert fails(se.check_sync, x, bounds, 0, per_span)


# ---------------------------------------------------------------------------------------------------------- knn links
def knn_standin(x, k, width, rows=None, ties_high=False, band_gt=False, no_cap=False):
    """The kernel's rule on the fp32 distances: outside the band |i - j| < width, the min(k, n_valid) smallest (distance, j).  Defects:
    ``ties_high`` (ties to the higher j), ``band_gt`` (columns with |i - j| > width only), ``no_cap`` (k not capped: band columns link)."""
    s = x.shape[1]
    rows = np.arange(s) if rows is None else np.asarray(rows)
    dist = ref.pair_distances_rows(x, rows)
    gap = np.abs(rows[:, None] - np.arange(s)[None, :])
    band = gap <= width if band_gt else gap < width
    key = np.where(band, F32(np.inf), dist)
    if ties_high:
        order = s - 1 - np.argsort(key[:, ::-1], axis=1, kind="stable")
    else:
        order = np.argsort(key, axis=1, kind="stable")
    n_valid = s - band.sum(axis=1)
    kk = np.full(len(rows), min(k, s)) if no_cap else np.minimum(k, n_valid)
    out = np.full((len(rows), s), F32(-1))
    for a in range(len(rows)):
        out[a, order[a, : kk[a]]] = dist[a, order[a, : kk[a]]]
    return out


def test_knn_features_make_the_order_exact():
    for case in se.KNN_CASES + [se.KNN_LIMIT]:
        d, s, k, width = case
        x = se.knn_features(case)
        assert x.shape == (d, s) and set(np.unique(x)) <= {0.0, 1.0, 2.0, 3.0} and 9 * d < 2 ** 24
        rows = np.arange(s) if s <= 600 else np.array(se.KNN_LIMIT_ROWS) % s
        exact = ((x.astype(np.int64)[:, rows, None] - x.astype(np.int64)[:, None, :]) ** 2).sum(axis=0)
        got = ref.pair_distances_rows(x, rows)
        assert np.array_equal(got, np.sqrt(exact.astype(F64)).astype(F32))  # fp32 sums exact; the root correctly rounded
        if s >= 7 and case not in se.KNN_ALL_OFF:
            key = np.where(np.abs(rows[:, None] - np.arange(s)) < width, -1, exact)
            assert any(len(np.unique(r[r >= 0])) < (r >= 0).sum() for r in key), case  # exact ties are present
    assert all((ref.knn_links_exact(se.knn_features(c), c[2], c[3]) == -1).all() for c in se.KNN_ALL_OFF)
    assert set(se.KNN_ALL_OFF) <= set(se.KNN_CASES)


def test_knn_exact_reference_equals_the_row_by_row_restatement():
    for case in [(3, 7, 2, 3), (3, 7, 16, 3), (2, 5, 3, 1), (20, 64, 14, 3), (5, 600, 599, 1)]:
        x = se.knn_features(case)
        dist = ref.pair_distances(x)
        sets = ref.knn_sets(dist, case[2], case[3])
        links = ref.knn_links_exact(x, case[2], case[3], block=37)
        for i, want in enumerate(sets):
            assert set(np.flatnonzero(links[i] >= 0).tolist()) == want
        assert np.array_equal(links[links >= 0], dist[links >= 0])
        rows = np.array([0, 3, case[1] - 1])
        assert np.array_equal(ref.knn_links_exact(x, case[2], case[3], rows=rows), links[rows])


@pytest.mark.parametrize("case", se.KNN_CASES, ids=se._ids)
def test_knn_standin_passes(case):
    x = se.knn_features(case)
    se.check_knn(case, x, knn_standin(x, case[2], case[3]))


def test_knn_standin_passes_the_limit_rows_and_gaussian_features():
    x = se.knn_features(se.KNN_LIMIT)
    rows = np.array(se.KNN_LIMIT_ROWS)
    links = np.full((x.shape[1], x.shape[1]), F32(-1))
    links[rows] = knn_standin(x, se.KNN_LIMIT[2], se.KNN_LIMIT[3], rows=rows)
    se.check_knn(se.KNN_LIMIT, x, links, rows=rows)
    xg = se.knn_gauss_features()
    se.check_knn_gauss(xg, knn_standin(xg, ref.knn_k(xg.shape[1]), 3))


@pytest.mark.parametrize("defect", ["ties_high", "band_gt", "no_cap"])
def test_knn_defects_are_caught(defect):
    small = [c for c in se.KNN_CASES if c[1] <= 600]
    caught = [c for c in small if fails(se.check_knn, c, se.knn_features(c), knn_standin(se.knn_features(c), c[2], c[3], **{defect: True}))]
    print(f"knn {defect}: caught on {len(caught)} of {len(small)} cases: {caught}")
    assert caught


# ---------------------------------------------------------------------------------------------------------- affinity + time-lag median
def affinity_standin(links, bandwidth, one_way=False, mirror=False):
    """The kernel's arithmetic: float32 exp(d / -bw) on mutual links, then the rank-3 element of the seven reflected diagonal
    neighbours.  Defects: ``one_way`` (a >= 0 alone), ``mirror`` (d c b | a b c d reflection, scipy's 'mirror')."""
    s = links.shape[0]
    on = (links >= 0) if one_way else (links >= 0) & (links.T >= 0)
    rec = np.where(on, se.rec_f32(links, bandwidth), F32(0)).astype(F32)
    i, j = np.meshgrid(np.arange(s), np.arange(s), indexing="ij")
    vals = []
    for sh in range(-3, 4):
        jp = j + sh
        if mirror:
            jp = np.where(jp < 0, -jp, np.where(jp >= s, 2 * s - jp - 2, jp))
        else:
            jp = np.where(jp < 0, -jp - 1, np.where(jp >= s, 2 * s - jp - 1, jp))
        row = i - j + jp
        ok = (row >= 0) & (row < s)
        vals.append(np.where(ok, rec[np.clip(row, 0, s - 1), jp], F32(0)))
    return rec, np.sort(np.stack(vals), axis=0)[3].astype(F32)


def test_affinity_links_hold_what_the_issue_asks():
    for s in se.AFF_SIZES:
        links = se.aff_links(s)
        on = links >= 0
        assert links.shape == (s, s) and not on.diagonal().any() and links[on].max() < 4
        assert (on & on.T).sum() >= 6 and (on & ~on.T).sum() >= 1, s  # mutual and one-way links
        assert on[1, 3] and not on[3, 1]
        assert np.array_equal(links[on & on.T], links.T[on & on.T])
        for i, j in se.aff_zero_pairs(s):
            assert links[i, j] == 0 and links[j, i] == 0
        if s > 7:
            frac = on.sum() / (s * s - s)
            assert 0.2 < frac < 0.4


@pytest.mark.parametrize("bandwidth", se.AFF_BANDWIDTHS)
@pytest.mark.parametrize("s", se.AFF_SIZES)
def test_affinity_standin_passes(s, bandwidth):
    links = se.aff_links(s)
    se.check_affinity(links, bandwidth, *affinity_standin(links, bandwidth))


@pytest.mark.parametrize("defect", ["one_way", "mirror"])
def test_affinity_defects_are_caught(defect):
    caught = [s for s in se.AFF_SIZES if s <= 33
              if fails(se.check_affinity, se.aff_links(s), 1.5, *affinity_standin(se.aff_links(s), 1.5, **{defect: True}))]
    print(f"affinity {defect}: caught at S = {caught}")
    assert caught
    if defect == "mirror":
        assert 4 in caught  # at S = 4 the reflection reaches 3 past each end
