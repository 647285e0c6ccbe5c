"""GPU: every C entry of csrc/segment.hip called directly through the C ABI, at the shapes and edges its kernels have separate code for,
between red zones, against a plain reference of the same operation (tests/segment_ref.py).

Each call allocates all device operands through redzone.Guard (the tempogram workspace sized exactly by maua_tempogram_ws_doubles), runs
twice into separate output windows (identical bits required) and ends with Guard.check: red zones intact, every output element written,
every output finite unless the case feeds non-finite input or asks for an empty span (whose result is NaN by the header).

Selections are compared bit for bit with no element exempt: the backlinks of the dynamic programme, the float32 medians, the whole link
matrix of the neighbour search (integer features: every squared distance is an exact integer below 2^24, so the order, the ties and the
square root are all determined), the time-lag median (a pure selection from the kernel's own `rec`).  Where a selection could hinge on
rounding the INPUT is built so that it does not, and that is checked on the CPU before the kernel runs (tests/
test_segment_entries_refs_host.py checks the same without a GPU): the best and second-best candidate of every frame of the dynamic
programme differ by >= 1e-8, and so does every local score from the 0.01 max threshold while no beat has been found.

Tolerances of the floating-point results are NOT taken from the kernels.  The figure is measured on the CPU over the case lists of this
module (`PYTHONPATH=. python tests/test_segment_entries_gpu.py` prints them without a GPU; the constants below are those rounded up to
two digits) and the tolerance is 4 x the figure:

    entry            scale      figure                                                              measured   tolerance (x4)
    tempogram        peak       float64 reference vs the same with input and output rounded to fp32  4.1e-08    1.7e-07
    tempogram_tiny   peak       the same, on the 1e-20 envelope (fp32 results are subnormal: ~1e-39)  9.3e-07    3.7e-06
    rec              absolute   float64 exp(-d / bw) vs an all-float32 evaluation (rec <= 1)          1.3e-07    5.2e-07

The kernels' internals are fp64 for the tempogram (only its input and output are fp32) and fp64 end to end for the beat tracker, whose
local and cumulative scores keep the project's rtol = atol = 1e-9 of test_segmentation_gpu.py.  The mean of beat_sync is the float64 mean
rounded to float32, within one float32 ulp.

Beat-sync bounds are clamped as a table (header: inside [0, n_frames], none below an earlier one); SYNC_CLAMP_SPANS is written out from
that text, not computed."""
import functools

import numpy as np
import pytest
import torch
from numpy.lib.stride_tricks import sliding_window_view

import segment_ref as ref
from test_signal_entries_gpu import EINVAL, F32, F64, Out, _refused, _rel_peak, _rng, _run, _same_bits

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

TINY32 = float(np.finfo(F32).tiny)

# measured figure per entry (see the module docstring); the tolerance is 4 x this
MEASURED = {
    "tempogram": 4.1e-08,
    "tempogram_tiny": 9.3e-07,
    "rec": 1.3e-07,
}
TOL = {k: 4.0 * v for k, v in MEASURED.items()}
BEAT_RTOL = BEAT_ATOL = 1e-9  # fp64 end to end: the bound of test_segmentation_gpu.py
MIN_GAP = 1e-8  # the dynamic programme's decisions are at least this far from a tie


def _ids(c):
    return "-".join(str(v) for v in c)


# ---------------------------------------------------------------------------------------------------------- tempogram
TEMPOGRAM_CASES = [(1, 2), (1, 3), (2, 2), (5, 255), (3, 256), (300, 257), (130, 344), (200, 511), (513, 512), (64, 513), (1, 1023),
                   (2, 1024), (600, 1024), (513, 2), (1100, 33)]  # (n_frames, win)
TEMPOGRAM_TINY_CASE = (40, 64)
TEMPOGRAM_RUNS = [(n, w, kind) for n, w in TEMPOGRAM_CASES for kind in ("uniform", "lead0") if kind == "uniform" or n >= 3] + \
    [TEMPOGRAM_TINY_CASE + ("tiny",)]


def tempogram_env(run):
    """The float64 envelope of a run; the entry receives it rounded to float32."""
    n, win, kind = run
    env = _rng(20, n, win).random(n)
    if kind == "lead0":
        env[: n // 3] = 0.0
    if kind == "tiny":
        env *= 1e-20
    return env


def tempogram_frame_energy(env, win):
    """Lag-0 autocorrelation (the largest |.|) of every windowed frame of the float32 envelope: the quantity the FLT_MIN test looks at."""
    padded = np.pad(env.astype(F32).astype(F64), win // 2, mode="linear_ramp", end_values=0)
    window = 0.5 - 0.5 * np.cos(2.0 * np.pi * np.arange(win) / win)
    return ((sliding_window_view(padded, win)[: env.size] * window) ** 2).sum(axis=1)


@functools.lru_cache(maxsize=None)
def tempogram_want(run):
    want = ref.tempogram_mean(tempogram_env(run), run[1])
    want.setflags(write=False)
    return want


def check_tempogram(run, tg):
    n, win, kind = run
    want = tempogram_want(run)
    assert tg.shape == (win,) and tg.dtype == F32
    err = _rel_peak(tg, want)
    print(f"tempogram {run}: err/peak {err:.3e}")
    assert err <= TOL["tempogram_tiny" if kind == "tiny" else "tempogram"], (run, err)
    energy = tempogram_frame_energy(tempogram_env(run), win)
    if kind == "tiny":
        assert (energy < TINY32).all() and (energy > 0).all()  # every frame takes the un-normalised branch
    elif (energy >= TINY32).all():
        assert tg[0] == F32(1.0), (run, tg[0])  # every frame is divided by its own lag-0 value


def _gpu_tempogram(gpu, env, win):
    from maua_stylegan2_amd import _lib

    n = env.size
    ws = int(_lib.load().maua_tempogram_ws_doubles(n, win))
    assert ws == min(n, 512) * win
    return _run(gpu, "maua_tempogram_f32", [("env", env.astype(F32)), ("n_frames", n), ("win", win), ("ws", Out((ws,), torch.float64)),
                                            ("tg", Out((win,)))])["tg"]


@pytest.mark.parametrize("run", TEMPOGRAM_RUNS, ids=_ids)
def test_tempogram_vs_reference(gpu, run):
    check_tempogram(run, _gpu_tempogram(gpu, tempogram_env(run), run[1]))


# ---------------------------------------------------------------------------------------------------------- beat tracking
BEAT_CASES = [(1, 2), (2, 2), (5, 2), (70, 3), (200, 5), (130, 7), (63, 21), (64, 21), (65, 21), (300, 344), (4500, 2000), (5000, 1999),
              (9000, 86)]  # (n_frames, period)
BEAT_SPIKE_PERIODS = [2, 3, 5, 7, 21, 86]
BEAT_ZERO_CASE = (70, 3)
BEAT_RUNS = [(n, p, kind) for n, p in BEAT_CASES for kind in ("uniform", "lead0") if kind == "uniform" or n >= 3] + \
    [(12 * p + 7, p, "spikes") for p in BEAT_SPIKE_PERIODS] + [BEAT_ZERO_CASE + ("zero",)]


def round_half_even(v):
    return int(np.round(v))


def beat_spike_frames(p):
    a, r = p + 1, round_half_even(p / 2)
    return [a, a + 2 * p, a + 2 * p + r, a + 4 * p + r, a + 4 * p + 2 * r]


def beat_onset(run):
    """The float64 onset envelope the entry receives (already normalised where the run normalises)."""
    n, p, kind = run
    r = _rng(21, n, p)
    if kind == "zero":
        return np.zeros(n)
    u = r.random(n)
    if kind == "spikes":  # a valley everywhere but five spikes 2p, r, 2p, r apart: the best predecessor is the spike before
        x = -200.0 * (1.0 + u)
        sp = beat_spike_frames(p)
        x[sp] = 1000.0 * (1.0 + u[sp])
        return x
    if kind == "lead0":
        u[: n // 3] = 0.0
    return u / u.std(ddof=1) if n > 1 else u


@functools.lru_cache(maxsize=None)
def beat_want(run):
    """(localscore, cumscore, backlink, min_gap, min_threshold_gap) of the float64 restatement."""
    ls = ref.localscore(beat_onset(run), run[1], normalise=False)
    out = (ls,) + ref.beat_dp_margins(ls, run[1])
    for a in out[:3]:
        a.setflags(write=False)
    return out


def beat_preconditions(run):
    """Conditions on the INPUT, checked on the reference before any kernel runs."""
    n, p, kind = run
    ls, cum, back, gap, thr_gap = beat_want(run)
    assert ls.shape == cum.shape == back.shape == (n,)
    assert gap >= MIN_GAP and thr_gap >= MIN_GAP, (run, gap, thr_gap)
    lead = int(np.flatnonzero(ls >= 0.01 * ls.max())[0])  # frames before the first beat (a later -1 is the predecessor "frame -1")
    assert (back[:lead] == -1).all()
    if kind == "lead0" and n >= 5:
        assert lead > 0, run  # a silent lead-in: no backlink before the first beat
    if kind == "spikes":
        chosen = (back - np.arange(n))[lead:]
        assert chosen.min() == -2 * p and chosen.max() == -round_half_even(p / 2), (run, chosen.min(), chosen.max())
    if kind == "zero":
        assert (ls == 0).all() and (cum == 0).all() and np.array_equal(back, np.arange(n) - p)


def check_beat(run, ls, cum, back):
    want_ls, want_cum, want_back = beat_want(run)[:3]
    if run[2] == "zero":
        assert (ls == 0).all() and (cum == 0).all()
    np.testing.assert_allclose(ls, want_ls, rtol=BEAT_RTOL, atol=BEAT_ATOL)
    np.testing.assert_allclose(cum, want_cum, rtol=BEAT_RTOL, atol=BEAT_ATOL)
    wrong = np.flatnonzero(np.asarray(back, np.int64) != want_back)
    assert wrong.size == 0, (run, wrong[:8], np.asarray(back)[wrong[:8]], want_back[wrong[:8]])


def _gpu_beat(gpu, x, period):
    n = x.size
    o = _run(gpu, "maua_beat_track_f64", [("onset", np.ascontiguousarray(x, F64)), ("n_frames", n), ("period", period),
                                          ("localscore", Out((n,), torch.float64)), ("cumscore", Out((n,), torch.float64)),
                                          ("backlink", Out((n,), torch.int32))])
    return o["localscore"], o["cumscore"], o["backlink"]


@pytest.mark.parametrize("run", BEAT_RUNS, ids=_ids)
def test_beat_track_vs_reference(gpu, run):
    beat_preconditions(run)
    check_beat(run, *_gpu_beat(gpu, beat_onset(run), run[1]))


# ---------------------------------------------------------------------------------------------------------- beat sync
SYNC_ROWS = [1, 3, 4, 5, 21]
SYNC_FRAMES = 5000
SYNC_SPANS = [1, 2, 3, 63, 64, 65, 127, 128, 129, 257, 4096]
SYNC_BOUNDS = np.concatenate([[0], np.cumsum(SYNC_SPANS)]).astype(np.int32)
SYNC_CLAMP_BOUNDS = np.array([-5, 0, 10, 10, 7, 4990, 5000, 5003, 6000], np.int32)
# the header's clamp, by hand: -5 -> 0; 7 is below the 10 before it -> 10; 5003 and 6000 -> 5000
SYNC_CLAMP_SPANS = [(0, 0), (0, 10), (10, 10), (10, 10), (10, 4990), (4990, 5000), (5000, 5000), (5000, 5000)]
SYNC_KINDS = ["spans", "spans-inf", "clamp"]


def sync_data(rows, inf=False, plain=False):
    """Random float32 rows (``plain``: nothing else) with, per row: a run of equal values that holds the median of the 128-frame span, signed zeros around the
    middle rank of the 64- and 65-frame spans (shuffled), and for ``inf`` two +inf in the 3-frame span, one +inf in the 127-frame span
    and one -inf in the 129-frame one."""
    r = _rng(22, rows)
    x = r.standard_normal((rows, SYNC_FRAMES)).astype(F32)
    if plain:
        return x
    b = SYNC_BOUNDS
    x[:, b[7] + 10: b[7] + 100] = F32(0.25)
    for span, (neg, zero) in ((4, (20, 24)), (5, (20, 25))):
        L = SYNC_SPANS[span]
        for row in range(rows):
            v = np.concatenate([-0.1 - r.random(neg), r.choice([0.0, -0.0], zero), 0.1 + r.random(L - neg - zero)]).astype(F32)
            x[row, b[span]: b[span + 1]] = r.permutation(v)
    if inf:
        x[:, b[2]: b[2] + 2] = np.inf
        x[:, b[6] + 77] = np.inf
        x[:, b[8] + 128] = -np.inf
    return x


def sync_run(rows, kind):
    if kind == "clamp":  # (plain rows: planted zeros would sit on the median of the long span however its start is clamped)
        return sync_data(rows, plain=True), SYNC_CLAMP_BOUNDS
    return sync_data(rows, inf=kind == "spans-inf"), SYNC_BOUNDS


def check_sync(x, bounds, median, got):
    want = ref.beat_sync_ref(x, bounds, median)
    assert got.shape == want.shape and got.dtype == F32
    assert np.array_equal(np.isnan(got), np.isnan(want)), "NaN exactly on the empty spans"
    ok = ~np.isnan(want)
    if median:
        assert _same_bits(got[ok], want[ok]), np.argwhere(ok & (got != want))[:8]
    else:
        fin = ok & np.isfinite(want)
        assert np.array_equal(got[ok & ~fin], want[ok & ~fin])
        with np.errstate(invalid="ignore"):
            ulps = np.abs(got[fin].astype(F64) - want[fin].astype(F64)) / np.spacing(np.abs(want[fin])).astype(F64)
        print(f"beat_sync mean rows={x.shape[0]}: worst {ulps.max() if ulps.size else 0:.2f} ulp")
        assert (ulps <= 1.0).all()


def _gpu_sync(gpu, x, bounds, median, nonfinite_ok):
    rows, n = x.shape
    n_spans = len(bounds) - 1
    return _run(gpu, "maua_beat_sync_f32", [("x", x), ("rows", rows), ("n_frames", n), ("bounds", np.asarray(bounds, np.int32)),
                                            ("n_spans", n_spans), ("median", median), ("out", Out((rows, n_spans)))],
                nonfinite_ok=nonfinite_ok)["out"]


@pytest.mark.parametrize("median", [0, 1])
@pytest.mark.parametrize("rows", SYNC_ROWS)
def test_beat_sync_vs_reference(gpu, rows, median):
    for kind in SYNC_KINDS:
        x, bounds = sync_run(rows, kind)
        got = _gpu_sync(gpu, x, bounds, median, nonfinite_ok=kind != "spans")  # (inf input; NaN of an empty span)
        check_sync(x, bounds, median, got)
        if kind == "clamp":
            empty = [a == b for a, b in SYNC_CLAMP_SPANS]
            assert np.array_equal(np.isnan(got), np.broadcast_to(empty, got.shape))
        if kind == "spans" and median:
            assert (got[:, 7] == F32(0.25)).all() and (got[:, 4] == 0).all() and (got[:, 5] == 0).all()


# ---------------------------------------------------------------------------------------------------------- knn links
KNN_CASES = [(1, 2, 1, 1), (2, 2, 4, 3), (3, 7, 2, 3), (3, 7, 16, 3), (2, 5, 3, 1), (20, 64, 14, 3), (20, 255, 30, 3), (20, 256, 30, 3),
             (20, 257, 30, 3), (1024, 40, 6, 3), (7, 513, 5, 100), (252, 1500, 78, 3), (5, 600, 599, 1), (2, 300, 4, 300)]  # (d, s, k, width)
KNN_ALL_OFF = [(2, 2, 4, 3), (2, 300, 4, 300)]  # the band covers every column: every output is -1
KNN_LIMIT = (2, 8192, 182, 3)
KNN_LIMIT_ROWS = [0, 1, 2, 3, 31, 32, 33, 4095, 4096, 8188, 8189, 8190, 8191]
KNN_GAUSS = (20, 301)


def knn_features(case):
    """Small integers as float32: every squared distance is an exact integer <= 9 d <= 9216 < 2^24."""
    d, s, _, _ = case
    return _rng(23, *case).integers(0, 4, size=(d, s)).astype(F32)


def check_knn(case, x, links, rows=None):
    d, s, k, width = case
    want = ref.knn_links_exact(x, k, width, rows=rows)
    got = links if rows is None else links[rows]
    assert got.shape == want.shape and links.dtype == F32
    bad = np.argwhere(got.view(np.int32) != want.view(np.int32))
    assert bad.size == 0, (case, bad[:8])
    if case in KNN_ALL_OFF:
        assert (got == -1).all()
    sq = got if rows is None else links[np.ix_(rows, rows)]
    both = (sq >= 0) & (sq.T >= 0)
    assert np.array_equal(sq.view(np.int32)[both], sq.T.view(np.int32)[both])  # d(i, j) and d(j, i) bit for bit


def _gpu_knn(gpu, x, k, width):
    d, s = x.shape
    return _run(gpu, "maua_knn_links_f32", [("x", x), ("d", d), ("s", s), ("k", k), ("width", width), ("links", Out((s, s)))])["links"]


@pytest.mark.parametrize("case", KNN_CASES, ids=_ids)
def test_knn_links_bit_for_bit(gpu, case):
    x = knn_features(case)
    check_knn(case, x, _gpu_knn(gpu, x, case[2], case[3]))


def test_knn_links_at_the_size_limit(gpu):
    x = knn_features(KNN_LIMIT)
    links = _gpu_knn(gpu, x, KNN_LIMIT[2], KNN_LIMIT[3])  # red zones, all written and two equal runs on the whole 8192 x 8192 output
    check_knn(KNN_LIMIT, x, links, rows=np.array(KNN_LIMIT_ROWS))


def knn_gauss_features():
    d, s = KNN_GAUSS
    return _rng(23, d, s).standard_normal((d, s)).astype(F32)


def check_knn_gauss(x, links, width=3):
    """Non-degenerate data: the link set of every row equals the restatement's, or differs only across a near-tie of the k-th distance."""
    s = x.shape[1]
    k = ref.knn_k(s, width)
    dist = ref.pair_distances(x)
    want = ref.knn_sets(dist, k, width)
    for i in range(s):
        got = set(np.flatnonzero(links[i] >= 0).tolist())
        assert len(got) == k
        if got != want[i]:
            row = sorted(dist[i, j] for j in range(s) if abs(i - j) >= width)
            assert abs(row[k] - row[k - 1]) <= 1e-5 * row[k], (i, got ^ want[i])
        np.testing.assert_allclose(links[i][sorted(got)], dist[i][sorted(got)], rtol=1e-6)
    both = (links >= 0) & (links.T >= 0)
    assert np.array_equal(links[both], links.T[both])


def test_knn_links_gaussian_features(gpu):
    x = knn_gauss_features()
    check_knn_gauss(x, _gpu_knn(gpu, x, ref.knn_k(x.shape[1]), 3))


# ---------------------------------------------------------------------------------------------------------- affinity + time-lag median
AFF_SIZES = [4, 5, 7, 31, 32, 33, 255, 256, 257]
AFF_BANDWIDTHS = [0.05, 1.5]
AFF_LITERAL_MAX = 64


def aff_links(s):
    """A host-built link matrix: distances in [0, 4) on a random 30 % of the off-diagonal cells, -1 elsewhere.  A cell and its transpose
    are chosen independently, so links are mutual or one-way by chance; a mutual pair shares one distance (as the neighbour search gives);
    and by construction (0, s-1) and (0, 2) are mutual at distance exactly 0, (1, 3) links one way only, and (0, 1), (1, 2), (2, 3) are
    mutual at three different distances: the first off-diagonal next to the corner is full, so that the medians there, which the
    reflection at the edge decides, are not all zero even at s = 4."""
    r = _rng(24, s)
    dist = (4.0 * r.random((s, s))).astype(F32)
    dist = np.triu(dist) + np.triu(dist, 1).T
    chosen = (r.random((s, s)) < 0.3) & ~np.eye(s, dtype=bool)
    links = np.where(chosen, dist, F32(-1)).astype(F32)
    for i, j, v, back in ((0, s - 1, 0.0, True), (0, 2, 0.0, True), (0, 1, 0.75, True), (1, 2, 0.5, True), (2, 3, 1.75, True),
                          (1, 3, 1.25, False)):
        links[i, j] = v
        links[j, i] = v if back else -1
    return links


def aff_zero_pairs(s):
    return [(0, s - 1), (s - 1, 0), (0, 2), (2, 0)]


def check_affinity(links, bandwidth, rec, rec_filt):
    s = links.shape[0]
    want = ref.affinity_from_links(links, F32(bandwidth))
    assert rec.shape == rec_filt.shape == (s, s) and rec.dtype == rec_filt.dtype == F32
    assert np.array_equal(rec == 0, want == 0), "zero exactly off the mutual links"
    err = float(np.abs(rec.astype(F64) - want).max())
    print(f"rec s={s} bw={bandwidth}: abs err {err:.3e}")
    assert err <= TOL["rec"], err
    for i, j in aff_zero_pairs(s):
        assert rec[i, j] == F32(1.0)
    sel = ref.timelag_median_formula(rec)  # a pure selection from the kernel's own rec
    bad = np.argwhere(rec_filt.view(np.int32) != sel.astype(F32).view(np.int32))
    assert bad.size == 0, bad[:8]
    if s <= AFF_LITERAL_MAX:
        assert np.abs(rec_filt.astype(F64) - ref.timelag_median_literal(want)).max() <= TOL["rec"]


def _gpu_affinity(gpu, links, bandwidth):
    s = links.shape[0]
    o = _run(gpu, "maua_rec_affinity_f32", [("links", links), ("s", s), ("bandwidth", float(bandwidth)), ("rec", Out((s, s))),
                                            ("rec_filt", Out((s, s)))])
    return o["rec"], o["rec_filt"]


@pytest.mark.parametrize("bandwidth", AFF_BANDWIDTHS)
@pytest.mark.parametrize("s", AFF_SIZES)
def test_rec_affinity_and_timelag_median(gpu, s, bandwidth):
    links = aff_links(s)
    check_affinity(links, bandwidth, *_gpu_affinity(gpu, links, bandwidth))


# ---------------------------------------------------------------------------------------------------------- refusals
def test_tempogram_refusals(gpu):
    n, win = 100, 344
    env = _rng(25).random(n).astype(F32)
    spec = [("env", env), ("n_frames", n), ("win", win), ("ws", Out((n * win,), torch.float64)), ("tg", Out((win,)))]
    _refused(gpu, "maua_tempogram_f32", spec,
             [({"win": v}, EINVAL) for v in (1, 0, -1, 1025)] + [({"n_frames": v}, EINVAL) for v in (0, -1)] +
             [({k: None}, EINVAL) for k in ("env", "ws", "tg")])


def test_beat_track_refusals(gpu):
    n = 100
    x = _rng(26).random(n)
    spec = [("onset", x), ("n_frames", n), ("period", 20), ("localscore", Out((n,), torch.float64)), ("cumscore", Out((n,), torch.float64)),
            ("backlink", Out((n,), torch.int32))]
    _refused(gpu, "maua_beat_track_f64", spec,
             [({"period": v}, EINVAL) for v in (1, 0, -3, 2001)] + [({"n_frames": v}, EINVAL) for v in (0, -1)] +
             [({k: None}, EINVAL) for k in ("onset", "localscore", "cumscore", "backlink")])


def test_beat_sync_refusals(gpu):
    x = sync_data(4)[:, :100].copy()
    bounds = np.array([0, 10, 50, 100], np.int32)
    spec = [("x", x), ("rows", 4), ("n_frames", 100), ("bounds", bounds), ("n_spans", 3), ("median", 1), ("out", Out((4, 3)))]
    _refused(gpu, "maua_beat_sync_f32", spec,
             [({"median": v}, EINVAL) for v in (2, -1)] + [({"n_spans": v}, EINVAL) for v in (0, -1)] + [({"rows": 0}, EINVAL),
              ({"n_frames": 0}, EINVAL)] + [({k: None}, EINVAL) for k in ("x", "bounds", "out")])


def test_knn_links_refusals(gpu):
    case = (20, 64, 4, 3)
    x = knn_features(case)
    spec = [("x", x), ("d", 20), ("s", 64), ("k", 4), ("width", 3), ("links", Out((64, 64)))]
    _refused(gpu, "maua_knn_links_f32", spec,
             [({"s": v}, EINVAL) for v in (1, 0, 8193)] + [({"d": v}, EINVAL) for v in (1025, 0)] + [({"k": v}, EINVAL) for v in (0, -1)] +
             [({"width": v}, EINVAL) for v in (0, -1)] + [({k: None}, EINVAL) for k in ("x", "links")])


def test_rec_affinity_refusals(gpu):
    links = aff_links(64)
    spec = [("links", links), ("s", 64), ("bandwidth", 1.0), ("rec", Out((64, 64))), ("rec_filt", Out((64, 64)))]
    _refused(gpu, "maua_rec_affinity_f32", spec,
             [({"s": v}, EINVAL) for v in (3, 0, 8193)] + [({"bandwidth": v}, EINVAL) for v in (0.0, -1.0, float("nan"), float("inf"))] +
             [({k: None}, EINVAL) for k in ("links", "rec", "rec_filt")])


# ---------------------------------------------------------------------------------------------------------- the tolerance table
def rec_f32(links, bandwidth):
    """exp(-d / bw) evaluated in float32 throughout (on every cell with a distance)."""
    d = np.where(links >= 0, links, F32(0)).astype(F32)
    return np.exp((d / -F32(bandwidth)).astype(F32)).astype(F32)


def measure():
    """The figures of the module docstring, on the CPU."""
    fig = {k: 0.0 for k in MEASURED}
    for run in TEMPOGRAM_RUNS:
        want = tempogram_want(run)
        lo = ref.tempogram_mean(tempogram_env(run).astype(F32), run[1]).astype(F32)
        key = "tempogram_tiny" if run[2] == "tiny" else "tempogram"
        fig[key] = max(fig[key], _rel_peak(lo, want))
    for s in AFF_SIZES:
        links = aff_links(s)
        for bw in AFF_BANDWIDTHS:
            d = np.where(links >= 0, links, 0).astype(F64)
            fig["rec"] = max(fig["rec"], float(np.abs(rec_f32(links, bw).astype(F64) - np.exp(-d / float(F32(bw)))).max()))
    return fig


if __name__ == "__main__":
    for name, v in measure().items():
        print(f"    {name:<16s} measured {v:.2e}   tolerance {4 * v:.2e}   (module constant {MEASURED[name]:.2e})")
    gaps = [beat_want(run)[3:] for run in BEAT_RUNS]
    print(f"    beat DP: smallest top-two gap {min(g for g, _ in gaps):.2e}, smallest threshold gap {min(t for _, t in gaps):.2e}")
