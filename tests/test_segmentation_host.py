"""CPU: the host side of laplacian_segmentation — argument checks of the new C entries, step 9's boundary assembly and the
ValueError cases, the time-lag median identity and the nearest-neighbour rule (no GPU needed)."""
import numpy as np
import pytest

import segment_ref as ref
from maua_stylegan2_amd.audioreactive import segment


def test_segment_entries_reject_bad_arguments_without_gpu(built_lib):
    from maua_stylegan2_amd import _lib

    lib = _lib.load()
    fake = 0x1000  # never dereferenced: rejected during validation
    assert lib.maua_tempogram_f32(None, 100, 344, fake, fake, None) == -22
    assert lib.maua_tempogram_f32(fake, 0, 344, fake, fake, None) == -22
    assert lib.maua_tempogram_f32(fake, 100, 1025, fake, fake, None) == -22
    assert lib.maua_tempogram_ws_doubles(100, 344) == 100 * 344 and lib.maua_tempogram_ws_doubles(10 ** 6, 344) == 512 * 344
    assert lib.maua_beat_track_f64(fake, 100, 1, fake, fake, fake, None) == -22
    assert lib.maua_beat_track_f64(fake, 100, 2001, fake, fake, fake, None) == -22
    assert lib.maua_beat_track_f64(fake, 0, 20, fake, fake, fake, None) == -22
    assert lib.maua_beat_sync_f32(fake, 4, 100, fake, 0, 1, fake, None) == -22
    assert lib.maua_beat_sync_f32(fake, 4, 100, fake, 3, 2, fake, None) == -22
    assert lib.maua_beat_sync_f32(None, 4, 100, fake, 3, 1, fake, None) == -22
    assert lib.maua_knn_links_f32(fake, 252, 8193, 4, 3, fake, None) == -22
    assert lib.maua_knn_links_f32(fake, 1025, 64, 4, 3, fake, None) == -22
    assert lib.maua_knn_links_f32(fake, 20, 64, 0, 3, fake, None) == -22
    assert lib.maua_knn_links_f32(fake, 20, 64, 4, 0, fake, None) == -22
    assert lib.maua_rec_affinity_f32(fake, 3, 1.0, fake, fake, None) == -22
    assert lib.maua_rec_affinity_f32(fake, 64, 0.0, fake, fake, None) == -22
    assert lib.maua_rec_affinity_f32(fake, 64, float("nan"), fake, fake, None) == -22
    assert lib.maua_rec_affinity_f32(fake, 64, float("inf"), fake, fake, None) == -22


def test_boundaries_relabel_in_order_of_first_appearance():
    beats = np.arange(10, 130, 10)  # 12 beats -> 13 sync columns
    seg = np.array([2, 2, 2, 0, 0, 0, 2, 2, 1, 1, 1, 1, 1])
    times, labels = segment.segment_boundaries(seg, beats, n_frames=200, sr=22050)
    assert labels == [0, 1, 0, 2]
    frames = [10, 40, 70, 90, 199]
    assert times == [0.0] + [f * 512 / 22050 for f in frames[1:]]
    assert len(times) == len(labels) + 1
    assert all(isinstance(t, float) for t in times) and all(type(v) is int for v in labels)


def test_boundary_at_the_last_sync_column_is_dropped():
    beats = np.array([5, 15, 25, 35, 45, 55, 65])  # 8 sync columns: column 7 has no beat frame
    seg = np.array([0, 0, 0, 1, 1, 1, 1, 2])
    times, labels = segment.segment_boundaries(seg, beats, n_frames=80, sr=22050)
    assert labels == [0, 1]
    assert times == [0.0, 35 * 512 / 22050, 79 * 512 / 22050]
    assert len(times) == len(labels) + 1


def test_times_follow_the_callers_rate():
    times, _ = segment.segment_boundaries(np.array([0, 0, 1, 1]), np.array([4, 8, 12]), n_frames=20, sr=44100)
    assert times == [0.0, 12 * 512 / 44100, 19 * 512 / 44100]


@pytest.mark.parametrize("k", [0, -1, 2.5, True])
def test_bad_k_raises(k):
    with pytest.raises(ValueError, match="k must be"):
        segment.laplacian_segmentation(np.zeros(22050, np.float32), 22050, k=k)


@pytest.mark.parametrize("sr", [0, -22050])
def test_bad_rate_raises(sr):
    with pytest.raises(ValueError, match="sr must be"):
        segment.laplacian_segmentation(np.zeros(22050, np.float32), sr, k=3)


def test_too_few_columns_raises():
    with pytest.raises(ValueError, match="beat-synchronous columns"):
        segment.check_columns(6, 3)
    with pytest.raises(ValueError, match="need at least 9"):
        segment.check_columns(8, 9)
    segment.check_columns(7, 3)
    segment.check_columns(9, 9)


def test_knn_count_and_sync_bounds():
    assert segment.knn_count(7) == 2 and segment.knn_count(8) == 2 * 2 and segment.knn_count(64) == 2 * 8
    assert segment.sync_bounds(np.array([0, 5, 9]), 12).tolist() == [0, 5, 9, 12]
    assert segment.sync_bounds(np.array([3, 5, 12]), 12).tolist() == [0, 3, 5, 12]
    assert ref.knn_k(301) == segment.knn_count(301)


def test_np_median_and_dct_helpers():
    import scipy.fftpack
    import torch

    x = np.random.default_rng(0).standard_normal((8, 5)).astype(np.float32)
    assert np.allclose(segment.np_median(torch.from_numpy(x), 0).numpy(), np.median(x, axis=0))
    db = np.random.default_rng(1).standard_normal((128, 3))
    want = scipy.fftpack.dct(db, axis=0, type=2, norm="ortho")[:20]
    assert np.allclose(segment.dct_matrix(20, 128).astype(np.float64) @ db, want, atol=1e-5)


def test_trim_and_last_beat_follow_the_recipe():
    rng = np.random.default_rng(2)
    ls = rng.standard_normal(200)
    cum, back = ref.beat_dp(ls, 10)
    assert segment.last_beat(cum) == int(np.flatnonzero(cum * ((cum > np.r_[cum[:1], cum[:-1]]) & (cum >= np.r_[cum[1:], cum[-1:]])) * 2
                                                       > np.median(cum[(cum > np.r_[cum[:1], cum[:-1]]) & (cum >= np.r_[cum[1:], cum[-1:]])])).max())
    beats = np.arange(5, 200, 10)
    import scipy.signal

    smooth = scipy.signal.convolve(ls[beats], scipy.signal.windows.hann(5), "same")
    valid = np.flatnonzero(smooth > 0)
    assert segment.trim_beats(ls, beats).tolist() == beats[valid.min(): valid.max()].tolist()


def test_tempo_prior_cuts_above_320_bpm():
    tg = np.zeros(344)
    tg[3] = 1.0  # 861 bpm: under the -inf part of the prior
    tg[22] = 0.5
    assert segment.tempo_from_tempogram(tg, 22050) == pytest.approx(60 * 22050 / (512 * 22))
    assert segment.tempo_from_tempogram(tg, 22050) == ref.tempo(tg, 22050)


@pytest.mark.parametrize("s", [7, 8, 64])
def test_lag_matrix_route_equals_the_diagonal_median(s):
    rng = np.random.default_rng(s)
    rec = rng.random((s, s))
    rec[rng.random((s, s)) < 0.4] = 0.0
    assert np.array_equal(ref.timelag_median_literal(rec), ref.timelag_median_formula(rec))


def test_kmeans_is_deterministic_and_finds_separated_clusters():
    rng = np.random.default_rng(3)
    x = np.concatenate([rng.normal(c, 0.05, (20, 2)) for c in ((0, 0), (3, 0), (0, 3))])
    a, b = segment.kmeans(x, 3), segment.kmeans(x, 3)
    assert np.array_equal(a, b)
    assert segment.relabel_first_appearance(a).tolist() == [0] * 20 + [1] * 20 + [2] * 20


@pytest.mark.parametrize("s,d", [(7, 20), (64, 20), (64, 252), (301, 20)])
def test_knn_rule_matches_librosas_search(s, d):
    """librosa's procedure: sklearn's k + 2 width nearest neighbours (self excluded), the |i - j| < width band removed, the k closest
    kept.  Equal to the restatement's rule wherever the k-th and (k+1)-th distances are not tied."""
    neighbors = pytest.importorskip("sklearn.neighbors")
    rng = np.random.default_rng(s + d)
    x = rng.standard_normal((d, s)).astype(np.float32)
    width = 3
    k = ref.knn_k(s, width)
    dist = ref.pair_distances(x)
    ours = ref.knn_sets(dist, k, width)
    knn = neighbors.NearestNeighbors(n_neighbors=min(s - 1, k + 2 * width), metric="euclidean").fit(x.T)
    graph = knn.kneighbors_graph(mode="distance").toarray()
    for i in range(s):
        cand = [j for j in np.flatnonzero(graph[i]) if abs(i - j) >= width]
        cand.sort(key=lambda j: graph[i, j])
        theirs = set(cand[:k])
        if theirs != ours[i]:
            row = sorted(dist[i, j] for j in range(s) if abs(i - j) >= width)
            assert len(row) > k and abs(row[k] - row[k - 1]) <= 1e-5 * row[k], (i, theirs ^ ours[i])
