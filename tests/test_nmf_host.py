"""CPU: the factorisation's reference (tests/nmf_ref.py) against known answers, its divergence on the planted case, the fp32 emulation
against the derived ceilings, the comparison helper against deliberately wrong variants, the host side of ``ar.nmf`` (normalisation and
ordering) and the refusals of the C entries (no device call is reached)."""
import numpy as np
import pytest
import torch

import nmf_ref as nr

CASES = nr.gpu_cases()


def test_the_case_list_covers_every_size():
    assert {c["F"] for c in CASES} == set(nr.FS) and {c["T"] for c in CASES} == set(nr.TS) and {c["K"] for c in CASES} == set(nr.KS)
    shapes = {(c["F"], c["T"], c["K"]) for c in CASES}
    assert (1025, 1, 32) in shapes and (1, 1000, 1) in shapes and set(nr.CHAINED) <= shapes
    for c in CASES:
        V, W, H = nr.make_case(c)
        assert V.dtype == W.dtype == H.dtype == np.float32 and (V > 0).all() and (W >= 0.5).all() and (H >= 0.5).all()
        assert (nr.product(W, H, 0.0) > 1e6 * nr.EPS).all()  # the clamp never decides


@pytest.mark.parametrize("dtype,tol", [(np.float64, 1e-14), (np.float32, 1e-6)], ids=["float64", "float32"])
def test_a_rank_one_matrix_is_a_fixed_point(dtype, tol):
    rng = np.random.default_rng(1)
    w, h = 0.5 + rng.random((37, 1)), 0.5 + rng.random((1, 53))
    V = w @ h
    W, H = nr.iterate(V, w, h, 5, dtype=dtype)
    assert nr.rel_error(W, w) < tol and nr.rel_error(H, h) < tol
    assert nr.divergence(V, w, h) < 1e-12
    W2, H2 = nr.iterate(V, 3.0 * w, h / 7.0, 1)  # one iteration from any scaling of the factors lands on a factorisation of V
    assert nr.rel_error(W2 @ H2, V) < 1e-14


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["float64", "float32"])
def test_zeros_are_absorbing(dtype):
    V, W, H = nr.make_case(dict(F=20, T=30, K=4, seed=3))
    rng = np.random.default_rng(4)
    zw, zh = rng.random(W.shape) < 0.2, rng.random(H.shape) < 0.2
    W[zw], H[zh] = 0, 0
    W[:, 2] = 0
    V[:, [0, 7, 29]] = 0
    H1 = nr.h_step(V, W, H, dtype=dtype)
    assert (H1[:, [0, 7, 29]] == 0).all() and (H1[2] == 0).all() and (H1[zh] == 0).all()
    W3, H3 = nr.iterate(V, W, H, 3, dtype=dtype)
    assert (W3[zw] == 0).all() and (H3[zh] == 0).all() and (W3[:, 2] == 0).all() and np.isfinite(W3).all() and np.isfinite(H3).all()
    assert nr.divergence_cols(V, W, H)[0] == nr.product(W, H, nr.EPS)[:, 0].sum()  # 0 log 0 = 0


def test_divergence_never_rises_on_the_planted_case():
    V, Wt, Ht = nr.planted()
    assert V.shape == (nr.PLANTED_F, nr.PLANTED_T) and V.dtype == np.float32
    ref = nr.planted_reference()
    d64 = ref["trace"]
    assert len(d64) == nr.PLANTED_ITERS + 1 and (np.diff(d64) < 0).all()
    d32, W32, _ = nr.divergence_trace(V, *nr.seeded_start(V, nr.PLANTED_K, nr.PLANTED_SEED), nr.PLANTED_ITERS, np.float32)
    assert (np.diff(d32) < 0).all()
    excess = (d32[-1] - d64[-1]) / d64[-1]
    print(f"planted: D64 {d64[-1]:.9g}, smallest decrease {(-np.diff(d64)).min():.3g}; emulation excess {excess:.3g}; "
          f"cosines {nr.template_cosines(ref['W'], Wt)}")
    assert excess <= nr.PLANTED_EXCESS * 1.01 and nr.PLANTED_MARGIN >= 4 * nr.PLANTED_EXCESS and nr.PLANTED_MARGIN >= 1e-6
    assert (nr.template_cosines(ref["W"], Wt) >= 0.9999).all() and (nr.template_cosines(W32, Wt) >= 0.9999).all()  # margin under 0.999


@pytest.mark.parametrize("case", CASES, ids=nr.case_id)
def test_the_emulation_stays_under_the_ceiling_and_sets_the_tolerances(case):
    ref, emu = nr.steps(case), nr.steps(case, np.float32)
    F, T, K = case["F"], case["T"], case["K"]
    e_h, e_w = nr.rel_error(emu["h_only"], ref["h_only"]), nr.rel_error(emu["w_only"], ref["w_only"])
    e_fw = nr.rel_error(emu["full"][0], ref["full"][0])
    assert e_h <= nr.h_ceiling(F, T, K) and e_w <= nr.w_only_ceiling(F, T, K) and e_fw <= nr.w_ceiling(F, T, K)
    assert 4 * e_h <= nr.H_STEP_TOL and 4 * e_w <= nr.W_ONLY_TOL and 4 * e_fw <= nr.W_AFTER_H_TOL  # the constants are 4 x the worst case
    assert nr.compare_steps(emu, ref) == []
    d32 = nr.divergence_cols(*nr.make_case(case), p_dtype=np.float32)
    assert (np.abs(d32 - nr.divergence_cols(*nr.make_case(case))) <= nr.divergence_tolerance(*nr.make_case(case))).all()


def test_the_tolerances_are_four_times_the_worst_emulation_error():
    worst = [max(nr.rel_error(pick(nr.steps(c, np.float32)), pick(nr.steps(c))) for c in CASES)
             for pick in (lambda s: s["h_only"], lambda s: s["w_only"], lambda s: s["full"][0])]
    for figure, tol in zip(worst, (nr.H_STEP_TOL, nr.W_ONLY_TOL, nr.W_AFTER_H_TOL)):
        assert 4 * figure <= tol <= 4 * figure * 1.1, (figure, tol)  # rounded up to two digits


DEFECTS = [dict(drop_last_row=True), dict(skip_component=0), dict(stale_h=True)]
DEFECT_CASES = [c for c in CASES if (c["F"], c["T"], c["K"]) in ((1025, 257, 16), (63, 64, 31), (2, 2, 2), (257, 255, 8))]


@pytest.mark.parametrize("defect", DEFECTS, ids=lambda d: next(iter(d)))
@pytest.mark.parametrize("case", DEFECT_CASES, ids=nr.case_id)
def test_an_emulation_with_one_defect_fails_the_comparison(case, defect):
    """The comparison of the GPU test (compare_steps at its tolerances) on an fp32 emulation that drops the last row of the H step's
    sums, skips component 0 of W.H, or feeds the old H to the W step."""
    bad = nr.steps(case, np.float32, **defect)
    complaints = nr.compare_steps(bad, nr.steps(case))
    assert complaints, defect
    if "stale_h" in defect:  # only the W of the full iteration sees it
        assert len(complaints) == 1 and "W of the full iteration" in complaints[0]


def test_normalisation_and_ordering():
    from maua_stylegan2_amd.audioreactive.decompose import _normalise_and_order

    rng = np.random.default_rng(6)
    W = rng.random((40, 6)).astype(np.float32) * np.array([1, 5, 0.1, 2, 1, 3], np.float32)
    W[:, 4] = W[:, 0]          # a tie: equal centroids keep their index order
    W[:, 2] = 0                # a dead component: centroid 0, first
    H = rng.random((6, 17)).astype(np.float32)
    Wn, Hn = _normalise_and_order(torch.from_numpy(W), torch.from_numpy(H))
    Wn, Hn = Wn.numpy(), Hn.numpy()
    want_w, want_h = nr.normalise_and_order(W, H)
    assert nr.rel_error(Wn, want_w) < 1e-6 and nr.rel_error(Hn, want_h) < 1e-6
    sums = Wn.sum(axis=0)
    assert np.allclose(sums[1:], 1, atol=1e-6) and sums[0] == 0
    assert np.allclose(Wn.astype(np.float64) @ Hn, W.astype(np.float64) @ H, rtol=1e-5, atol=1e-7)
    c = nr.centroids(Wn)
    assert (np.diff(c) >= 0).all()
    tie = [i for i in range(6) if np.allclose(Wn[:, i] * W[:, 0].sum(), W[:, 0], rtol=1e-5)]
    assert len(tie) == 2 and tie[1] == tie[0] + 1 and np.allclose(Hn[tie[0]], H[0] * W[:, 0].sum(), rtol=1e-5)


def test_seeded_start_is_deterministic_and_scaled():
    V, _, _ = nr.planted()
    W, H = nr.seeded_start(V, 3, 0)
    W2, H2 = nr.seeded_start(V, 3, 0)
    assert np.array_equal(W, W2) and np.array_equal(H, H2) and W.dtype == H.dtype == np.float32
    assert not np.array_equal(W, nr.seeded_start(V, 3, 1)[0])
    assert 0.5 < (W.astype(np.float64) @ H).mean() / (V.mean() / 4) < 2.0  # E[W.H] = K scale^2 / 4 = mean(V) / 4


def test_entries_refuse_bad_arguments_without_a_device(built_lib):
    """Validation comes before any HIP call (the pointers are never dereferenced on the host); n_iter = 0 returns 0 and launches
    nothing, so it too needs no device."""
    from maua_stylegan2_amd import _lib

    lib = _lib.load()
    fake = 0x1000
    ok = dict(v=fake, w=fake, h=fake, F=8, T=9, K=3, n_iter=0, uw=1, uh=1, eps=1e-12)

    def nmf(**kw):
        a = dict(ok, **kw)
        return lib.maua_nmf_kl_f32(a["v"], a["w"], a["h"], a["F"], a["T"], a["K"], a["n_iter"], a["uw"], a["uh"], a["eps"], None)

    def div(**kw):
        a = dict(ok, d=fake)
        a.update(kw)
        return lib.maua_nmf_kl_div_f32(a["v"], a["w"], a["h"], a["F"], a["T"], a["K"], a["eps"], a["d"], None)

    assert nmf() == 0 and nmf(K=32) == 0 and nmf(uw=0) == 0 and nmf(uh=0) == 0 and nmf(F=1 << 15, T=(1 << 16) - 1) == 0
    for kw in (dict(v=None), dict(w=None), dict(h=None), dict(F=0), dict(T=0), dict(K=0), dict(T=-3), dict(K=33), dict(n_iter=-1),
               dict(eps=0.0), dict(eps=-1.0), dict(eps=float("nan")), dict(eps=float("inf")), dict(uw=0, uh=0), dict(F=1 << 16, T=1 << 15)):
        assert nmf(**kw) == -22, kw
    for kw in (dict(v=None), dict(w=None), dict(h=None), dict(d=None), dict(F=0), dict(T=0), dict(K=0), dict(K=33), dict(eps=0.0),
               dict(eps=float("nan")), dict(F=1 << 16, T=1 << 15)):
        assert div(**kw) == -22, kw
    assert lib.maua_abi_version() == 8


def test_nmf_says_what_to_change():
    import maua_stylegan2_amd.audioreactive as ar

    V = np.ones((4, 5), np.float32)
    for kw in (dict(n_components=0), dict(n_components=33), dict(n_components=2, n_iter=-1), dict(n_components=2, eps=0.0)):
        with pytest.raises(ValueError, match="nmf:"):
            ar.nmf(V, **kw)
    assert callable(ar.decompose) and callable(ar.components) and ar.NMF_MAX_COMPONENTS == 32
