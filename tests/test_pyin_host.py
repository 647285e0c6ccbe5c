"""CPU: the pYIN reference (tests/pyin_ref.py) against things that are not itself — the Viterbi restatement against brute-force
enumeration of every path, stage A on hand-built rows with known answers, the whole tracker on noisy tones that plain YIN gets wrong
and on the arpeggio — and four deliberately wrong variants that must fail these checks.  Also what the GPU tests rely on: the vectorised
decoder equals the scalar definition bit for bit, few frames of the stage-A case list are exempt, the entries refuse bad arguments
before any device call."""
import itertools
import math

import numpy as np
import pytest

import pitch_ref as pr
import pyin_ref as q


# ------------------------------------------------------------------------------------------------ Viterbi against brute force
def brute_force(lov, lou, width, consts):
    """(best score, the best path that is smallest read from its last state backwards) over every path of 2 P states."""
    T, P = lov.shape
    best, best_path = None, None
    for path in itertools.product(range(2 * P), repeat=T):
        s = q.path_score(path, lov, lou, width, *consts)
        if s is None:
            continue
        if best is None or s > best or (s == best and path[::-1] < best_path[::-1]):
            best, best_path = s, path
    return best, best_path


def real_consts(P, W):
    tri, norm = q.transition_tables(P, W)
    return tri, norm, -math.log(2 * P), math.log(0.99), math.log(0.01)


def integer_consts(P, W):
    """Integer-valued tables: every sum of the recursion is exact, so ties are real ties and the decoder's rule (lowest index at every
    choice) is the path that is smallest read backwards."""
    d = np.arange(-W, W + 1)
    return -np.abs(d).astype(np.float64), np.arange(P, dtype=np.float64) % 2, -1.0, 0.0, -1.0


SMALL = [(P, T, W) for P in (1, 2, 3) for T in (1, 2, 3, 5) for W in (0, 1, 2)]


def random_inputs(P, T, seed, tied):
    rng = np.random.default_rng(seed)
    if tied:
        return -rng.integers(0, 3, (T, P)).astype(np.float32), -rng.integers(0, 3, T).astype(np.float32)
    return np.log(rng.random((T, P)) + 1e-3).astype(np.float32), np.log(rng.random(T) + 1e-3).astype(np.float32)


def check_against_brute_force(decoder, tied, seeds=(0, 1, 2)):
    """Complaints of ``decoder`` over SMALL: the final maximum equals the best path's score exactly, the decoded path is that path (with
    tied inputs on integer tables: the smallest read backwards), and its own score is the maximum."""
    bad = []
    for P, T, W in SMALL:
        for seed in seeds:
            lov, lou = random_inputs(P, T, 100 * seed + 7 * P + T + W, tied)
            consts = integer_consts(P, W) if tied else real_consts(P, W)
            delta, back, states = decoder(lov, lou, W, *consts)
            score, path = brute_force(lov, lou, W, consts)
            if delta.max() != score:
                bad.append(f"P{P} T{T} W{W} seed {seed}: final maximum {delta.max()!r} != best path score {score!r}")
            elif tuple(int(s) for s in states) != path:
                bad.append(f"P{P} T{T} W{W} seed {seed}: path {states.tolist()} != {list(path)}")
    return bad


@pytest.mark.parametrize("tied", [False, True], ids=["random", "tied"])
def test_viterbi_reference_equals_brute_force(tied):
    assert check_against_brute_force(q.viterbi_loop, tied) == []
    assert check_against_brute_force(q.viterbi, tied) == []


def test_vectorised_decoder_equals_the_scalar_definition():
    """Bit for bit, -inf rows, an all -inf frame and a NaN included, on every small case of the GPU list and a few larger ones."""
    cases = [c for c in q.b_cases() if c["n_bins"] <= 65 and c["n_frames"] <= 3]
    cases += [dict(n_bins=7, width=w, n_frames=9, kind=kind, seed=40 + w) for w in (0, 2, 9) for kind in q.B_KINDS]
    assert len(cases) >= 20
    for case in cases:
        lov, lou = q.make_logobs(case)
        fast = q.viterbi(lov, lou, case["width"], *q.b_constants(case))
        slow = q.viterbi_loop(lov, lou, case["width"], *q.b_constants(case))
        for a, b, name in zip(fast, slow, ("delta_last", "backptr", "states")):
            assert np.array_equal(a, b, equal_nan=True), (q.b_case_id(case), name)


def test_an_all_minus_inf_frame_decodes_to_the_lowest_index():
    case = dict(n_bins=3, width=1, n_frames=4, kind="inf_frame", seed=3)
    lov, lou = q.make_logobs(case)
    delta, back, states = q.viterbi_loop(lov, lou, 1, *q.b_constants(case))
    assert (delta == -np.inf).all() and states[-1] == 0
    assert (back[3] == np.array([0, 0, 1, 0, 0, 1])).all()  # every window keeps its first element


def merging_case():
    """Two candidates that differ by one ulp before the voicing constant is added and round to the same number after it: the arg-max
    taken first picks the larger (bin 1), the constant added first ties them and the tie goes to bin 0."""
    P, W = 2, 1
    tri, norm = np.zeros(3), np.zeros(2)
    lov = np.array([[1.0, np.float32(1.0) + np.float32(2.0 ** -23)], [0.0, -50.0]], np.float32)
    lou = np.array([-np.inf, -np.inf], np.float32)
    return lov, lou, W, (tri, norm, 0.0, -1.0e12, -2.0e12)


def test_the_constant_is_added_after_the_argmax():
    lov, lou, W, consts = merging_case()
    _, back, states = q.viterbi_loop(lov, lou, W, *consts)
    assert states.tolist() == [1, 0] and back[1, 0] == 1
    _, back, states = q.viterbi(lov, lou, W, *consts)
    assert states.tolist() == [1, 0] and back[1, 0] == 1


# ------------------------------------------------------------------------------------------------ stage A on hand-built rows
CUM10 = np.arange(11, dtype=np.float32) / np.float32(10)      # a uniform prior over 10 thresholds: cum[k] = k / 10, exact enough to read
EDGES = np.array([8.5, 6.5, 4.5, 2.5, 0.5], np.float32)      # bins of two lags each: (6.5, 8.5], (4.5, 6.5], (2.5, 4.5], (0.5, 2.5]


def stage_a(row, tau_min=1, no_trough=0.0, **kw):
    r = np.asarray([row], np.float32)
    return q.candidates(r, tau_min, r.shape[1] - 1, CUM10, 10, no_trough, EDGES, **kw)


def test_one_trough():
    #            0    1    2    3     4    5    6    7    8
    a = stage_a([1.0, 0.9, 0.8, 0.25, 0.8, 0.9, 1.0, 1.0, 1.0])
    assert [(c[0], c[3]) for c in a["cands"][0]] == [(3, 2)]
    assert a["obs"][0].tolist() == [0, 0, np.float32(1.0) - np.float32(0.2), 0]   # thresholds 0.3 .. 1.0: cum[10] - cum[2]
    assert a["period"][0, 2] == 3.0 and a["voiced_prob"][0] == a["obs"][0, 2]
    b = stage_a([1.0, 0.9, 0.8, 0.25, 0.8, 0.9, 1.0, 1.0, 1.0], no_trough=0.5)     # + 0.5 x cum[2]: the thresholds nothing gets under
    assert b["obs"][0, 2] == np.float32(0.8) + np.float32(np.float32(0.5) * np.float32(0.2))


def test_two_descending_record_troughs_share_the_thresholds():
    #            0    1    2     3    4    5     6    7    8
    a = stage_a([1.0, 0.9, 0.55, 0.9, 0.9, 0.15, 0.3, 0.9, 1.0])
    assert [(c[0], c[3]) for c in a["cands"][0]] == [(2, 3), (5, 1)]
    assert a["obs"][0, 3] == CUM10[10] - CUM10[5]       # the first trough owns the thresholds 0.6 .. 1.0
    assert a["obs"][0, 1] == CUM10[5] - CUM10[1]        # the lower one those it alone gets under: 0.2 .. 0.5
    assert 5.0 < a["period"][0, 1] < 5.5                # refined towards the lower neighbour
    assert abs(float(a["voiced_prob"][0]) - 0.9) < 1e-6


def test_a_trough_that_is_no_record_gets_nothing():
    #            0    1    2    3    4    5     6    7    8
    a = stage_a([1.0, 0.9, 0.2, 0.9, 0.9, 0.45, 0.9, 0.9, 1.0])
    assert [c[0] for c in a["cands"][0]] == [2]
    assert a["obs"][0].tolist() == [0, 0, 0, CUM10[10] - CUM10[2]] and a["period"][0].tolist() == [0, 0, 0, 2.0]
    wrong = stage_a([1.0, 0.9, 0.2, 0.9, 0.9, 0.45, 0.9, 0.9, 1.0], first_only=False)
    assert wrong["obs"][0, 1] > 0                       # (the deliberate defect hands the second trough mass)


def test_no_trough_a_plateau_a_trough_at_tau_min_and_heights_from_one_up():
    rising = stage_a([1.0, 0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8], tau_min=2)   # the left neighbour of tau_min counts as +inf, whatever it is
    assert [c[0] for c in rising["cands"][0]] == [2] and rising["period"][0, 3] == 2.0   # (a straight line: no curvature, not refined)
    at_min = stage_a([1.0, 0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8], tau_min=1)
    assert [c[0] for c in at_min["cands"][0]] == [1] and at_min["period"][0, 3] == 1.0   # (tau - 1 < 1: not refined)
    falling = stage_a([1.0, 0.9, 0.8, 0.7, 0.6, 0.5, 0.4, 0.3, 0.2])             # tau_max is never a trough
    assert falling["cands"][0] == [] and not falling["obs"].any() and not falling["period"].any() and falling["voiced_prob"][0] == 0
    plateau = stage_a([1.0, 0.9, 0.3, 0.3, 0.3, 0.9, 1.0, 1.0, 1.0])             # < on the left, <= on the right: its first lag only
    assert [c[0] for c in plateau["cands"][0]] == [2]
    high = stage_a([1.0, 1.5, 1.0, 1.5, 1.25, 1.5, 1.5, 1.5, 1.5], no_trough=0.0)   # heights >= 1 lie under no threshold
    assert high["cands"][0] == [] and high["voiced_prob"][0] == 0
    high = stage_a([1.0, 1.5, 1.0, 1.5, 1.25, 1.5, 1.5, 1.5, 1.5], no_trough=0.25)  # ... the fallback still picks the global minimum
    assert [c[0] for c in high["cands"][0]] == [2] and high["voiced_prob"][0] == 0.25


def test_threshold_index():
    x = np.array([-np.inf, -1.0, 0.0, 0.0999, 0.1, 0.5, 0.999, 1.0, 7.0, np.inf, np.nan], np.float32)
    assert q.thr_index(x, 10).tolist() == [0, 0, 0, 0, 1, 5, 9, 10, 10, 10, 10]
    assert q.thr_index(x, 1).tolist() == [0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1]


def test_host_tables():
    cum = q.threshold_prior()
    assert cum.dtype == np.float32 and cum[0] == 0 and abs(float(cum[-1]) - 1) < 1e-6 and (np.diff(cum) >= 0).all()
    assert (q.pitch_bins(65.0, 2100.0, 10), q.transition_width(35.92, 512, 22050, 10)) == (602, 50)
    edges = q.bin_edges(22050, 65.0, 10, 602)
    assert (np.diff(edges) < 0).all() and edges[0] > 22050 / 65.0 > edges[1]
    tri, norm = q.transition_tables(5, 2)
    assert np.allclose(np.exp(tri), [1, 2, 3, 2, 1]) and np.allclose(np.exp(norm), [6, 8, 9, 8, 6])


def test_stage_a_case_list_is_usable():
    """Few frames of a case have a candidate within twice the period tolerance of a bin edge (decided here, on the CPU), the float32
    restatement stays within the quoted figure of the float64 one, and the two agree on every discrete decision."""
    worst = 0.0
    for case in q.a_cases():
        _, edges = q.case_tables(case)
        r32, r64 = q.a_reference(case), q.a_reference(case, np.float64)
        assert int(q.near_edge_frames(r32, edges).sum()) <= q.max_exempt(case["n_frames"]), q.a_case_id(case)
        assert [[c[0] for c in f] for f in r32["cands"]] == [[c[0] for c in f] for f in r64["cands"]], q.a_case_id(case)
        both = (r32["period"] > 0) & (r64["period"] > 0)
        if both.any():
            worst = max(worst, float(np.max(np.abs(r32["period"][both] - r64["period"][both]) / r64["period"][both])))
        assert q.compare_candidates(r32, r32, edges) == []
    print(f"period, fp32 against float64: {worst:.3g} relative (quoted {q.PERIOD_FIGURE:.3g})")
    assert worst <= q.PERIOD_FIGURE * 1.001


# ------------------------------------------------------------------------------------------------ known answers
def noisy_failures(**variant):
    """Complaints over the four noisy tones: every interior frame voiced and within 100 cents, plain YIN wrong on >= 40 % of them."""
    bad = []
    for (freq, snr), quoted in zip(q.NOISY_CASES, q.NOISY_WORST_CENTS):
        y = q.noisy_tone(freq, snr)
        got = q.pyin(y, pr.TONE_SR, **variant)
        c = pr.cents(got["f0"][q.INTERIOR], freq)
        wrong = float(np.mean(pr.cents(q.yin_f0(y)[q.INTERIOR], freq) > 50))
        print(f"{freq} Hz {snr} dB: worst {c.max():.1f} cents (quoted {quoted}), YIN wrong on {100 * wrong:.0f} %")
        if not got["voiced_flag"][q.INTERIOR].all():
            bad.append(f"{freq} Hz {snr} dB: {int((~got['voiced_flag'][q.INTERIOR]).sum())} interior frames unvoiced")
        if not c.max() <= q.NOISY_BOUND_CENTS:
            bad.append(f"{freq} Hz {snr} dB: worst {c.max():.1f} cents")
        if not abs(c.max() - quoted) <= 0.06:
            bad.append(f"{freq} Hz {snr} dB: worst {c.max():.2f} cents, pyin_ref.py quotes {quoted}")
        if not wrong >= q.NOISY_YIN_WRONG:
            bad.append(f"{freq} Hz {snr} dB: plain YIN is wrong on only {100 * wrong:.0f} % of the frames")
    return bad


def arpeggio_failures(**variant):
    y, _ = pr.arpeggio()
    got = q.pyin(y, pr.TONE_SR, **variant)
    inside, silent = q.arpeggio_frame_sets()
    assert len(inside) == 24 and len(silent) == 18
    bad = [f"frame {t} inside a note is unvoiced" for t, _ in inside if not got["voiced_flag"][t]]
    worst = max(float(pr.cents(got["f0"][t], f)) for t, f in inside)
    print(f"arpeggio: worst {worst:.3f} cents inside the notes (bound {q.ARPEGGIO_BOUND_CENTS})")
    if not worst <= q.ARPEGGIO_BOUND_CENTS:
        bad.append(f"worst {worst:.3f} cents inside a note")
    bad += [f"silent frame {t} is voiced" for t in silent if got["voiced_flag"][t]]
    return bad


def test_noisy_tones_that_plain_yin_gets_wrong():
    assert noisy_failures() == []


def test_arpeggio_notes_and_silences():
    assert arpeggio_failures() == []
    assert q.ARPEGGIO_BOUND_CENTS >= 1.5 * q.ARPEGGIO_WORST_CENTS


# ------------------------------------------------------------------------------------------------ deliberate defects
def test_ties_broken_towards_the_higher_index_fail():
    wrong = lambda *a: q.viterbi_loop(*a, tie_high=True)  # noqa: E731
    assert check_against_brute_force(wrong, tied=True) != []


def test_the_constant_added_before_the_argmax_fails():
    lov, lou, W, consts = merging_case()
    _, back, states = q.viterbi_loop(lov, lou, W, *consts, add_first=True)
    assert states.tolist() != [1, 0]


def test_the_normaliser_dropped_fails():
    wrong = lambda *a: q.viterbi_loop(*a, normalise=False)  # noqa: E731
    assert check_against_brute_force(wrong, tied=False) != []


def test_mass_for_every_trough_below_the_threshold_fails():
    """Every trough taking every threshold it lies under hands the subharmonics and the noise troughs the mass that belongs to the first
    trough below: the known answers no longer hold."""
    assert noisy_failures(first_only=False) + arpeggio_failures(first_only=False) != []


# ------------------------------------------------------------------------------------------------ the entries' argument checks (no device call)
def test_entries_refuse_bad_arguments_without_a_gpu(built_lib):
    from maua_stylegan2_amd import _lib

    lib = _lib.load()
    fake = 0x1000  # never dereferenced: these calls are refused during validation
    good = dict(cmndf=fake, n_frames=3, tau_min=10, tau_max=340, cum=fake, n_thr=100, ntp=0.01, edge=fake, n_bins=602, obs=fake, period=fake, vp=fake)

    def cand(**kw):
        a = dict(good, **kw)
        return lib.maua_pyin_candidates_f32(a["cmndf"], a["n_frames"], a["tau_min"], a["tau_max"], a["cum"], a["n_thr"], a["ntp"], a["edge"],
                                            a["n_bins"], a["obs"], a["period"], a["vp"], None)

    for kw in ([{k: None} for k in ("cmndf", "cum", "edge", "obs", "period", "vp")]
               + [dict(n_frames=0), dict(tau_min=0), dict(tau_min=340), dict(tau_max=2049), dict(n_thr=0), dict(n_thr=257), dict(n_bins=0),
                  dict(n_bins=1025), dict(ntp=-0.1), dict(ntp=1.5), dict(ntp=float("nan")), dict(ntp=float("inf"))]):
        assert cand(**kw) == -22, kw
    good_b = dict(lov=fake, lou=fake, T=3, P=602, W=50, tri=fake, norm=fake, delta=fake, back=fake, states=fake)

    def vit(**kw):
        a = dict(good_b, **kw)
        return lib.maua_pyin_viterbi_f64(a["lov"], a["lou"], a["T"], a["P"], a["W"], a["tri"], a["norm"], -1.0, -0.01, -4.6, a["delta"],
                                         a["back"], a["states"], None)

    for kw in [{k: None} for k in ("lov", "lou", "tri", "norm", "delta", "back", "states")] + [dict(T=0), dict(P=0), dict(P=1025), dict(W=-1), dict(W=129)]:
        assert vit(**kw) == -22, kw


def test_limits_have_twins_in_signal_py():
    import os
    import re

    from conftest import REPO
    from maua_stylegan2_amd.audioreactive import signal

    header = open(os.path.join(REPO, "include", "maua_hip.h")).read()
    limit = lambda name: int(re.search(rf"#define {name} (\d+)", header).group(1))  # noqa: E731
    assert (signal.PYIN_MAX_BINS, signal.PYIN_MAX_THRESHOLDS, signal.PYIN_MAX_WIDTH) == (limit("MAUA_PYIN_MAX_BINS"), limit("MAUA_PYIN_MAX_THRESHOLDS"),
                                                                                        limit("MAUA_PYIN_MAX_WIDTH")) == (q.MAX_BINS, q.MAX_THRESHOLDS, q.MAX_WIDTH)
