"""CPU: tests/hmm_ref.py — the numpy restatement of the two hidden-Markov-model entries — against brute-force enumeration of every
path and against hand-built models whose answer is known; the four deliberately wrong variants must each be caught by those same
comparisons.  Then the host side of audioreactive/harmony.py on a synthetic chromagram, no audio and no device: the vocabulary, the
observations, silent frames, the hold over N, root merging and the rotation to a tonic, decoded by the restatement."""
import math

import numpy as np
import pytest
import torch

import hmm_ref as q
from maua_stylegan2_amd.audioreactive import harmony

torch.set_grad_enabled(False)


# ------------------------------------------------------------------------------------------------ the restatement is right
def random_model(S, T, seed):
    case = dict(S=S, T=T, kind="random", seed=seed)
    return q.viterbi_operands(case)


def brute_force_failures(variant=None):
    """The comparisons against enumeration, S <= 3 and T <= 6: the path (where the best path is unique), its score, the marginals and
    the log-likelihood."""
    bad = []
    for S, T, seed in [(1, 1, 0), (1, 4, 1), (2, 1, 2), (2, 2, 3), (2, 6, 4), (3, 3, 5), (3, 5, 6), (3, 6, 7), (3, 6, 8), (2, 5, 9)]:
        logobs, log_trans, log_init = random_model(S, T, seed)
        top, best, marg, loglik = q.brute_force(logobs, log_trans, log_init)
        delta, back, states = q.viterbi(logobs, log_trans, log_init, variant)
        if len(best) == 1 and tuple(states.tolist()) != best[0]:
            bad.append(f"S={S} T={T}: path {states.tolist()} for {best[0]}")
        if abs(delta.max() - top) > 1e-12 * max(1.0, abs(top)):
            bad.append(f"S={S} T={T}: score {delta.max()} for {top}")
        if variant in (None, "transposed", "no_init"):
            obs = np.exp(logobs.astype(np.float64)).astype(np.float32)  # (the entry reads fp32 likelihoods: enumerate with those)
            _, _, marg, loglik = q.brute_force(np.log(obs.astype(np.float64)), log_trans, log_init)
            gamma, scale = q.posterior(obs, np.exp(log_trans), np.exp(log_init), variant)
            if np.abs(gamma - marg).max() > 1e-12:
                bad.append(f"S={S} T={T}: marginals off by {np.abs(gamma - marg).max():.3g}")
            if abs(np.log(scale).sum() - loglik) > 1e-12 * max(1.0, abs(loglik)):
                bad.append(f"S={S} T={T}: log-likelihood {np.log(scale).sum()} for {loglik}")
    return bad


def left_to_right(S=5, stay=3):
    """States 0 -> 1 -> ... -> S - 1, only 'stay' and 'advance' allowed, flat observations except that frame stay * k prefers state k:
    the path is 0 0 0 1 1 1 2 2 2 ..."""
    T = S * stay
    log_trans = np.full((S, S), -np.inf)
    for i in range(S):
        log_trans[i, i] = math.log(0.5)
        if i + 1 < S:
            log_trans[i, i + 1] = math.log(0.5)
    log_init = np.full(S, -np.inf)
    log_init[0] = 0.0
    logobs = np.zeros((T, S), np.float32)
    for k in range(S):
        logobs[stay * k, k] = 4.0
    return logobs, log_trans, log_init, np.repeat(np.arange(S), stay)


def hand_built_failures(variant=None):
    bad = []
    logobs, log_trans, log_init, want = left_to_right()
    delta, back, states = q.viterbi(logobs, log_trans, log_init, variant)
    if not np.array_equal(states, want):
        bad.append(f"left-to-right: {states.tolist()}")
    if variant in (None, "transposed", "no_init"):
        gamma, _ = q.posterior(np.exp(logobs.astype(np.float64)), np.exp(log_trans), np.exp(log_init), variant)
        ahead = np.triu(np.ones_like(gamma, dtype=bool), 1)  # state k cannot be reached before frame k
        if not (np.all(gamma[ahead] == 0) and abs(gamma[0, 0] - 1) < 1e-15 and gamma[-1, 0] < 0.01 and gamma[-1, -2:].sum() > 0.9):
            bad.append("left-to-right: the posterior does not start in state 0 and move to the last states")
    # forbidden transitions: two states that may never follow each other, the observations ask for a switch every frame
    lt = np.array([[0.0, -np.inf], [-np.inf, 0.0]])
    lo = np.array([[1, 0], [0, 5], [5, 0], [0, 5]], np.float32)
    _, _, states = q.viterbi(lo, lt, np.log([0.5, 0.5]), variant)
    if not np.array_equal(states, [1, 1, 1, 1]):
        bad.append(f"forbidden: {states.tolist()}")
    # all ties, integer operands: every path scores the same, the rules pick state 0 throughout
    S, T = 4, 6
    _, back, states = q.viterbi(np.ones((T, S), np.float32), np.full((S, S), -1.0), np.zeros(S), variant)
    if states.any() or back[1:].any():
        bad.append(f"ties: {states.tolist()}")
    # an initial distribution that decides: flat observations and transitions, the path stays where it starts
    lt = np.log(np.array([[0.9, 0.1], [0.1, 0.9]]))
    _, _, states = q.viterbi(np.zeros((3, 2), np.float32), lt, np.log([0.2, 0.8]), variant)
    if not np.array_equal(states, [1, 1, 1]):
        bad.append(f"init: {states.tolist()}")
    return bad


def test_restatement_against_brute_force():
    assert brute_force_failures() == []


def test_restatement_on_hand_built_models():
    assert hand_built_failures() == []


@pytest.mark.parametrize("variant", q.VARIANTS)
def test_the_comparisons_catch_a_wrong_variant(variant):
    caught = brute_force_failures(variant) + hand_built_failures(variant)
    print(f"{variant}: {len(caught)} failures, first: {caught[:1]}")
    assert caught


def test_corner_cases_of_the_definition():
    # a frame of nothing but -inf decodes to the lowest index; a NaN never replaces and is never replaced
    lo = np.zeros((3, 3), np.float32)
    lo[1] = -np.inf
    delta, back, states = q.viterbi(lo, np.zeros((3, 3)), np.zeros(3))
    assert np.isneginf(delta).all() and states.tolist() == [0, 0, 0]
    lo = np.zeros((3, 3), np.float32)
    lo[0, 0] = np.nan
    delta, back, _ = q.viterbi(lo, np.zeros((3, 3)), np.zeros(3))
    assert np.isnan(delta).all() and not back[1:].any()
    lo[0] = [0, np.nan, 1]
    delta, back, _ = q.viterbi(lo, np.zeros((3, 3)), np.zeros(3))
    assert back[1].tolist() == [2, 2, 2] and not np.isnan(delta).any()  # the NaN at source 1 loses against source 2, which beats source 0
    # the posterior of an all-zero frame: c = 0 and NaN from there on, in all of gamma
    ob = np.ones((4, 2), np.float32)
    ob[2] = 0
    gamma, scale = q.posterior(ob, np.full((2, 2), 0.5), [0.5, 0.5])
    assert scale[2] == 0 and np.isnan(scale[3]) and np.isfinite(scale[:2]).all() and np.isnan(gamma).all()
    # rows of gamma sum to one, and T = 1 is the normalised first frame
    obs, trans, init = q.posterior_operands(dict(S=7, T=40, kind="random", seed=3))
    gamma, scale = q.posterior(obs, trans, init)
    assert np.abs(gamma.sum(1) - 1).max() < 1e-13
    g1, s1 = q.posterior(obs[:1], trans, init)
    assert np.array_equal(g1[0], init * obs[0].astype(np.float64) / s1[0])


def test_case_lists_and_operands():
    for kinds, make in ((q.VITERBI_KINDS, q.viterbi_operands), (q.POSTERIOR_KINDS, q.posterior_operands)):
        cases = q.cases(kinds)
        assert len(cases) == len(kinds) * len(q.STATES) * len(q.FRAMES) and len({q.case_id(c) for c in cases}) == len(cases)
        for case in cases:
            if case["T"] > 3 or case["S"] > 25:
                continue
            frames, matrix, vector = make(case)
            assert frames.dtype == np.float32 and frames.shape == (case["T"], case["S"]) and matrix.shape == (case["S"],) * 2
            assert matrix.dtype == vector.dtype == np.float64
    lo, lt, li = q.viterbi_operands(dict(S=25, T=257, kind="integer", seed=5))
    _, back, _ = q.viterbi(lo, lt, li)
    assert all(len(np.unique(lt[:, j])) < 25 for j in range(25))  # ties in every column
    lo, lt, li = q.viterbi_operands(dict(S=25, T=3, kind="neginf", seed=5))
    assert np.isneginf(lt).any() and np.isfinite(np.diag(lt)).all() and np.isfinite(li).any()
    assert np.isnan(q.viterbi_operands(dict(S=25, T=3, kind="nan", seed=5))[0]).sum() == 1
    ob, tr, _ = q.posterior_operands(dict(S=25, T=3, kind="zero_row", seed=5))
    assert not ob[1].any() and ob[0].max() == 1
    assert (q.posterior_operands(dict(S=25, T=3, kind="zeros", seed=5))[1] == 0).any()
    assert q.same_bits_or_nan(np.array([1.0, np.nan]), np.array([1.0, -np.nan])) and not q.same_bits_or_nan(np.array([1.0, np.nan]), np.array([np.nan, 1.0]))
    assert not q.same_bits_or_nan(np.array([0.0]), np.array([-0.0]))


def test_entries_refuse_bad_arguments_without_a_gpu(built_lib):
    from maua_stylegan2_amd import _lib

    lib = _lib.load()
    fake = 0x1000  # never dereferenced
    vit = lambda **kw: lib.maua_hmm_viterbi_f64(*[kw.get(k, fake) for k in ("logobs", "trans", "init")], kw.get("T", 4), kw.get("S", 4),  # noqa: E731
                                                *[kw.get(k, fake) for k in ("delta", "back", "states")], None)
    post = lambda **kw: lib.maua_hmm_posterior_f64(*[kw.get(k, fake) for k in ("obs", "trans", "init")], kw.get("T", 4), kw.get("S", 4),  # noqa: E731
                                                   *[kw.get(k, fake) for k in ("gamma", "scale")], None)
    for name in ("logobs", "trans", "init", "delta", "back", "states"):
        assert vit(**{name: None}) == -22, name
    for name in ("obs", "trans", "init", "gamma", "scale"):
        assert post(**{name: None}) == -22, name
    for kw in (dict(T=0), dict(T=-1), dict(T=(1 << 22) + 1), dict(S=0), dict(S=-5), dict(S=129)):
        assert vit(**kw) == -22 and post(**kw) == -22, kw
    for fn, arg in ((harmony.viterbi, np.zeros((3, 129), np.float32)), (harmony.hmm_posterior, np.zeros((3, 129), np.float32)),
                    (harmony.viterbi, np.zeros((0, 4), np.float32)), (harmony.viterbi, np.zeros(4, np.float32))):
        with pytest.raises(ValueError):  # raised from the shapes, before anything touches a device
            fn(arg, np.zeros((arg.shape[-1],) * 2), np.zeros(arg.shape[-1]))
    with pytest.raises(ValueError, match="transition matrix"):
        harmony.viterbi(np.zeros((3, 4), np.float32), np.zeros((4, 5)), np.zeros(4))


# ------------------------------------------------------------------------------------------------ the chord model, host side
def test_chord_vocabulary():
    names, templates = harmony.chord_vocabulary("triads")
    assert len(names) == 25 and templates.shape == (25, 12) and templates.dtype == np.float32
    assert names[:3] == ["C:maj", "C#:maj", "D:maj"] and names[12] == "C:min" and names[23] == "B:min" and names[-1] == "N"
    assert np.abs(np.linalg.norm(templates.astype(np.float64), axis=1) - 1).max() < 1e-7
    assert np.flatnonzero(templates[names.index("A:min")]).tolist() == [0, 4, 9] and np.flatnonzero(templates[names.index("G:maj")]).tolist() == [2, 7, 11]
    assert np.all(templates[-1] == templates[-1][0]) and len({float(v) for v in templates[0] if v > 0}) == 1  # flat; binary
    names7, templates7 = harmony.chord_vocabulary("sevenths")
    assert len(names7) == 97 and names7[24:26] == ["C:7", "C#:7"] and names7[-2] == "B:sus4" and names7[-1] == "N"
    for name, pcs in (("G:7", [2, 5, 7, 11]), ("C:maj7", [0, 4, 7, 11]), ("A:min7", [0, 4, 7, 9]), ("B:dim", [2, 5, 11]), ("C:aug", [0, 4, 8]),
                      ("C:sus4", [0, 5, 7])):
        assert np.flatnonzero(templates7[names7.index(name)]).tolist() == pcs, name
    own, t_own = harmony.chord_vocabulary(["min", "dim"])
    assert own[0] == "C:min" and own[12] == "C:dim" and len(own) == 25 and np.array_equal(t_own[:12], templates[12:24])
    for bad in ("jazz", ["maj", "power"], [], ["maj", "maj"]):
        with pytest.raises(ValueError):
            harmony.chord_vocabulary(bad)
    for k in range(12):  # a root up a semitone is the template rotated by one
        assert np.array_equal(templates7[12 * 3 + (k + 1) % 12], np.roll(templates7[12 * 3 + k], 1))


def synthetic_chroma():
    """[12, 40]: 10 frames of C major, 5 nearly silent, 10 of A minor, 5 nearly silent, 10 of G major; a little of every other pitch
    class everywhere."""
    rng = np.random.default_rng(0)
    chroma = 0.05 * rng.random((12, 40))
    for lo, hi, pcs in ((0, 10, (0, 4, 7)), (15, 25, (9, 0, 4)), (30, 40, (7, 11, 2))):
        chroma[list(pcs), lo:hi] += np.array([1.0, 0.7, 0.8])[:, None]
    chroma[:, 10:15] *= 0.01
    chroma[:, 25:30] *= 0.01
    return chroma.astype(np.float32)


def decode(chroma, vocabulary="triads", kappa=20.0, hold=1.0, silence=0.02, frame_rate=10.0):
    names, templates = harmony.chord_vocabulary(vocabulary)
    ch = torch.from_numpy(chroma)
    silent = harmony.silent_frames(ch.sum(0), silence)
    cos = (torch.from_numpy(templates) @ harmony.unit_columns(ch)).t()
    logobs = harmony.chord_observations(cos, silent, kappa)
    log_trans, log_init = harmony.chord_transitions(len(names), frame_rate, hold)
    _, _, labels = q.viterbi(logobs.numpy(), log_trans, log_init)
    gamma, _ = q.posterior(harmony.likelihoods(logobs).numpy(), np.exp(log_trans), np.exp(log_init))
    return names, silent.numpy(), logobs.numpy(), labels, gamma


def test_observations_silence_and_transitions():
    chroma = synthetic_chroma()
    names, silent, logobs, labels, gamma = decode(chroma)
    N = len(names) - 1
    assert silent.tolist() == [False] * 10 + [True] * 5 + [False] * 10 + [True] * 5 + [False] * 10
    assert logobs.dtype == np.float32 and logobs.shape == (40, 25)
    assert np.all(logobs[silent, :N] == 0) and np.all(logobs[silent, N] == 20.0)
    unit = chroma.astype(np.float64) / np.linalg.norm(chroma.astype(np.float64), axis=0)
    want = 20.0 * harmony.chord_vocabulary("triads")[1].astype(np.float64) @ unit
    assert np.abs(logobs[~silent] - want.T[~silent]).max() < 2e-5   # kappa x a cosine in float32
    assert logobs[~silent].max() <= 20.0 + 2e-5
    want_labels = [names.index("C:maj")] * 10 + [N] * 5 + [names.index("A:min")] * 10 + [N] * 5 + [names.index("G:maj")] * 10
    assert labels.tolist() == want_labels
    assert np.all(gamma[np.arange(40), labels] > 0.9) and np.abs(gamma.sum(1) - 1).max() < 1e-12
    obs = harmony.likelihoods(torch.from_numpy(logobs)).numpy()
    assert obs.dtype == np.float32 and np.all(obs.max(1) == 1) and obs.min() >= 0
    # an all-zero clip is silent throughout (0 <= silence x 0)
    assert bool(harmony.silent_frames(torch.zeros(5), 0.02).all())
    assert not bool(harmony.unit_columns(torch.zeros(12, 3)).any())
    log_trans, log_init = harmony.chord_transitions(25, 43.066, 1.0)
    stay = math.exp(-1 / 43.066)
    assert np.allclose(np.diag(log_trans), math.log(stay), rtol=0, atol=1e-15) and np.allclose(log_trans[0, 1:], math.log((1 - stay) / 24), rtol=0, atol=1e-12)
    assert np.abs(np.exp(log_trans).sum(1) - 1).max() < 1e-12 and np.all(log_init == -math.log(25))
    assert harmony.chord_transitions(1, 43.0, 1.0)[0].tolist() == [[0.0]]
    with pytest.raises(ValueError):
        harmony.chord_transitions(25, 43.0, 0)


def test_a_longer_hold_changes_later_and_the_flicker_goes():
    """One frame of another chord inside a long one: the per-frame argmax follows it, the decoder does not."""
    chroma = synthetic_chroma()
    chroma[:, 5] = chroma[:, 35]  # a G major frame inside the C major
    names, _, logobs, labels, _ = decode(chroma, frame_rate=22050 / 512)
    assert int(np.argmax(logobs[5])) == names.index("G:maj") and labels[5] == names.index("C:maj")


def test_chord_rows_hold_merge_and_rotation():
    names, _ = harmony.chord_vocabulary("triads")
    N, c_maj, a_min, g_maj, c_min = 24, 0, 12 + 9, 7, 12
    labels = torch.tensor([N, N, c_maj, c_maj, N, a_min, N, g_maj, c_min, N], dtype=torch.int32)
    posterior = torch.rand(10, 25, generator=torch.Generator().manual_seed(0))
    posterior /= posterior.sum(1, keepdim=True)
    rows = harmony.chord_rows(labels, posterior, 25, by="chord")
    assert rows.shape == (10, 24) and rows.dtype == torch.float32 and bool((rows.sum(1) == 1).all())
    assert rows.argmax(1).tolist() == [c_maj, c_maj, c_maj, c_maj, c_maj, a_min, a_min, g_maj, c_min, c_min]  # N holds; leading N takes the first
    root = harmony.chord_rows(labels, posterior, 25, by="root")
    assert root.shape == (10, 12) and root.argmax(1).tolist() == [0, 0, 0, 0, 0, 9, 9, 7, 0, 0] and bool((root.sum(1) == 1).all())
    soft = harmony.chord_rows(labels, posterior, 25, by="chord", soft=True)
    held = [2, 2, 2, 3, 3, 5, 5, 7, 8, 8]
    assert torch.equal(soft, posterior[held, :24])
    soft_root = harmony.chord_rows(labels, posterior, 25, by="root", soft=True)
    assert torch.allclose(soft_root, posterior[held, :12] + posterior[held, 12:24], rtol=0, atol=1e-7)
    assert harmony.chord_rows(torch.full((4,), N, dtype=torch.int32), posterior[:4], 25) is None
    with pytest.raises(ValueError):
        harmony.chord_rows(labels, posterior, 25, by="bass")
    # rotation: with tonic G (7) a G chord lands in column 0, C (the subdominant) in column 5
    turned = harmony.rotate_roots(root, 7)
    assert turned.argmax(1).tolist() == [5, 5, 5, 5, 5, 2, 2, 0, 5, 5]
    assert torch.equal(harmony.rotate_roots(root, 0), root) and torch.equal(harmony.rotate_roots(harmony.rotate_roots(root, 7), 5), root)
    both = harmony.rotate_roots(rows, 7)  # by="chord": every block of 12 turns on its own
    assert both.argmax(1).tolist() == [5, 5, 5, 5, 5, 12 + 2, 12 + 2, 0, 12 + 5, 12 + 5]


def test_key_of_chroma():
    major, minor = np.array(harmony.KK_MAJOR), np.array(harmony.KK_MINOR)
    assert major[0] == 6.35 and major[7] == 5.19 and minor[0] == 6.33 and minor[3] == 5.38 and len(major) == len(minor) == 12
    for tonic in range(12):
        assert harmony.key_of_chroma(torch.from_numpy(np.roll(major, tonic)))[:3] == (tonic, "major", f"{harmony.NOTE_NAMES[tonic]} major")
        got = harmony.key_of_chroma(torch.from_numpy(3.0 * np.roll(minor, tonic) + 1.0))  # Pearson: scale and offset do not matter
        assert got[:2] == (tonic, "minor") and abs(float(got[3][12 + tonic]) - 1) < 1e-12
    assert harmony.key_of_chroma(torch.ones(12))[:2] == (0, "major")  # no variance: every score 0, the lowest index
    scale_c = np.zeros(12)
    scale_c[[0, 2, 4, 5, 7, 9, 11]] = 1.0
    scale_c[[0, 4, 7]] += 1.0
    assert harmony.key_of_chroma(torch.from_numpy(scale_c))[2] == "C major"
    assert harmony.key_of_chroma(torch.from_numpy(np.roll(scale_c, 6)))[2] == "F# major"
