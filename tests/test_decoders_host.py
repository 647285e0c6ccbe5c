"""CPU: what gives tests/test_decoders_property_gpu.py and the edge lists of tests/hmm_ref.py and tests/pyin_ref.py their meaning.
The edge lists reach the edges they name (the walk-back chunking of csrc/hmm.hip is restated in hmm_ref.chunks); every identity the
device test checks holds between the numpy restatements on the same cases, so a failure on the device implicates a kernel; every
deliberately wrong decoder, put on one side, breaks an identity on a listed case; the explicit examples of the strategies pin the
coverage and every draw stays in range; and maua_bar_lds_bytes agrees with its restatement."""
import functools

import numpy as np
import pytest

import bar_ref
import decoder_cases as dc
import hmm_ref
import pyin_ref

REF = dict(hmm=hmm_ref.viterbi, pyin=pyin_ref.viterbi, bar=bar_ref.decode)


# ------------------------------------------------------------------------------------------------ the edge lists reach what they name
def test_chunking_restated():
    R = hmm_ref.TRACE_ROWS
    assert hmm_ref.chunks(1) == [(0, 1)] and hmm_ref.chunks(R) == [(0, R)] and hmm_ref.chunks(R + 1) == [(1, R), (0, 1)]
    assert hmm_ref.chunks(2 * R) == [(R, R), (0, R)] and hmm_ref.chunks(2 * R + 1) == [(R + 1, R), (1, R), (0, 1)]
    for T in (1, 2, R - 1, R, R + 1, 2000, 2 * R + 1, 5000):   # the chunks tile 0 .. T - 1 without gap or overlap, last frame first
        rows = [lo + r for lo, n in hmm_ref.chunks(T) for r in range(n - 1, -1, -1)]
        assert rows == list(range(T - 1, -1, -1)), T
    back = np.random.default_rng(0).integers(0, 5, (2 * R + 7, 5)).astype(np.uint8)
    back[0] = np.arange(5)
    plain = np.zeros(len(back), np.int32)
    s = plain[-1] = 3
    for t in range(len(back) - 1, 0, -1):
        s = plain[t - 1] = back[t][s]
    assert np.array_equal(hmm_ref.walk_back(back, 3), plain)
    for variant in hmm_ref.CHUNK_VARIANTS:
        assert not np.array_equal(hmm_ref.walk_back(back, 3, variant), plain), variant
        assert np.array_equal(hmm_ref.walk_back(back[:R - 1], 3, variant), hmm_ref.walk_back(back[:R - 1], 3)), variant   # one chunk: nothing to get wrong


def test_hmm_edge_list_reaches_the_chunk_and_wave_edges():
    R = hmm_ref.TRACE_ROWS
    shapes = {T: hmm_ref.chunks(T) for _, T in hmm_ref.EDGE_CASES}
    sizes = {T: [n for _, n in c] for T, c in shapes.items()}
    assert [R] in sizes.values()            # one chunk, exactly full
    assert [R, 1] in sizes.values()         # a last chunk of one row
    assert [R, R] in sizes.values()         # two full chunks
    assert [R, R, 1] in sizes.values()      # two full chunks and a row
    assert [R - 1] in sizes.values() and [R, R - 1] in sizes.values()   # and one row short of each
    assert set(hmm_ref.SWEEP_STATES) - {1, 2} <= {S for S, _ in hmm_ref.EDGE_CASES}   # (1 and 2 are on hmm_ref.STATES)
    assert set(hmm_ref.SWEEP_STATES) <= {S for S, _ in hmm_ref.EDGE_CASES} | set(hmm_ref.STATES)
    assert {T % 2 for _, T in hmm_ref.EDGE_CASES} == {0, 1}                          # the posterior's two buffers, both ways round
    assert not any(T in (R, R + 1, 2 * R, 2 * R + 1) for T in hmm_ref.FRAMES + (hmm_ref.LONG_CASE["T"],))   # (why the list was needed)
    for kinds in (hmm_ref.EDGE_VITERBI_KINDS, hmm_ref.EDGE_POSTERIOR_KINDS):
        cases = hmm_ref.edge_cases(kinds)
        assert len(cases) == len(kinds) * len(hmm_ref.EDGE_CASES) and len({hmm_ref.case_id(c) for c in cases}) == len(cases)
        assert len({c["seed"] for c in cases}) == len(cases)


def test_pyin_edge_list_reaches_the_clamp_at_every_wave_count():
    pairs = set(pyin_ref.EDGE_CASES)
    for name, bins in (("one wave", (63, 64)), ("the 64 / 65 boundary", (65,)), ("two waves", (127, 128))):
        for relation in (lambda P, W: W == P - 2, lambda P, W: W == P - 1, lambda P, W: W >= P):
            assert any(P in bins and relation(P, W) for P, W in pairs), name
    assert (129, 128) in pairs and all(W <= pyin_ref.MAX_WIDTH for _, W in pairs)    # (W >= P ends at P = 128: the width limit)
    cases = pyin_ref.edge_cases()
    assert len(cases) == len(pairs) * len(pyin_ref.EDGE_KINDS) and len({pyin_ref.b_case_id(c) for c in cases}) == len(cases)
    assert {"integer", "random"} <= {c["kind"] for c in cases}
    for P, W in pairs:
        assert {c["n_frames"] for c in cases if (c["n_bins"], c["width"]) == (P, W)} == set(pyin_ref.EDGE_FRAMES)
    lov, lou = pyin_ref.make_logobs(dict(n_bins=5, width=4, n_frames=4, kind="corners", seed=1))
    assert np.argmax(lov, 1).tolist() == [0, 4, 0, 4] and lov.max() <= 0 and np.all(np.sort(lov, 1)[:, -2] == -40)


# ------------------------------------------------------------------------------------------------ the restatements themselves
def test_vectorised_pyin_decoder_equals_the_scalar_definition_on_nan_observations():
    """The random-shape test draws the NaN kind at any size, so pyin_ref.viterbi handles a NaN observation in vector form: bit for
    bit the scalar definition, with one NaN, a frame of NaN, a NaN in the unvoiced column and NaN in the first frame, up to three waves
    with W >= P - 1 and W < P - 1 at the width limit."""
    n = 0
    for P, W, T in [(1, 0, 3), (2, 1, 4), (3, 5, 4), (7, 2, 9), (20, 3, 8), (20, 25, 8), (33, 40, 5), (129, 128, 4), (160, 128, 3)]:
        for seed in range(4):
            lov, lou = pyin_ref.make_logobs(dict(n_bins=P, width=W, n_frames=T, kind="nan", seed=seed))
            if seed == 1:
                lou[T // 2] = np.nan
            if seed == 2:
                lov[1, 0] = lov[0, P - 1] = np.nan
            if seed == 3:
                lov[1, :] = np.nan
            consts = pyin_ref.b_constants(dict(n_bins=P, width=W))
            fast, slow = pyin_ref.viterbi(lov, lou, W, *consts), pyin_ref.viterbi_loop(lov, lou, W, *consts)
            for a, b, name in zip(fast, slow, ("delta_last", "backptr", "states")):
                assert np.array_equal(a, b, equal_nan=True), (P, W, T, seed, name)
            n += 1
    assert n == 36


def test_pyin_expand():
    P, W = 4, 1
    consts = pyin_ref.integer_constants(P, W)
    lt, li = pyin_ref.expand(P, W, *consts)
    tri, norm, init, stay, switch = consts
    assert lt.shape == (8, 8) and li.tolist() == [init] * 8
    assert lt[0, 0] == (-norm[0] + tri[1]) + stay and lt[1, 2] == (-norm[1] + tri[2]) + stay and lt[2, 1] == (-norm[2] + tri[0]) + stay
    assert lt[1, 4 + 2] == (-norm[1] + tri[2]) + switch and lt[4 + 3, 2] == (-norm[3] + tri[0]) + switch and lt[4 + 3, 4 + 3] == (-norm[3] + tri[1]) + stay
    assert np.isneginf(lt[0, 2]) and np.isneginf(lt[0, 4 + 2]) and np.isneginf(lt[4 + 3, 1]) and np.isfinite(lt).sum() == 4 * (3 * P - 2)
    obs = pyin_ref.dense_observations(np.arange(8, dtype=np.float32).reshape(2, 4), np.array([-1, -2], np.float32))
    assert obs.dtype == np.float32 and obs.tolist() == [[0, 1, 2, 3, -1, -1, -1, -1], [4, 5, 6, 7, -2, -2, -2, -2]]


# ------------------------------------------------------------------------------------------------ the identities, and that they can fail
def test_the_identities_hold_between_the_restatements():
    assert dc.identity_complaints(**REF) == []
    # the cases are what the device test's docstring says they are
    assert {(1, 0), (64, 0)} <= {(P, W) for P, W, _ in dc.PYIN_DENSE} and all(2 * P <= hmm_ref.MAX_STATES for P, _, _ in dc.PYIN_DENSE)
    for wanted in (lambda P, W, T: W == P - 1 and P > 1, lambda P, W, T: W >= P, lambda P, W, T: T == 1, lambda P, W, T: P == 64):
        assert any(wanted(*c) for c in dc.PYIN_DENSE)
    assert all(sum(iv) * B <= hmm_ref.MAX_STATES for iv, B, _ in dc.BAR_DENSE) and len(dc.BAR_DENSE) >= 10 and len(dc.PYIN_DENSE) >= 10
    R = hmm_ref.TRACE_ROWS
    assert any(T > R for _, T in dc.HMM_SHIFT) and any(T > 2 * R for _, T in dc.HMM_SHIFT)
    assert any({R - 1, R, R + 1} <= set(prefixes) and T > R + 1 for _, T, prefixes in dc.HMM_PREFIX)
    for iv, beats, T in dc.BAR_SHIFT:
        assert bar_ref.lds_bytes(len(iv), max(beats), iv[-1]) > 0
    # the operands are integers throughout, and ties are everywhere: the identities are exact, not lucky
    for ops in (dc.pyin_integer_operands(7, 6, 12, 0)[:2] + dc.pyin_integer_operands(7, 6, 12, 0)[3:5], dc.bar_integer_operands([3, 4, 5, 7], 33, 0)):
        for a in ops:
            assert np.array_equal(np.asarray(a, np.float64), np.round(np.asarray(a, np.float64)))
    lo, I, W, lc = dc.bar_integer_operands([3, 4, 5, 7], 33, 0)
    assert len(np.unique(lc)) <= 4 and len(np.unique(lo)) <= 3


def wrong_pyin(reach):
    return lambda lov, lou, W, *consts: pyin_ref.viterbi(lov, lou, W, *consts, reach=reach(W, lov.shape[1]))


SHORT_REACH = lambda W, P: max(0, min(W, P - 2))   # noqa: E731  the scan one offset short where W >= P - 1
LONG_REACH = lambda W, P: min(W, P)                # noqa: E731  the clamp the scan would have without its "- 1"


@pytest.mark.parametrize("variant", hmm_ref.VARIANTS + hmm_ref.CHUNK_VARIANTS)
def test_a_wrong_dense_decoder_breaks_an_identity(variant):
    bad = dc.identity_complaints(**REF, hmm_other=functools.partial(hmm_ref.viterbi, variant=variant))
    print(f"{variant}: {len(bad)} complaints, first {bad[:2]}")
    assert bad
    if variant in hmm_ref.CHUNK_VARIANTS:   # only a walk back of more than one chunk shows them: the shift cases past 1024 frames
        assert {b.split(":")[0] for b in bad} == {"hmm-shift (3, 1025)", "hmm-shift (65, 2049)"}
        # ... and only because the OTHER side is right here.  On the device both sides of the shift are the same kernel: a wrong walk back
        # gives the same wrong states twice and the identity holds.  What guards the device against it is the bit-for-bit comparison over
        # hmm_ref.EDGE_CASES (and the T = 2000 cases), as test_which_lists_catch_the_new_wrong_variants measures — not the identities.
        wrong = functools.partial(hmm_ref.viterbi, variant=variant)
        assert [b for case in dc.HMM_SHIFT for b in dc.check_hmm_shift(case, wrong, wrong)] == []


@pytest.mark.parametrize("variant", bar_ref.VARIANTS)
def test_a_wrong_bar_decoder_breaks_an_identity(variant):
    bad = dc.identity_complaints(**REF, bar_other=functools.partial(bar_ref.decode, variant=variant))
    print(f"{variant}: {len(bad)} complaints, first {bad[:2]}")
    assert bad


def test_a_short_pyin_scan_breaks_an_identity_and_a_long_one_is_no_defect():
    """reach = min(W, P - 2) loses the farthest source and is caught.  reach = min(W, P), the clamp without its "- 1", is measured to
    change nothing at all: offsets +-P leave [0, P - 1] for every lane and land on the W >= P elements of -inf either side of the
    row, which never win — so no list can catch it, and the kernel would stay inside its buffers with it."""
    bad = dc.identity_complaints(**REF, pyin_other=wrong_pyin(SHORT_REACH))
    print(f"short reach: {len(bad)} complaints, first {bad[:2]}")
    assert bad
    assert dc.identity_complaints(**REF, pyin_other=wrong_pyin(LONG_REACH)) == []
    for case in pyin_ref.edge_cases() + [c for c in pyin_ref.b_cases() if c["kind"] != "nan" and c["n_bins"] <= 65]:
        ops = dc.pyin_operands(case)
        for a, b in zip(pyin_ref.viterbi(*ops), wrong_pyin(LONG_REACH)(*ops)):
            assert np.array_equal(a, b), pyin_ref.b_case_id(case)


# Measured by the test below, not expected: which bit-for-bit case lists tell the two new wrong decoders from the definition.
CAUGHT_BY = {("chunk_repeat", "before"): True, ("chunk_repeat", "edge"): True, ("chunk_drop", "before"): True, ("chunk_drop", "edge"): True,
             ("short_reach", "before"): True, ("short_reach", "edge"): True, ("short_reach", "edge without corners"): False}


def test_which_lists_catch_the_new_wrong_variants():
    """The lists from before this change (hmm_ref.cases at T = 2000, two chunks; pyin_ref.b_cases at P <= 3) do catch both: what they
    lacked is the edges, not the power to see these defects.  The pYIN edge pairs with the integer and random kinds alone do not catch
    the short scan — the farthest source never wins there — which is why the list has the corners kind."""
    got = {}
    lists = {"before": [c for c in hmm_ref.cases(hmm_ref.VITERBI_KINDS) if c["T"] >= hmm_ref.TRACE_ROWS and c["S"] <= 25],
             "edge": [c for c in hmm_ref.edge_cases(hmm_ref.EDGE_VITERBI_KINDS) if c["S"] <= 65]}   # (the larger S add seconds, not answers)
    for name, cases in lists.items():
        caught = {v: [] for v in hmm_ref.CHUNK_VARIANTS}
        for case in cases:
            _, back, states = hmm_ref.viterbi(*hmm_ref.viterbi_operands(case))
            assert np.array_equal(hmm_ref.walk_back(back, int(states[-1])), states)
            for v in hmm_ref.CHUNK_VARIANTS:
                if not np.array_equal(hmm_ref.walk_back(back, int(states[-1]), v), states):
                    caught[v].append(hmm_ref.case_id(case))
        for v in hmm_ref.CHUNK_VARIANTS:
            print(f"{v}, {name}: caught by {len(caught[v])} of {len(cases)} cases, first {caught[v][:3]}")
            got[(v, name)] = bool(caught[v])
    edge = pyin_ref.edge_cases()
    for name, cases in (("before", [c for c in pyin_ref.b_cases() if c["kind"] != "nan"]), ("edge", edge),
                        ("edge without corners", [c for c in edge if c["kind"] != "corners"])):
        caught = []
        for case in cases:
            ops = dc.pyin_operands(case)
            with np.errstate(invalid="ignore"):
                if not all(np.array_equal(a, b, equal_nan=True) for a, b in zip(pyin_ref.viterbi(*ops), wrong_pyin(SHORT_REACH)(*ops))):
                    caught.append(pyin_ref.b_case_id(case))
        print(f"short_reach, {name}: caught by {len(caught)} of {len(cases)} cases, first {caught[:3]}")
        got[("short_reach", name)] = bool(caught)
    assert got == CAUGHT_BY


# ------------------------------------------------------------------------------------------------ the strategies
def in_hmm_range(c, kinds):
    return 1 <= c["S"] <= hmm_ref.MAX_STATES and 1 <= c["T"] <= 300 and c["kind"] in kinds and 0 <= c["seed"] <= 1 << 16


def in_pyin_range(c):
    return (1 <= c["n_bins"] <= pyin_ref.MAX_BINS and 0 <= c["width"] <= pyin_ref.MAX_WIDTH and 1 <= c["n_frames"] <= 300
            and c["kind"] in pyin_ref.B_KINDS and not (c["kind"] == "nan" and c["n_frames"] < 3))


def in_bar_range(c):
    iv, beats = c["intervals"], c["beats"]
    return (1 <= len(iv) <= 6 and all(a < b for a, b in zip(iv, iv[1:])) and 1 <= iv[0] and iv[-1] <= 24 and 1 <= len(beats) <= 3
            and all(1 <= b <= 8 for b in beats) and 1 <= c["T"] <= 3 * iv[-1] + 5
            and bar_ref.lds_bytes(len(iv), max(beats), iv[-1]) > 0)   # a refusal inside the property would hide a case: none may be drawn


def test_the_explicit_examples_pin_the_coverage():
    """What hypothesis draws depends on the process (sweep's docstring), so the coverage every property needs is carried by explicit
    examples, which lie inside the ranges of their strategies: every kind, S and P below, at and above 64, the unroll and stride edges,
    W either side of the scan's clamp, the limits; for the bar model (at most 48 lanes: 64 is no lane count it can straddle) the most
    lanes and slots of the range, a clip shorter than the longest interval and one that wraps the ring more than twice."""
    for kinds in (hmm_ref.VITERBI_KINDS, hmm_ref.POSTERIOR_KINDS):
        ex = dc.hmm_examples(kinds)
        assert all(in_hmm_range(c, kinds) for c in ex) and {c["kind"] for c in ex} == set(kinds)
        assert {c["S"] for c in ex} == set(hmm_ref.SWEEP_STATES) >= {3, 4, 5, 63, 64, 65, 127, 128} and {1, 300} <= {c["T"] for c in ex}
    ex = dc.pyin_examples()
    assert all(in_pyin_range(c) for c in ex) and {c["kind"] for c in ex} == set(pyin_ref.B_KINDS)
    assert {1, 63, 64, 65, 127, 128, 129, pyin_ref.MAX_BINS} <= {c["n_bins"] for c in ex} and {0, pyin_ref.MAX_WIDTH} <= {c["width"] for c in ex}
    for relation in (lambda c: c["width"] == c["n_bins"] - 2, lambda c: c["width"] == c["n_bins"] - 1, lambda c: c["width"] >= c["n_bins"]):
        assert any(relation(c) for c in ex)
    ex = dc.bar_examples()
    assert all(in_bar_range(c) for c in ex)
    assert max(len(c["intervals"]) * max(c["beats"]) for c in ex) == 48 and any(c["intervals"][-1] == 24 and len(c["intervals"]) == 6 for c in ex)
    assert any(c["T"] <= c["intervals"][-1] for c in ex) and any(c["T"] > 2 * c["intervals"][-1] for c in ex)
    assert any(c["T"] == 1 for c in ex) and any(len(c["beats"]) == 3 for c in ex)
    assert bar_ref.lds_bytes(6, 8, 24) > 0   # the largest model of the range


def test_the_strategies_stay_inside_their_ranges():
    """Asserted of every draw, so true of whatever a device run draws: the ranges, no NaN kind without a frame before its NaN, no bar
    model that the entry would refuse.  The explicit examples come first and the draws follow."""
    sweeps = {"viterbi": (dc.hmm_strategy(hmm_ref.VITERBI_KINDS), dc.hmm_examples(hmm_ref.VITERBI_KINDS), lambda c: in_hmm_range(c, hmm_ref.VITERBI_KINDS)),
              "posterior": (dc.hmm_strategy(hmm_ref.POSTERIOR_KINDS), dc.hmm_examples(hmm_ref.POSTERIOR_KINDS), lambda c: in_hmm_range(c, hmm_ref.POSTERIOR_KINDS)),
              "pyin": (dc.pyin_strategy(), dc.pyin_examples(), in_pyin_range), "bar": (dc.bar_strategy(), dc.bar_examples(), in_bar_range)}
    for name, (strategy, examples, in_range) in sweeps.items():
        seen = dc.sweep(strategy, lambda case: None, examples)
        print(f"{name}: {len(examples)} explicit examples, {len(seen) - len(examples)} draws, first draw {seen[len(examples)]}")
        assert seen[:len(examples)] == examples and len(seen) == len(examples) + dc.MAX_EXAMPLES, name
        assert all(in_range(c) for c in seen), name
        many = dc.sweep(strategy, lambda case: None, max_examples=400)
        assert len(many) >= 200 and all(in_range(c) for c in many), name


# ------------------------------------------------------------------------------------------------ the size function
def test_bar_lds_bytes_agrees_with_its_restatement(built_lib):
    from maua_stylegan2_amd import _lib

    lib = _lib.load()
    rng = np.random.default_rng(5)
    shapes = [(int(rng.integers(0, bar_ref.MAX_TEMPI + 3)), int(rng.integers(0, bar_ref.MAX_BEATS + 3)), int(rng.integers(0, bar_ref.MAX_INTERVAL + 3)))
              for _ in range(300)]
    shapes += [(int(rng.integers(1, 40)), int(rng.integers(1, 9)), int(rng.integers(1, 120))) for _ in range(300)]   # round the 160 KiB plan
    for K in (1, bar_ref.MAX_TEMPI, bar_ref.MAX_TEMPI + 1):      # every limit and limit + 1, crossed
        for B in (1, bar_ref.MAX_BEATS, bar_ref.MAX_BEATS + 1):
            for I in (1, bar_ref.MAX_INTERVAL, bar_ref.MAX_INTERVAL + 1):
                shapes.append((K, B, I))
    # the LDS plan itself at its limit: the largest ring that fits for a few (K, B), and one slot more
    for K, B in ((1, 1), (2, 8), (34, 4), (100, 1), (40, 8), (128, 8)):
        lanes = K * B
        fits = (bar_ref.LDS_LIMIT // 8 - K * (K | 1) - 2 * lanes) // lanes
        shapes += [(K, B, fits), (K, B, fits + 1)]
        if 1 <= fits < bar_ref.MAX_INTERVAL:
            assert bar_ref.lds_bytes(K, B, fits) > 0 and bar_ref.lds_bytes(K, B, fits + 1) == 0, (K, B, fits)
    n_fit = 0
    for K, B, I in shapes:
        got = lib.maua_bar_lds_bytes(K, B, I)
        assert got == bar_ref.lds_bytes(K, B, I), (K, B, I, got)
        n_fit += got > 0
    print(f"{len(shapes)} shapes, {n_fit} of them fit")
    assert n_fit >= 100 and len(shapes) - n_fit >= 100
