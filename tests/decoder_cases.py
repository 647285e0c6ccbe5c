"""What tests/test_decoders_property_gpu.py (on the device) and tests/test_decoders_host.py (between the restatements) share: the
hypothesis strategies of the four sequence decoders (csrc/hmm.hip, csrc/pyin.hip, csrc/bar.hip) with their explicit examples and the
one function that runs them, and the identities that relate two entries to each other or an entry to itself, with their cases.

The identities are written against callables, never against a device:
    hmm(logobs [T, S] fp32, log_trans, log_init)                              -> (delta_last, backptr [T, S], states)
    pyin(lov [T, P] fp32, lou [T] fp32, W, log_tri, log_norm, init, stay, sw) -> (delta_last, backptr [T, 2 P], states)
    bar(logobs [T, 3] fp32, interval, width, log_change, beats_per_bar)       -> (score [n_models], path [n_models, T, 3])
Every identity uses integer-valued operands: each sum is exact, so two orders of the same additions give the same bits and there is no
tolerance anywhere.  A check returns its complaints, an empty list for agreement."""
import numpy as np
from hypothesis import HealthCheck, Phase, example, given, settings, strategies as st

import bar_ref
import hmm_ref
import pyin_ref

# the settings of every property test of the suite (tests/test_property_gpu.py takes them from here)
COMMON = dict(deadline=None, derandomize=True, suppress_health_check=[HealthCheck.function_scoped_fixture, HealthCheck.too_slow])
MAX_EXAMPLES = 40
# No example database and no shrinking: a failing example is reported as drawn.  hypothesis still replays a failing example once for
# its report, so a plain mismatch launches its kernel a second time; after a HIP error the device test launches nothing more, the
# replay included (the FATAL list of tests/test_decoders_property_gpu.py).
SWEEP = dict(database=None, phases=[Phase.explicit, Phase.generate], **COMMON)


def sweep(strategy, body, examples=(), max_examples=MAX_EXAMPLES):
    """``body(case)`` over the explicit ``examples`` and then ``max_examples`` derandomised draws of ``strategy``; returns every case
    in the order run.  What is drawn is NOT the same from one process to another: hypothesis seeds a derandomised run from the wrapped
    function's source but also feeds its generators with constants it finds in whatever project modules are loaded.  So nothing may
    lean on a particular draw: the coverage a property needs — every kind, both sides of 64, the edge values — is pinned by the explicit
    examples, and the draws add breadth on top."""
    seen = []

    def run(case):
        seen.append(case)
        body(case)

    run = given(case=strategy)(run)
    for case in reversed(list(examples)):
        run = example(case=case)(run)
    settings(max_examples=max_examples, **SWEEP)(run)()
    return seen


# ------------------------------------------------------------------------------------------------ strategies
SEEDS = st.integers(0, 1 << 16)
PYIN_EDGE_BINS = (1, 2, 63, 64, 65, 127, 128, 129, 1023, 1024)
PYIN_EDGE_WIDTHS = (0, 1, 62, 63, 64, 65, 126, 127, 128)


def hmm_strategy(kinds):
    """S in 1 .. 128 with the wave and unroll edges mixed in, T in 1 .. 300: a case of hmm_ref.viterbi_operands / posterior_operands."""
    return st.fixed_dictionaries(dict(S=st.one_of(st.integers(1, hmm_ref.MAX_STATES), st.sampled_from(hmm_ref.SWEEP_STATES)),
                                      T=st.integers(1, 300), kind=st.sampled_from(kinds), seed=SEEDS))


@st.composite
def pyin_strategy(draw):
    """P in 1 .. 1024 and W in 0 .. 128 with their edge values mixed in, T in 1 .. 300 (from 3 for the NaN kind, which puts its NaN in
    frame T // 2 and needs a frame before it): a case of pyin_ref.make_logobs / b_constants."""
    kind = draw(st.sampled_from(pyin_ref.B_KINDS))
    return dict(n_bins=draw(st.one_of(st.integers(1, pyin_ref.MAX_BINS), st.sampled_from(PYIN_EDGE_BINS))),
                width=draw(st.one_of(st.integers(0, pyin_ref.MAX_WIDTH), st.sampled_from(PYIN_EDGE_WIDTHS))),
                n_frames=draw(st.integers(3 if kind == "nan" else 1, 300)), kind=kind, seed=draw(SEEDS))


@st.composite
def bar_strategy(draw):
    """One to six strictly ascending intervals from 1 .. 24, one to three bar lengths from 1 .. 8, T in 1 .. 3 max(interval) + 5 (the
    ring wraps up to three times): at most 48 lanes of 24 slots, which one CU always holds."""
    intervals = sorted(draw(st.lists(st.integers(1, 24), min_size=1, max_size=6, unique=True)))
    beats = tuple(draw(st.lists(st.integers(1, 8), min_size=1, max_size=3)))
    return dict(intervals=intervals, beats=beats, T=draw(st.integers(1, 3 * intervals[-1] + 5)), seed=draw(SEEDS))


def pyin_operands(case):
    lov, lou = pyin_ref.make_logobs(case)
    return (lov, lou, case["width"]) + tuple(pyin_ref.b_constants(case))


def bar_operands(case):
    return bar_ref.random_operands(case["intervals"], case["T"], case["seed"])


# Explicit examples: what a property must meet whatever is drawn.
def hmm_examples(kinds):
    """Every S of hmm_ref.SWEEP_STATES (both sides of 64, the unroll remainder, the S | 1 stride), every kind, T from 1 to 300."""
    frames = (1, 2, 3, 64, 65, 127, 128, 257, 299, 300)
    return [dict(S=S, T=frames[n], kind=kinds[n % len(kinds)], seed=n) for n, S in enumerate(hmm_ref.SWEEP_STATES)]


def pyin_examples():
    """The edge values of P and W either side of the clamp reach = min(W, P - 1) and of 64, the limits of both, every kind."""
    shapes = ((1, 0, 1), (2, 1, 2), (63, 62, 3), (64, 64, 5), (65, 63, 64), (127, 128, 9), (128, 127, 300), (129, 128, 4), (1023, 128, 3), (1024, 0, 7))
    cases = [dict(n_bins=P, width=W, n_frames=T, kind=pyin_ref.B_KINDS[n % len(pyin_ref.B_KINDS)], seed=n) for n, (P, W, T) in enumerate(shapes)]
    return [dict(c, n_frames=max(c["n_frames"], 3)) if c["kind"] == "nan" else c for c in cases]


def bar_examples():
    """One lane and one frame; the most lanes and slots of the range (48 x 24); clips shorter than the longest interval and ones that
    wrap the ring more than twice; three bar lengths in one launch."""
    return [dict(intervals=[1], beats=(1,), T=1, seed=0), dict(intervals=[24], beats=(8,), T=77, seed=1),
            dict(intervals=[1, 2, 3, 4, 5, 24], beats=(8, 1, 3), T=20, seed=2), dict(intervals=[2, 3], beats=(2, 2), T=14, seed=3),
            dict(intervals=[19, 20, 21, 22, 23, 24], beats=(8,), T=77, seed=4), dict(intervals=[7, 11], beats=(5, 3, 4), T=11, seed=5)]


# ------------------------------------------------------------------------------------------------ the cases of the identities
# (P, W, T), 2 P <= 128 states: W = 0, W = P - 1, W >= P, P = 1, P = 64 and T = 1 are all here
PYIN_DENSE = [(1, 0, 1), (1, 3, 5), (2, 1, 7), (5, 0, 9), (7, 6, 12), (8, 20, 6), (33, 5, 1), (63, 62, 3), (64, 0, 3), (64, 63, 4), (64, 70, 5),
              (31, 128, 8)]
# (intervals, B, T), sum(interval) B <= 128 states
BAR_DENSE = [([1], 1, 4), ([2, 3], 2, 1), ([2, 3], 2, 40), ([1, 2, 4], 3, 30), ([3, 4, 5, 7], 3, 97), ([3, 4, 5, 7], 6, 33), ([5], 8, 23), ([4, 9], 4, 64),
             ([6, 7, 8], 5, 50), ([1, 2, 3, 4, 5, 6], 6, 41), ([16], 8, 70), ([2, 3, 5, 11], 6, 2), ([24], 5, 77)]
HMM_SHIFT = [(1, 1), (5, 40), (64, 257), (128, 33), (3, 1025), (65, 2049)]      # (S, T): one chunk of the walk back, two, and three
PYIN_SHIFT = [(1, 0, 1), (5, 2, 30), (64, 63, 40), (129, 128, 20), (602, 50, 12)]  # (P, W, T)
BAR_SHIFT = [([1], (1,), 5), ([2, 3], (2,), 40), ([3, 4, 5, 7], (3, 4), 97), ([5, 6, 9], (1, 8), 10), ([2, 11, 24], (3,), 77)]
HMM_PREFIX = [(6, 1100, (1, 2, 1023, 1024, 1025)), (128, 40, (7, 39))]          # (S, T, the T' decoded on their own)
PYIN_PREFIX = [(65, 64, 30, (1, 2, 17)), (200, 10, 12, (5, 11))]                # (P, W, T, T')


def _bits(a, b):
    return hmm_ref.same_bits(np.asarray(a, np.float64), np.asarray(b, np.float64))


def pyin_integer_operands(P, W, T, seed):
    lov, lou = pyin_ref.make_logobs(dict(n_bins=P, width=W, n_frames=T, kind="integer", seed=seed))
    return (lov, lou, W) + tuple(pyin_ref.integer_constants(P, W))


def bar_integer_operands(intervals, T, seed):
    return bar_ref.random_operands(intervals, T, seed, matrix="integer", obs="integer")


def _offsets(T, seed):
    return np.random.default_rng(seed).integers(-3, 4, T).astype(np.float32)


def check_pyin_dense(case, pyin, hmm):
    """C.1: the pYIN decoder against the dense decoder on the written-out 2 P-state model (pyin_ref.expand).  The tie rules coincide:
    both take the first maximum in ascending source order, and pYIN prefers the voiced source on a tie."""
    P, W, T = case
    ops = pyin_integer_operands(P, W, T, 100 + P + W + T)
    delta, back, states = pyin(*ops)
    lt, li = pyin_ref.expand(P, W, *ops[3:])
    d_delta, d_back, d_states = hmm(pyin_ref.dense_observations(ops[0], ops[1]), lt, li)
    bad = []
    if not _bits(delta, d_delta):
        bad.append(f"pyin-dense {case}: delta_last")
    if not np.array_equal(np.asarray(states, np.int64), np.asarray(d_states, np.int64)):
        bad.append(f"pyin-dense {case}: states")
    if not np.array_equal(np.asarray(back, np.int64), np.asarray(d_back, np.int64)):   # uint16 against uint8
        bad.append(f"pyin-dense {case}: backptr")
    return bad


def check_bar_dense(case, bar, hmm):
    """C.2: the bar-pointer decoder against the dense decoder on the model with every state written out (bar_ref.expand)."""
    intervals, B, T = case
    lo, I, W, lc = bar_integer_operands(intervals, T, 200 + B + T)
    score, path = bar(lo, I, W, lc, (B,))
    lt, li, column, table = bar_ref.expand(I, W, lc, B)
    assert len(table) <= hmm_ref.MAX_STATES
    delta, _, states = hmm(np.ascontiguousarray(lo[:, column]), lt, li)
    bad = []
    if not _bits(score[0], np.max(delta)):
        bad.append(f"bar-dense {case}: score {score[0]!r} for {np.max(delta)!r}")
    if not np.array_equal(table[np.asarray(states, np.int64)], np.asarray(path)[0]):
        bad.append(f"bar-dense {case}: path")
    return bad


def check_hmm_shift(case, hmm, other):
    """C.3: an integer c_t added to every state's observation of frame t leaves backptr and states as they are and adds sum(c_t) to
    delta_last exactly.  ``hmm`` decodes the plain operands, ``other`` the shifted ones."""
    S, T = case
    lo, lt, li = hmm_ref.viterbi_operands(dict(S=S, T=T, kind="integer", seed=300 + S + T))
    c = _offsets(T, 301 + S + T)
    base, moved = hmm(lo, lt, li), other(lo + c[:, None], lt, li)
    return _shift_complaints(f"hmm-shift {case}", base, moved, c)


def check_pyin_shift(case, pyin, other):
    P, W, T = case
    ops = pyin_integer_operands(P, W, T, 400 + P + W + T)
    c = _offsets(T, 401 + P + W + T)
    base, moved = pyin(*ops), other(ops[0] + c[:, None], ops[1] + c, *ops[2:])
    return _shift_complaints(f"pyin-shift {case}", base, moved, c)


def _shift_complaints(what, base, moved, c):
    bad = []
    if not _bits(np.asarray(base[0]) + float(c.astype(np.float64).sum()), moved[0]):
        bad.append(f"{what}: delta_last")
    if not np.array_equal(base[1], moved[1]):
        bad.append(f"{what}: backptr")
    if not np.array_equal(base[2], moved[2]):
        bad.append(f"{what}: states")
    return bad


def check_bar_shift(case, bar, other):
    intervals, beats, T = case
    lo, I, W, lc = bar_integer_operands(intervals, T, 500 + T)
    c = _offsets(T, 501 + T)
    base, moved = bar(lo, I, W, lc, beats), other(lo + c[:, None], I, W, lc, beats)
    bad = []
    if not _bits(np.asarray(base[0]) + float(c.astype(np.float64).sum()), moved[0]):
        bad.append(f"bar-shift {case}: score")
    if not np.array_equal(base[1], moved[1]):
        bad.append(f"bar-shift {case}: path")
    return bad


def check_hmm_prefix(case, hmm, other):
    """C.4: the forward pass is causal — the first T' frames decoded on their own (by ``other``) give the first T' rows of backptr."""
    S, T, prefixes = case
    lo, lt, li = hmm_ref.viterbi_operands(dict(S=S, T=T, kind="integer", seed=600 + S + T))
    full = hmm(lo, lt, li)
    return [f"hmm-prefix {(S, T, n)}: backptr" for n in prefixes if not np.array_equal(other(lo[:n], lt, li)[1], full[1][:n])]


def check_pyin_prefix(case, pyin, other):
    P, W, T, prefixes = case
    ops = pyin_integer_operands(P, W, T, 700 + P + W + T)
    full = pyin(*ops)
    return [f"pyin-prefix {(P, W, T, n)}: backptr" for n in prefixes if not np.array_equal(other(ops[0][:n], ops[1][:n], *ops[2:])[1], full[1][:n])]


def identity_complaints(hmm, pyin, bar, hmm_other=None, pyin_other=None, bar_other=None):
    """Every identity over every case.  The ``*_other`` decoders (default: the same ones) stand on ONE side of an identity: the dense
    side of C.1 and C.2 for hmm, the pYIN / bar side of C.1 / C.2, and the second decode of C.3 and C.4."""
    hmm_other, pyin_other, bar_other = hmm_other or hmm, pyin_other or pyin, bar_other or bar
    bad = []
    for case in PYIN_DENSE:
        bad += check_pyin_dense(case, pyin_other, hmm_other)
    for case in BAR_DENSE:
        bad += check_bar_dense(case, bar_other, hmm_other)
    for case in HMM_SHIFT:
        bad += check_hmm_shift(case, hmm, hmm_other)
    for case in PYIN_SHIFT:
        bad += check_pyin_shift(case, pyin, pyin_other)
    for case in BAR_SHIFT:
        bad += check_bar_shift(case, bar, bar_other)
    for case in HMM_PREFIX:
        bad += check_hmm_prefix(case, hmm, hmm_other)
    for case in PYIN_PREFIX:
        bad += check_pyin_prefix(case, pyin, pyin_other)
    return bad
