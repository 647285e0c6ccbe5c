"""GPU: the four sequence decoders (csrc/hmm.hip, csrc/pyin.hip, csrc/bar.hip) on random shapes and against each other.

Random shapes (hypothesis, the strategies of tests/decoder_cases.py: derandomised, no example database, no shrinking; explicit
examples pin every kind, both sides of 64 and the edge values, whatever is drawn): every case goes through the C ABI between red
zones, twice, and is compared bit for bit with the numpy restatement of its entry — the entries are defined to the bit, so a random
shape needs no tolerance, only one run of a restatement.

Identities (the cases of tests/decoder_cases.py, all on integer-valued operands, so equality is exact): pYIN against the dense
decoder on the written-out 2 P-state model and the bar-pointer decoder against the dense decoder through bar_ref.expand, both
sides on the device; an integer offset per frame changes no decision and adds its sum to the score; a prefix of the frames
gives a prefix of the back pointers.  tests/test_decoders_host.py shows that the same identities hold between the restatements and
that a wrong decoder breaks them, so a failure here implicates a kernel.

A positive return code of an entry or a device error ends the session (pytest.exit): nothing is started on a device that has
reported a HIP error, the one replay hypothesis makes of a failing example included (a plain mismatch is replayed once).  The
identities put the same kernel on both sides of C.3 and C.4, so a defect of the walk back alone passes them: the device's guard
against that is hmm_ref.EDGE_CASES in tests/test_hmm_gpu.py.  Launch and compare helpers are those of tests/test_hmm_gpu.py,
test_pyin_gpu.py and test_bar_gpu.py."""
import time

import numpy as np
import pytest
import torch

import bar_ref
import decoder_cases as dc
import hmm_ref
import pyin_ref
import test_bar_gpu as bg
import test_hmm_gpu as hg
import test_pyin_gpu as pg
from redzone import Guard

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

FATAL = []   # the first HIP error of the session: every later device call ends the session again instead of launching


def launched(rc, what):
    if rc > 0:
        FATAL.append(f"{what}: HIP error {rc}")
        pytest.exit(FATAL[0], returncode=3)
    assert rc == 0, f"{what}: refused with {rc}"


def on_device(gpu, what, body):
    """``body(guard)`` -> [(output names to check, host copies), ...] of two identical launches; red zones intact, every element written,
    the two runs equal in every bit."""
    if FATAL:
        pytest.exit(FATAL[0], returncode=3)
    try:
        with torch.cuda.device(gpu):
            g = Guard(gpu)
            names, runs = body(g)
            g.check(written=names, nonfinite_ok=names)
    except RuntimeError as err:   # (what torch raises for a HIP error; a failed comparison is an AssertionError)
        FATAL.append(f"{what}: {err}")
        pytest.exit(FATAL[0], returncode=3)
    for key in runs[0]:
        assert hmm_ref.same_bits(runs[0][key], runs[1][key]), f"{what}: {key}: two runs differ"
    return runs[0]


# ------------------------------------------------------------------------------------------------ the entries as callables
def dev_hmm(gpu, logobs, log_trans, log_init):
    case = dict(T=logobs.shape[0], S=logobs.shape[1])
    what = f"maua_hmm_viterbi_f64 S={case['S']} T={case['T']}"

    def body(g):
        ops = hg.operands(g, (logobs, log_trans, log_init))
        runs = []
        for tag in ("a", "b"):
            out = hg.v_windows(g, case, tag)
            launched(hg.v_call(ops, case, out), what)
            runs.append(out)
        torch.cuda.synchronize(gpu)
        return [f"{k}.{tag}" for tag in ("a", "b") for k in hg.V_OUT], [hg.v_host(out, case) for out in runs]

    got = on_device(gpu, what, body)
    return got["delta_last"], got["backptr"], got["states"]


def dev_posterior(gpu, obs, trans, init):
    case = dict(T=obs.shape[0], S=obs.shape[1])
    what = f"maua_hmm_posterior_f64 S={case['S']} T={case['T']}"

    def body(g):
        ops = hg.operands(g, (obs, trans, init))
        runs = []
        for tag in ("a", "b"):
            out = hg.p_windows(g, case, tag)
            launched(hg.p_call(ops, case, out), what)
            runs.append(out)
        torch.cuda.synchronize(gpu)
        return [f"{k}.{tag}" for tag in ("a", "b") for k in hg.P_OUT], [hg.p_host(out) for out in runs]

    return on_device(gpu, what, body)


def dev_pyin(gpu, lov, lou, width, log_tri, log_norm, log_init, log_stay, log_switch):
    case = dict(n_frames=lov.shape[0], n_bins=lov.shape[1], width=width)
    what = "maua_pyin_viterbi_f64 P={n_bins} W={width} T={n_frames}".format(**case)

    def body(g):
        ops = (g.inp(lov, "lov"), g.inp(lou, "lou"), g.inp(log_tri, "tri", torch.float64), g.inp(log_norm, "norm", torch.float64),
               (log_init, log_stay, log_switch))
        runs = []
        for tag in ("a", "b"):
            out = pg.b_windows(g, case, tag)
            launched(pg.b_call(*ops, case, out), what)
            runs.append(out)
        torch.cuda.synchronize(gpu)
        return [f"{k}.{tag}" for tag in ("a", "b") for k in pg.B_OUT], [pg.b_host(out, case) for out in runs]

    got = on_device(gpu, what, body)
    return got["delta_last"], got["backptr"], got["states"]


def dev_bar(gpu, logobs, interval, width, log_change, beats):
    what = f"maua_bar_viterbi_f64 intervals={list(map(int, interval))} beats={tuple(beats)} T={len(logobs)}"

    def body(g):
        d_lo, d_lc = g.inp(logobs, "logobs"), g.inp(log_change, "log_change", torch.float64)
        runs = []
        for tag in ("a", "b"):
            out = bg.windows(g, len(logobs), len(interval), beats, tag)
            launched(bg.call(d_lo, d_lc, interval, width, beats, len(logobs), out), what)
            runs.append(out)
        torch.cuda.synchronize(gpu)
        return [f"{k}.{tag}" for tag in ("a", "b") for k in bg.OUT], [{k: out[k].cpu().numpy() for k in bg.OUT} for out in runs]

    got = on_device(gpu, what, body)
    return got["score"], got["path"]


def bound(fn, gpu):
    return lambda *args: fn(gpu, *args)


# ------------------------------------------------------------------------------------------------ random shapes
def run_sweep(name, strategy, examples, body, side=None, kinds=None):
    """The explicit examples and MAX_EXAMPLES draws through ``body``.  What hypothesis draws differs from process to process, so the
    coverage is asserted on what actually ran here: every operand kind, and ``side`` (S, P) on both sides of 64."""
    start = time.perf_counter()
    seen = dc.sweep(strategy, body, examples)
    print(f"{name}: {len(examples)} explicit examples and {len(seen) - len(examples)} draws in {time.perf_counter() - start:.1f} s")
    assert seen[:len(examples)] == list(examples)
    assert len(seen) - len(examples) >= dc.MAX_EXAMPLES // 2   # (hypothesis stops early only when a strategy runs out of distinct draws)
    if side is not None:
        assert any(side(c) < 64 for c in seen) and any(side(c) == 64 for c in seen) and any(side(c) > 64 for c in seen)
    if kinds is not None:
        assert {c["kind"] for c in seen} == set(kinds)
    return seen


def test_hmm_viterbi_random_shapes(gpu):
    def body(case):
        arrays = hmm_ref.viterbi_operands(case)
        delta, back, states = dev_hmm(gpu, *arrays)
        hg.assert_viterbi(dict(delta_last=delta, backptr=back, states=states), hmm_ref.viterbi(*arrays), hmm_ref.case_id(case))

    run_sweep("maua_hmm_viterbi_f64", dc.hmm_strategy(hmm_ref.VITERBI_KINDS), dc.hmm_examples(hmm_ref.VITERBI_KINDS), body,
              side=lambda c: c["S"], kinds=hmm_ref.VITERBI_KINDS)


def test_hmm_posterior_random_shapes(gpu):
    def body(case):
        arrays = hmm_ref.posterior_operands(case)
        hg.assert_posterior(dev_posterior(gpu, *arrays), hmm_ref.posterior(*arrays), hmm_ref.case_id(case), exact=False)

    run_sweep("maua_hmm_posterior_f64", dc.hmm_strategy(hmm_ref.POSTERIOR_KINDS), dc.hmm_examples(hmm_ref.POSTERIOR_KINDS), body,
              side=lambda c: c["S"], kinds=hmm_ref.POSTERIOR_KINDS)


def test_pyin_viterbi_random_shapes(gpu):
    def body(case):
        ops = dc.pyin_operands(case)
        delta, back, states = dev_pyin(gpu, *ops)
        pg.assert_b_equal(dict(delta_last=delta, backptr=back, states=states), pyin_ref.viterbi(*ops), pyin_ref.b_case_id(case))

    seen = run_sweep("maua_pyin_viterbi_f64", dc.pyin_strategy(), dc.pyin_examples(), body, side=lambda c: c["n_bins"], kinds=pyin_ref.B_KINDS)
    for relation in (lambda c: c["width"] == c["n_bins"] - 2, lambda c: c["width"] == c["n_bins"] - 1, lambda c: c["width"] >= c["n_bins"]):
        assert any(relation(c) for c in seen)   # either side of the scan's clamp


def test_bar_viterbi_random_shapes(gpu):
    def body(case):
        ops = dc.bar_operands(case)
        score, path = dev_bar(gpu, *ops, case["beats"])
        want_score, want_path = bar_ref.decode(*ops, case["beats"])
        assert bar_ref.same_bits(score, want_score), f"{case}: score {score.tolist()} for {want_score.tolist()}"
        assert bar_ref.same_bits(path, want_path), f"{case}: {int((path != want_path).any(-1).sum())} path frames differ"

    seen = run_sweep("maua_bar_viterbi_f64", dc.bar_strategy(), dc.bar_examples(), body)
    # (at most 48 lanes: 64 is no lane count this range can straddle; its edges are the ring's)
    assert any(c["T"] <= c["intervals"][-1] for c in seen) and any(c["T"] > 2 * c["intervals"][-1] for c in seen)
    assert max(len(c["intervals"]) * max(c["beats"]) for c in seen) == 48 and any(len(c["beats"]) == 3 for c in seen)


# ------------------------------------------------------------------------------------------------ identities
@pytest.mark.parametrize("case", dc.PYIN_DENSE, ids=str)
def test_pyin_against_the_dense_decoder(gpu, case):
    assert dc.check_pyin_dense(case, bound(dev_pyin, gpu), bound(dev_hmm, gpu)) == []


@pytest.mark.parametrize("case", dc.BAR_DENSE, ids=str)
def test_bar_pointer_against_the_dense_decoder(gpu, case):
    assert dc.check_bar_dense(case, bound(dev_bar, gpu), bound(dev_hmm, gpu)) == []


@pytest.mark.parametrize("case", dc.HMM_SHIFT, ids=str)
def test_hmm_shift(gpu, case):
    assert dc.check_hmm_shift(case, bound(dev_hmm, gpu), bound(dev_hmm, gpu)) == []


@pytest.mark.parametrize("case", dc.PYIN_SHIFT, ids=str)
def test_pyin_shift(gpu, case):
    assert dc.check_pyin_shift(case, bound(dev_pyin, gpu), bound(dev_pyin, gpu)) == []


@pytest.mark.parametrize("case", dc.BAR_SHIFT, ids=str)
def test_bar_shift(gpu, case):
    assert dc.check_bar_shift(case, bound(dev_bar, gpu), bound(dev_bar, gpu)) == []


@pytest.mark.parametrize("case", dc.HMM_PREFIX, ids=str)
def test_hmm_prefix(gpu, case):
    assert dc.check_hmm_prefix(case, bound(dev_hmm, gpu), bound(dev_hmm, gpu)) == []


@pytest.mark.parametrize("case", dc.PYIN_PREFIX, ids=str)
def test_pyin_prefix(gpu, case):
    assert dc.check_pyin_prefix(case, bound(dev_pyin, gpu), bound(dev_pyin, gpu)) == []
