"""GPU: the two hidden-Markov-model entries (csrc/hmm.hip) called through the C ABI between red zones, over the case lists of
tests/hmm_ref.py: S in {1, 2, 25, 64, 97, 128} x T in {1, 2, 3, 257, 2000} x every operand kind — one lane and one frame, the last
partial wave (97), the padded LDS stride and the byte back pointer at their limits (128), more frames than one chunk of the walk back
(2000) — and over hmm_ref.EDGE_CASES, the (S, T) pairs on the edges of that chunking (T = 1023 .. 2049) and of the waves, the stride and
the unroll (S = 3 .. 128).  Every output of both entries bit for bit against the float64 restatement, two runs identical.  The one exception is written
down in hmm_ref.same_bits_or_nan: where the posterior's definition yields a NaN (a NaN operand, an all-zero frame) the positions of
the NaNs are compared, not their payload.  Every case ends with Guard.check: red zones intact, every output element written."""
import numpy as np
import pytest
import torch

import hmm_ref as q
from maua_stylegan2_amd import _lib
from redzone import Guard

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

EINVAL = -22
V_OUT = ("delta_last", "backptr", "states")
P_OUT = ("gamma", "scale")


def v_windows(g, case, tag):
    T, S = case["T"], case["S"]
    return {"delta_last": g.out((S,), f"delta_last.{tag}", torch.float64), "backptr": g.out((T * S,), f"backptr.{tag}", torch.uint8),
            "states": g.out((T,), f"states.{tag}", torch.int32)}


def p_windows(g, case, tag):
    T, S = case["T"], case["S"]
    return {"gamma": g.out((T, S), f"gamma.{tag}", torch.float64), "scale": g.out((T,), f"scale.{tag}", torch.float64)}


def operands(g, arrays):
    frames, matrix, vector = arrays
    return g.inp(frames, "frames"), g.inp(matrix, "matrix", torch.float64), g.inp(vector, "vector", torch.float64)


def v_call(ops, case, out, **override):
    a = dict(case, **override)
    ptr = lambda name, t: None if a.get("null") == name else t.data_ptr()  # noqa: E731
    return _lib.load().maua_hmm_viterbi_f64(ptr("frames", ops[0]), ptr("matrix", ops[1]), ptr("vector", ops[2]), a["T"], a["S"],
                                            ptr("delta_last", out["delta_last"]), ptr("backptr", out["backptr"]), ptr("states", out["states"]),
                                            _lib.stream_ptr(ops[0].device))


def p_call(ops, case, out, **override):
    a = dict(case, **override)
    ptr = lambda name, t: None if a.get("null") == name else t.data_ptr()  # noqa: E731
    return _lib.load().maua_hmm_posterior_f64(ptr("frames", ops[0]), ptr("matrix", ops[1]), ptr("vector", ops[2]), a["T"], a["S"],
                                              ptr("gamma", out["gamma"]), ptr("scale", out["scale"]), _lib.stream_ptr(ops[0].device))


def v_host(out, case):
    return {"delta_last": out["delta_last"].cpu().numpy(), "states": out["states"].cpu().numpy(),
            "backptr": out["backptr"].cpu().numpy().reshape(case["T"], case["S"])}


def p_host(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def run_twice(gpu, case, arrays, windows, call, names):
    with torch.cuda.device(gpu):
        g = Guard(gpu)
        ops = operands(g, arrays)
        runs = []
        for tag in ("a", "b"):
            out = windows(g, case, tag)
            assert call(ops, case, out) == 0
            runs.append(out)
        g.check(written=[f"{k}.{tag}" for tag in ("a", "b") for k in names], nonfinite_ok=[f"{k}.{tag}" for tag in ("a", "b") for k in names])
    return runs


def assert_viterbi(got, ref, what):
    delta, back, states = ref
    assert q.same_bits(got["delta_last"], delta), f"{what}: delta_last"
    assert np.array_equal(got["backptr"], back), f"{what}: backptr differs in {int((got['backptr'] != back).sum())} elements"
    assert q.same_bits(got["states"], states), f"{what}: states"


def assert_posterior(got, ref, what, exact):
    same = q.same_bits if exact else q.same_bits_or_nan
    gamma, scale = ref
    assert same(got["scale"], scale), f"{what}: scale"
    assert same(got["gamma"], gamma), f"{what}: gamma differs in {int((got['gamma'] != gamma).sum())} elements"


@pytest.mark.parametrize("case", q.cases(q.VITERBI_KINDS), ids=q.case_id)
def test_viterbi_bit_for_bit(gpu, case):
    arrays = q.viterbi_operands(case)
    ref = q.viterbi(*arrays)
    a, b = (v_host(out, case) for out in run_twice(gpu, case, arrays, v_windows, v_call, V_OUT))
    for key in V_OUT:
        assert q.same_bits(a[key], b[key]), f"{key}: two runs differ"
    assert_viterbi(a, ref, q.case_id(case))


@pytest.mark.parametrize("case", q.cases(q.POSTERIOR_KINDS), ids=q.case_id)
def test_posterior_bit_for_bit(gpu, case):
    arrays = q.posterior_operands(case)
    ref = q.posterior(*arrays)
    a, b = (p_host(out) for out in run_twice(gpu, case, arrays, p_windows, p_call, P_OUT))
    for key in P_OUT:
        assert q.same_bits(a[key], b[key]), f"{key}: two runs differ"
    yields_nan = case["kind"] in ("nan", "zero_row")
    if not yields_nan:
        assert np.isfinite(ref[0]).all() and np.isfinite(ref[1]).all() and np.abs(ref[0].sum(1) - 1).max() < 1e-12
    assert_posterior(a, ref, q.case_id(case), exact=not yields_nan)


@pytest.mark.parametrize("case", q.edge_cases(q.EDGE_VITERBI_KINDS), ids=q.case_id)
def test_viterbi_chunk_and_wave_edges(gpu, case):
    """hmm_ref.EDGE_CASES: the walk back with an exactly full chunk, a last chunk of one row, two full chunks and two and a row, at
    the S either side of the second wave, of the S | 1 stride and of the unroll remainder."""
    test_viterbi_bit_for_bit(gpu, case)


@pytest.mark.parametrize("case", q.edge_cases(q.EDGE_POSTERIOR_KINDS), ids=q.case_id)
def test_posterior_parity_and_wave_edges(gpu, case):
    """The same (S, T) pairs through the posterior: both parities of T for the two buffers of its backward sweep."""
    test_posterior_bit_for_bit(gpu, case)


def test_viterbi_twenty_thousand_frames(gpu):
    """T = 20 000, S = 25 (a long track against the triads): twenty chunks of the walk back, delta four orders of magnitude from
    where it starts."""
    arrays = q.viterbi_operands(q.LONG_CASE)
    ref = q.viterbi(*arrays)
    a, _ = (v_host(out, q.LONG_CASE) for out in run_twice(gpu, q.LONG_CASE, arrays, v_windows, v_call, V_OUT))
    print(f"final delta {ref[0].max():.1f}, {len(np.unique(ref[2]))} states visited, {int((np.diff(ref[2]) != 0).sum())} changes")
    assert abs(ref[0].max()) > 1e4 and len(np.unique(ref[2])) == 25
    assert_viterbi(a, ref, "long")


def test_refusals_leave_the_outputs_untouched(gpu):
    case = dict(S=25, T=3, kind="random", seed=2)
    shapes = [dict(T=0), dict(T=-3), dict(T=(1 << 22) + 1), dict(S=0), dict(S=-1), dict(S=129)]
    with torch.cuda.device(gpu):
        g = Guard(gpu)
        v_ops = operands(g, q.viterbi_operands(case))
        p_ops = operands(g, q.posterior_operands(case))
        for i, kw in enumerate([dict(null=k) for k in ("frames", "matrix", "vector") + V_OUT] + shapes):
            out = v_windows(g, case, f"v{i}")
            assert v_call(v_ops, case, out, **kw) == EINVAL, kw
            assert all(g.untouched(f"{k}.v{i}") for k in V_OUT), kw
        for i, kw in enumerate([dict(null=k) for k in ("frames", "matrix", "vector") + P_OUT] + shapes):
            out = p_windows(g, case, f"p{i}")
            assert p_call(p_ops, case, out, **kw) == EINVAL, kw
            assert all(g.untouched(f"{k}.p{i}") for k in P_OUT), kw
        g.check()


def test_both_entries_are_capturable(gpu):
    """Captured into one hipGraph and replayed on new input in the same buffers: each replay equals the eager calls bit for bit (and
    the second one the restatement)."""
    case = dict(S=97, T=257, kind="random", seed=21)
    other = dict(case, seed=22)
    stream = torch.cuda.Stream(gpu)
    with torch.cuda.device(gpu):
        g = Guard(gpu)
        v_ops = operands(g, q.viterbi_operands(case))
        p_ops = operands(g, q.posterior_operands(case))
        v_cap, p_cap = v_windows(g, case, "graph"), p_windows(g, case, "graph")
        assert v_call(v_ops, case, v_cap) == 0 and p_call(p_ops, case, p_cap) == 0  # (a kernel's first launch sets its LDS attribute)
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            with _lib.HipGraph() as graph:
                rc_v = v_call(v_ops, case, v_cap)
                rc_p = p_call(p_ops, case, p_cap)
            assert rc_v == 0 and rc_p == 0
            replays = []
            for n, c in enumerate((case, other)):
                for ops, make in ((v_ops, q.viterbi_operands), (p_ops, q.posterior_operands)):
                    for dst, src in zip(ops, make(c)):
                        dst.copy_(torch.from_numpy(src).to(gpu))
                stream.synchronize()
                graph.replay()
                stream.synchronize()
                replays.append((v_host(v_cap, c), p_host(p_cap)))
                v_eager, p_eager = v_windows(g, c, f"eager{n}"), p_windows(g, c, f"eager{n}")
                assert v_call(v_ops, c, v_eager) == 0 and p_call(p_ops, c, p_eager) == 0
                stream.synchronize()
                for key in V_OUT:
                    assert q.same_bits(replays[-1][0][key], v_host(v_eager, c)[key]), key
                for key in P_OUT:
                    assert q.same_bits(replays[-1][1][key], p_host(p_eager)[key]), key
        torch.cuda.synchronize()
        tags = ("graph", "eager0", "eager1")  # (the bytes behind an odd count of back pointers stay canary: not a float to judge)
        g.check(written=[f"{k}.{tag}" for tag in tags for k in V_OUT + P_OUT], nonfinite_ok=[f"backptr.{tag}" for tag in tags])
    assert not q.same_bits(replays[0][0]["states"], replays[1][0]["states"]) and not q.same_bits(replays[0][1]["gamma"], replays[1][1]["gamma"])
    assert_viterbi(replays[1][0], q.viterbi(*q.viterbi_operands(other)), "replay")
    assert_posterior(replays[1][1], q.posterior(*q.posterior_operands(other)), "replay", exact=True)


def test_wrappers_return_device_tensors(gpu):
    import maua_stylegan2_amd.audioreactive as ar

    case = dict(S=25, T=257, kind="random", seed=31)
    logobs, log_trans, log_init = q.viterbi_operands(case)
    states, delta_last = ar.viterbi(logobs, torch.from_numpy(log_trans), log_init)
    assert states.is_cuda and states.dtype == torch.int32 and states.shape == (257,) and delta_last.dtype == torch.float64 and delta_last.shape == (25,)
    ref = q.viterbi(logobs, log_trans, log_init)
    assert q.same_bits(states.cpu().numpy(), ref[2]) and q.same_bits(delta_last.cpu().numpy(), ref[0])
    obs, trans, init = q.posterior_operands(case)
    gamma, loglik = ar.hmm_posterior(torch.from_numpy(obs).to(gpu), trans, init)
    want, scale = q.posterior(obs, trans, init)
    assert gamma.is_cuda and gamma.dtype == torch.float64 and q.same_bits(gamma.cpu().numpy(), want)
    assert isinstance(loglik, float) and abs(loglik - np.log(scale).sum()) <= 1e-12 * abs(np.log(scale).sum())
    with pytest.raises(ValueError, match="1 .. 128"):
        ar.viterbi(np.zeros((3, 129), np.float32), np.zeros((129, 129)), np.zeros(129))
