"""GPU: the two pYIN entries (csrc/pyin.hip) called through the C ABI between red zones, over the case lists of tests/pyin_ref.py.

maua_pyin_candidates_f32 on host-built d' rows against the float32 restatement: obs and voiced_prob within n 2^-24 1.01 (n = the
summands of the element), obs bit for bit where an element has at most one summand, period within 4 x the float32-against-float64
figure, bins exact except on the frames (decided on the CPU, at most 2 % of a case) where a refined period lies within twice that
tolerance of a bin edge.  maua_pyin_viterbi_f64 against the float64 restatement, bit for bit in delta_last, backptr and states, over
b_cases() and over pyin_ref.EDGE_CASES, the (P, W) pairs either side of the scan's clamp at one wave, 64 / 65 and two waves.  Every
case ends with Guard.check: red zones intact, every output element written."""
import numpy as np
import pytest
import torch

import pyin_ref as q
from maua_stylegan2_amd import _lib
from redzone import Guard

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

EINVAL = -22
A_OUT = ("obs", "period", "voiced_prob")
B_OUT = ("delta_last", "backptr", "states")


# ------------------------------------------------------------------------------------------------ entry A
def a_windows(g, case, tag):
    T, P = case["n_frames"], case["n_bins"]
    return {"obs": g.out((T, P), f"obs.{tag}"), "period": g.out((T, P), f"period.{tag}"), "voiced_prob": g.out((T,), f"voiced_prob.{tag}")}


def a_call(rows, cum, edges, case, out, **override):
    a = dict(case, **override)
    ptr = lambda name, t: None if a.get("null") == name else t.data_ptr()  # noqa: E731
    return _lib.load().maua_pyin_candidates_f32(ptr("cmndf", rows), a["n_frames"], a["tau_min"], a["tau_max"], ptr("cum_prior", cum), a["n_thr"],
                                                a["no_trough_prob"], ptr("edges", edges), a["n_bins"], ptr("obs", out["obs"]),
                                                ptr("period", out["period"]), ptr("voiced_prob", out["voiced_prob"]),
                                                _lib.stream_ptr(rows.device))


def host(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("case", q.a_cases(), ids=q.a_case_id)
def test_candidates_against_the_float32_restatement(gpu, case):
    cum, edges = q.case_tables(case)
    ref = q.a_reference(case)
    assert int(q.near_edge_frames(ref, edges).sum()) <= q.max_exempt(case["n_frames"])  # decided before the kernel runs
    with torch.cuda.device(gpu):
        g = Guard(gpu)
        rows, cum_d, edges_d = g.inp(q.make_rows(case), "cmndf"), g.inp(cum, "cum_prior"), g.inp(edges, "edges")
        runs = []
        for tag in ("a", "b"):
            out = a_windows(g, case, tag)
            assert a_call(rows, cum_d, edges_d, case, out) == 0
            runs.append(out)
        g.check(written=[f"{k}.{tag}" for tag in ("a", "b") for k in A_OUT])
    a, b = host(runs[0]), host(runs[1])
    for key in A_OUT:
        assert same_bits(a[key], b[key]), f"{key}: two runs differ"
    worst = float(np.abs(a["obs"].astype(np.float64) - ref["obs"]).max())
    print(f"[{q.a_case_id(case)}] obs worst {worst:.3g}, voiced_prob worst {np.abs(a['voiced_prob'].astype(np.float64) - ref['voiced_prob']).max():.3g}, "
          f"{sum(len(c) for c in ref['cands'])} candidates")
    assert q.compare_candidates(a, ref, edges) == []


def test_candidates_refusals_leave_the_outputs_untouched(gpu):
    case = dict(tau_min=10, tau_max=340, kind="random", n_bins=65, n_frames=2, n_thr=100, no_trough_prob=0.01, seed=1)
    cum, edges = q.case_tables(case)
    refused = ([dict(null=k) for k in ("cmndf", "cum_prior", "edges", "obs", "period", "voiced_prob")]
               + [dict(n_frames=0), dict(n_frames=-1), dict(tau_min=0), dict(tau_min=340), dict(tau_max=2049), dict(n_thr=0), dict(n_thr=257),
                  dict(n_bins=0), dict(n_bins=1025), dict(no_trough_prob=-0.01), dict(no_trough_prob=1.01), dict(no_trough_prob=float("nan")),
                  dict(no_trough_prob=float("inf"))])
    with torch.cuda.device(gpu):
        g = Guard(gpu)
        rows, cum_d, edges_d = g.inp(q.make_rows(case), "cmndf"), g.inp(cum, "cum_prior"), g.inp(edges, "edges")
        for i, kw in enumerate(refused):
            out = a_windows(g, case, f"r{i}")
            assert a_call(rows, cum_d, edges_d, case, out, **kw) == EINVAL, kw
            assert all(g.untouched(f"{k}.r{i}") for k in A_OUT), kw
        g.check()


# ------------------------------------------------------------------------------------------------ entry B
def b_windows(g, case, tag):
    T, P = case["n_frames"], case["n_bins"]
    return {"delta_last": g.out((2 * P,), f"delta_last.{tag}", torch.float64), "states": g.out((T,), f"states.{tag}", torch.int32),
            "backptr": g.out((T * 2 * P // 2,), f"backptr.{tag}", torch.int32)}  # T x 2 P uint16 = T P dwords


def b_call(lov, lou, tri, norm, consts, case, out, **override):
    a = dict(case, **override)
    ptr = lambda name, t: None if a.get("null") == name else t.data_ptr()  # noqa: E731
    return _lib.load().maua_pyin_viterbi_f64(ptr("lov", lov), ptr("lou", lou), a["n_frames"], a["n_bins"], a["width"], ptr("tri", tri),
                                             ptr("norm", norm), consts[0], consts[1], consts[2], ptr("delta_last", out["delta_last"]),
                                             ptr("backptr", out["backptr"]), ptr("states", out["states"]), _lib.stream_ptr(lov.device))


def b_host(out, case):
    return {"delta_last": out["delta_last"].cpu().numpy(), "states": out["states"].cpu().numpy(),
            "backptr": out["backptr"].cpu().numpy().view(np.uint16).reshape(case["n_frames"], 2 * case["n_bins"])}


def b_operands(g, case):
    lov, lou = q.make_logobs(case)
    tri, norm, *consts = q.b_constants(case)
    return (g.inp(lov, "lov"), g.inp(lou, "lou"), g.inp(tri, "tri", torch.float64), g.inp(norm, "norm", torch.float64), consts), (lov, lou)


def run_b(gpu, case):
    with torch.cuda.device(gpu):
        g = Guard(gpu)
        ops, raw = b_operands(g, case)
        out = b_windows(g, case, "a")
        assert b_call(*ops, case, out) == 0
        g.check(written=[f"{k}.a" for k in B_OUT], nonfinite_ok=["delta_last.a"])
        return b_host(out, case), raw


def assert_b_equal(got, ref, what):
    delta, back, states = ref
    assert same_bits(got["delta_last"], delta), f"{what}: delta_last"
    assert np.array_equal(got["backptr"], back), f"{what}: backptr differs in {int((got['backptr'] != back).sum())} elements"
    assert np.array_equal(got["states"], states), f"{what}: states"


@pytest.mark.parametrize("case", q.b_cases(), ids=q.b_case_id)
def test_viterbi_bit_for_bit(gpu, case):
    ref = q.b_reference(case)
    got, (lov, lou) = run_b(gpu, case)
    assert_b_equal(got, ref, q.b_case_id(case))
    if case["kind"] == "nan":  # nothing before the frame of the NaN changes: the forward pass is causal
        clean_case = dict(case, kind="random")
        clean, _ = run_b(gpu, clean_case)
        at = case["n_frames"] // 2
        assert np.array_equal(got["backptr"][:at + 1], clean["backptr"][:at + 1])  # (row `at` is decided by the frames before it)
    if case["kind"] == "inf_frame" and case["n_frames"] > 1:
        assert np.isneginf(got["delta_last"]).all() and got["states"][-1] == 0


@pytest.mark.parametrize("case", q.edge_cases(), ids=q.b_case_id)
def test_viterbi_reach_clamp_edges(gpu, case):
    """pyin_ref.EDGE_CASES: W = P - 2, P - 1 and >= P (either side of the scan's clamp reach = min(W, P - 1)) with one wave, across the
    64 / 65 boundary and with two waves; two runs identical."""
    ref = q.b_reference(case)
    with torch.cuda.device(gpu):
        g = Guard(gpu)
        ops, _ = b_operands(g, case)
        runs = []
        for tag in ("a", "b"):
            out = b_windows(g, case, tag)
            assert b_call(*ops, case, out) == 0
            runs.append(out)
        g.check(written=[f"{k}.{tag}" for tag in ("a", "b") for k in B_OUT])
        a, b = (b_host(out, case) for out in runs)
    for key in B_OUT:
        assert same_bits(a[key], b[key]), f"{key}: two runs differ"
    assert_b_equal(a, ref, q.b_case_id(case))


def test_viterbi_twenty_thousand_frames(gpu):
    """P = 602, W = 50, T = 20 000: delta reaches -1e5, where only double accumulators keep the decisions of the reference."""
    ref = q.b_reference(q.LONG_CASE)
    got, _ = run_b(gpu, q.LONG_CASE)
    print(f"final delta {ref[0].max():.1f}, {int((ref[2] < 602).sum())} voiced frames of 20000")
    assert ref[0].max() < -2e4
    assert_b_equal(got, ref, "long")


def test_viterbi_refusals_leave_the_outputs_untouched(gpu):
    case = dict(n_bins=65, width=50, n_frames=3, kind="random", seed=2)
    refused = ([dict(null=k) for k in ("lov", "lou", "tri", "norm", "delta_last", "backptr", "states")]
               + [dict(n_frames=0), dict(n_frames=-3), dict(n_bins=0), dict(n_bins=1025), dict(width=-1), dict(width=129)])
    with torch.cuda.device(gpu):
        g = Guard(gpu)
        ops, _ = b_operands(g, case)
        for i, kw in enumerate(refused):
            out = b_windows(g, case, f"r{i}")
            assert b_call(*ops, case, out, **kw) == EINVAL, kw
            assert all(g.untouched(f"{k}.r{i}") for k in B_OUT), kw
        g.check()


# ------------------------------------------------------------------------------------------------ both entries under capture
def test_both_entries_are_capturable(gpu):
    """Captured into one hipGraph and replayed on new input in the same buffers: each replay equals the eager calls bit for bit."""
    a_case = dict(tau_min=10, tau_max=340, kind="random", n_bins=602, n_frames=65, n_thr=100, no_trough_prob=0.01, seed=11)
    b_case = dict(n_bins=65, width=50, n_frames=257, kind="random", seed=12)
    a_other, b_other = dict(a_case, seed=13), dict(b_case, seed=14, kind="integer")
    cum, edges = q.case_tables(a_case)
    stream = torch.cuda.Stream(gpu)
    with torch.cuda.device(gpu):
        g = Guard(gpu)
        rows, cum_d, edges_d = g.inp(q.make_rows(a_case), "cmndf"), g.inp(cum, "cum_prior"), g.inp(edges, "edges")
        ops, _ = b_operands(g, b_case)
        a_cap, b_cap = a_windows(g, a_case, "graph"), b_windows(g, b_case, "graph")
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            with _lib.HipGraph() as graph:
                rc_a = a_call(rows, cum_d, edges_d, a_case, a_cap)
                rc_b = b_call(*ops, b_case, b_cap)
            assert rc_a == 0 and rc_b == 0
            replays = []
            for ac, bc in ((a_case, b_case), (a_other, b_other)):
                rows.copy_(torch.from_numpy(q.make_rows(ac)).to(gpu))
                lov, lou = q.make_logobs(bc)
                ops[0].copy_(torch.from_numpy(lov).to(gpu)), ops[1].copy_(torch.from_numpy(lou).to(gpu))
                stream.synchronize()
                graph.replay()
                stream.synchronize()
                replays.append((host(a_cap), b_host(b_cap, bc)))
                a_eager, b_eager = a_windows(g, ac, f"eager{len(replays)}"), b_windows(g, bc, f"eager{len(replays)}")
                assert a_call(rows, cum_d, edges_d, ac, a_eager) == 0 and b_call(*ops, bc, b_eager) == 0
                stream.synchronize()
                for key in A_OUT:
                    assert same_bits(replays[-1][0][key], host(a_eager)[key]), key
                for key in B_OUT:
                    assert same_bits(replays[-1][1][key], b_host(b_eager, bc)[key]), key
        torch.cuda.synchronize()
        g.check(written=[f"{k}.{tag}" for tag in ("graph", "eager1", "eager2") for k in A_OUT + B_OUT])
    assert not same_bits(replays[0][0]["obs"], replays[1][0]["obs"]) and not same_bits(replays[0][1]["states"], replays[1][1]["states"])
    assert q.compare_candidates(replays[1][0], q.a_reference(a_other), edges) == []
    assert_b_equal(replays[1][1], q.b_reference(b_other), "replay")
