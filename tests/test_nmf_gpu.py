"""GPU: maua_nmf_kl_f32 / maua_nmf_kl_div_f32 (csrc/nmf.hip) called through the C ABI between red zones, over the case list of
tests/nmf_ref.py, against the float64 definition there.

The entry works in place, so a run starts from guarded windows that hold a copy of the start: "every element written" cannot be read
off a canary; an element the kernel skipped keeps its start value and fails the tolerance instead (the updates move the elements by
tens of per cent, the tolerance is 1e-5).  The tolerances are those of nmf_ref.py: 4 x the error of an all-fp32 emulation over this
same list, never the kernel's."""
import numpy as np
import pytest
import torch

import nmf_ref as nr
from maua_stylegan2_amd import _lib
from redzone import Guard

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

EINVAL = -22
CASES = nr.gpu_cases()


def state(g, W0, H0, tag):
    """Guarded in-place windows ``w.<tag>`` / ``h.<tag>`` holding the start."""
    w, h = g.out(W0.shape, f"w.{tag}"), g.out(H0.shape, f"h.{tag}")
    w.copy_(torch.from_numpy(W0)), h.copy_(torch.from_numpy(H0))
    return w, h


def call(v, w, h, /, n_iter=1, update_w=1, update_h=1, eps=nr.EPS, **override):
    a = dict(v=v.data_ptr(), w=w.data_ptr(), h=h.data_ptr(), F=v.shape[0], T=v.shape[1], K=w.shape[1])
    a.update(override)
    return _lib.load().maua_nmf_kl_f32(a["v"], a["w"], a["h"], a["F"], a["T"], a["K"], n_iter, update_w, update_h, eps, _lib.stream_ptr(v.device))


def div_call(v, w, h, d, /, eps=nr.EPS, **override):
    a = dict(v=v.data_ptr(), w=w.data_ptr(), h=h.data_ptr(), d=d.data_ptr(), F=v.shape[0], T=v.shape[1], K=w.shape[1])
    a.update(override)
    return _lib.load().maua_nmf_kl_div_f32(a["v"], a["w"], a["h"], a["F"], a["T"], a["K"], eps, a["d"], _lib.stream_ptr(v.device))


def run(g, v, W0, H0, tag, **kw):
    w, h = state(g, W0, H0, tag)
    assert call(v, w, h, **kw) == 0, (tag, kw)
    return w, h


def bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.ascontiguousarray(a)
    return a.view(np.int64 if a.dtype == np.float64 else np.int32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


@pytest.mark.parametrize("case", CASES, ids=nr.case_id)
def test_single_steps_against_float64(gpu, case):
    V, W0, H0 = nr.make_case(case)
    ref = nr.steps(case)  # before the kernel runs
    flags = {"h_only": dict(update_w=0), "w_only": dict(update_h=0), "full": {}}
    with torch.cuda.device(gpu):
        g = Guard(gpu)
        v = g.inp(V, "v")
        runs = {(kind, rep): run(g, v, W0, H0, f"{kind}.{rep}", **kw) for kind, kw in flags.items() for rep in "ab"}
        g.check(written=[f"{name}.{kind}.{rep}" for kind in flags for rep in "ab" for name in "wh"])
    for kind in flags:
        for i in (0, 1):
            assert same_bits(runs[kind, "a"][i], runs[kind, "b"][i]), f"{kind}: two runs differ"
    host = {kind: tuple(t.cpu().numpy() for t in runs[kind, "a"]) for kind in flags}
    assert same_bits(host["h_only"][0], W0), "an H-only step changed W"
    assert same_bits(host["w_only"][1], H0), "a W-only step changed H"
    assert same_bits(host["full"][1], host["h_only"][1]), "the H step of an iteration differs from the H-only step"
    got = {"h_only": host["h_only"][1], "w_only": host["w_only"][0], "full": host["full"]}
    F, T, K = case["F"], case["T"], case["K"]
    print(f"[{nr.case_id(case)}] H-only {nr.rel_error(got['h_only'], ref['h_only']):.3g} (tol {nr.H_STEP_TOL:.3g}, ceiling {nr.h_ceiling(F, T, K):.3g})  "
          f"W-only {nr.rel_error(got['w_only'], ref['w_only']):.3g} ({nr.W_ONLY_TOL:.3g}, {nr.w_only_ceiling(F, T, K):.3g})  "
          f"W after H {nr.rel_error(got['full'][0], ref['full'][0]):.3g} ({nr.W_AFTER_H_TOL:.3g}, {nr.w_ceiling(F, T, K):.3g})")
    assert nr.compare_steps(got, ref) == []


@pytest.mark.parametrize("shape", nr.CHAINED, ids=lambda s: "F{}-T{}-K{}".format(*s))
def test_chained_iterations(gpu, shape):
    """8 iterations one call at a time, each compared with ONE float64 iteration from the device's own previous state (no error
    accumulates into the comparison); the n_iter = 8 call from the same start equals the eight calls bit for bit."""
    case = next(c for c in CASES if (c["F"], c["T"], c["K"]) == shape)
    V, W0, H0 = nr.make_case(case)
    with torch.cuda.device(gpu):
        g = Guard(gpu)
        v = g.inp(V, "v")
        w, h = state(g, W0, H0, "single")
        trail = [(W0, H0)]
        for _ in range(8):
            assert call(v, w, h) == 0
            trail.append((w.cpu().numpy(), h.cpu().numpy()))
        w8, h8 = run(g, v, W0, H0, "eight", n_iter=8)
        g.check(written=["w.single", "h.single", "w.eight", "h.eight"])
    assert same_bits(w8, trail[-1][0]) and same_bits(h8, trail[-1][1]), "n_iter = 8 differs from eight calls of one"
    worst = [0.0, 0.0]
    for (Wp, Hp), (Wn, Hn) in zip(trail[:-1], trail[1:]):
        Wr, Hr = nr.iterate(V, Wp, Hp, 1)
        worst = [max(worst[0], nr.rel_error(Hn, Hr)), max(worst[1], nr.rel_error(Wn, Wr))]
        assert nr.compare(Hn, Hr, nr.H_STEP_TOL, "H") + nr.compare(Wn, Wr, nr.W_AFTER_H_TOL, "W") == []
    print(f"[{nr.case_id(case)}] chained: worst H {worst[0]:.3g}, W {worst[1]:.3g}")


@pytest.mark.parametrize("case", CASES, ids=nr.case_id)
def test_divergence_entry(gpu, case):
    V, W0, H0 = nr.make_case(case)
    want, tol = nr.divergence_cols(V, W0, H0), nr.divergence_tolerance(V, W0, H0)
    with torch.cuda.device(gpu):
        g = Guard(gpu)
        v, w, h = g.inp(V, "v"), g.inp(W0, "w"), g.inp(H0, "h")
        outs = [g.out((case["T"],), f"d.{rep}", torch.float64) for rep in "ab"]
        for d in outs:
            assert div_call(v, w, h, d) == 0
        g.check(written=["d.a", "d.b"])
    assert same_bits(outs[0], outs[1]), "two runs differ"
    err = np.abs(outs[0].cpu().numpy() - want)
    print(f"[{nr.case_id(case)}] divergence: worst |error| / tolerance {float((err / tol).max()):.3g}")
    assert (err <= tol).all()


def test_zeros_absorb_bit_for_bit(gpu):
    """Planted zeros in W and H stay zero over 3 iterations; silent columns of V give zero columns of H and a zero template a zero
    activation row after ONE H step."""
    case = dict(F=65, T=257, K=5, seed=77)
    V, W0, H0 = nr.make_case(case)
    rng = np.random.default_rng(78)
    zw, zh = rng.random(W0.shape) < 0.1, rng.random(H0.shape) < 0.1
    W0[zw], H0[zh] = 0.0, 0.0
    silent = [0, 63, 64, 200, 256]
    V[:, silent] = 0.0
    W0[:, 3] = 0.0
    with torch.cuda.device(gpu):
        g = Guard(gpu)
        v = g.inp(V, "v")
        w1, h1 = run(g, v, W0, H0, "one", update_w=0)
        w3, h3 = run(g, v, W0, H0, "three", n_iter=3)
        g.check(written=["w.one", "h.one", "w.three", "h.three"])
    h1, w3, h3 = h1.cpu().numpy(), w3.cpu().numpy(), h3.cpu().numpy()
    zero = np.zeros(1, np.float32).view(np.int32)[0]
    assert (bits(h1)[:, silent] == zero).all() and (bits(h1)[3] == zero).all()
    assert (bits(h1)[zh] == zero).all() and (bits(h3)[zh] == zero).all() and (bits(w3)[zw] == zero).all()
    assert (bits(w3)[:, 3] == zero).all() and (bits(h3)[3] == zero).all() and (bits(h3)[:, silent] == zero).all()
    live = ~zh
    live[:, silent], live[3] = False, False
    assert (h1[live] > 0).all()


def test_exact_quotients_give_exact_results(gpu):
    """Integers chosen so that every product, sum and quotient is a float32 number: P = 4 * 2^j, V / P in {1, 2, 4}, the sums are small
    integers and the denominators powers of two.  The result is float64's, bit for bit."""
    rng = np.random.default_rng(5)
    with torch.cuda.device(gpu):
        g = Guard(gpu)
        # H step: F = 128 (every wave of a workgroup sums 32 rows), T = 130 (three workgroups, the last with 2 live lanes), W = 1
        F, T = 128, 130
        W0 = np.ones((F, 2), np.float32)
        H0 = (np.array([[1.0], [3.0]]) * 2.0 ** rng.integers(-2, 3, (1, T))).astype(np.float32)
        V = (H0.sum(axis=0)[None, :] * 2.0 ** rng.integers(0, 3, (F, T))).astype(np.float32)
        _, h = run(g, g.inp(V, "v.h"), W0, H0, "hstep", update_w=0)
        want_h = nr.h_step(V, W0, H0)
        # W step: T = 512 (two strides of the 256 lanes), F = 5 (three workgroups, the last with one live row), H = 1
        F, T = 5, 512
        H1 = np.ones((2, T), np.float32)
        W1 = (np.array([[1.0, 3.0]]) * 2.0 ** rng.integers(-2, 3, (F, 1))).astype(np.float32)
        V1 = (W1.sum(axis=1)[:, None] * 2.0 ** rng.integers(0, 3, (F, T))).astype(np.float32)
        w, _ = run(g, g.inp(V1, "v.w"), W1, H1, "wstep", update_h=0)
        want_w = nr.w_step(V1, W1, H1)
        g.check(written=["w.hstep", "h.hstep", "w.wstep", "h.wstep"])
    assert np.array_equal(want_h, want_h.astype(np.float32)) and np.array_equal(want_w, want_w.astype(np.float32))
    assert not np.array_equal(want_h, H0) and not np.array_equal(want_w, W1)
    assert same_bits(h, want_h.astype(np.float32)) and same_bits(w, want_w.astype(np.float32))


def test_zero_iterations_launch_nothing(gpu):
    case = CASES[3]
    V, W0, H0 = nr.make_case(case)
    with torch.cuda.device(gpu):
        g = Guard(gpu)
        v = g.inp(V, "v")
        w, h = g.out(W0.shape, "w.none"), g.out(H0.shape, "h.none")
        assert call(v, w, h, n_iter=0) == 0
        assert g.untouched("w.none") and g.untouched("h.none")
        g.check()


@pytest.mark.parametrize("poison", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_a_non_finite_value_stays_in_its_column_with_a_fixed_dictionary(gpu, poison):
    case = next(c for c in CASES if (c["F"], c["T"], c["K"]) == (65, 257, 16))
    V, W0, H0 = nr.make_case(case)
    f, t = 40, 130
    bad = V.copy()
    bad[f, t] = poison
    clear = np.arange(case["T"]) != t
    with torch.cuda.device(gpu):
        g = Guard(gpu)
        runs = {}
        for name, data in (("clean", V), ("dirty", bad)):
            v = g.inp(data, f"v.{name}")
            for n in (1, 3):
                runs[name, n] = run(g, v, W0, H0, f"{name}{n}", n_iter=n, update_w=0)[1]
        names = [f"{x}.{name}{n}" for x in "wh" for name in ("clean", "dirty") for n in (1, 3)]
        g.check(written=names, nonfinite_ok=[n for n in names if "dirty" in n])
    for n in (1, 3):
        clean, dirty = runs["clean", n].cpu().numpy(), runs["dirty", n].cpu().numpy()
        assert np.array_equal(bits(clean)[:, clear], bits(dirty)[:, clear]), "a column that does not hold the value changed"
        assert not np.array_equal(bits(clean)[:, t], bits(dirty)[:, t])


def test_refused_calls_leave_the_outputs_untouched(gpu):
    V, W0, H0 = nr.make_case(dict(F=8, T=70, K=3, seed=9))
    refused = [dict(v=None), dict(w=None), dict(h=None), dict(F=0), dict(T=0), dict(K=0), dict(F=-1), dict(K=33), dict(n_iter=-1),
               dict(eps=0.0), dict(eps=-1e-12), dict(eps=float("nan")), dict(eps=float("inf")), dict(update_w=0, update_h=0),
               dict(F=1 << 16, T=1 << 15)]
    with torch.cuda.device(gpu):
        g = Guard(gpu)
        v = g.inp(V, "v")
        for i, kw in enumerate(refused):
            w, h = g.out(W0.shape, f"w.r{i}"), g.out(H0.shape, f"h.r{i}")
            assert call(v, w, h, **kw) == EINVAL, kw
            assert g.untouched(f"w.r{i}") and g.untouched(f"h.r{i}"), kw
        win, hin = g.inp(W0, "w"), g.inp(H0, "h")
        for i, kw in enumerate([dict(v=None), dict(w=None), dict(h=None), dict(d=None), dict(F=0), dict(T=0), dict(K=0), dict(K=33),
                                dict(eps=0.0), dict(eps=float("nan")), dict(F=1 << 16, T=1 << 15)]):
            d = g.out((70,), f"d.r{i}", torch.float64)
            assert div_call(v, win, hin, d, **kw) == EINVAL, kw
            assert g.untouched(f"d.r{i}"), kw
        g.check()


def test_the_call_is_capturable(gpu):
    """Three iterations recorded in a torch.cuda.graph; each replay, from the restored start, equals the eager call bit for bit."""
    case = next(c for c in CASES if (c["F"], c["T"], c["K"]) == (257, 255, 8))
    V, W0, H0 = nr.make_case(case)
    with torch.cuda.device(gpu):
        g = Guard(gpu)
        v = g.inp(V, "v")
        we, he = run(g, v, W0, H0, "eager", n_iter=3)
        w, h = state(g, W0, H0, "graph")
        d = g.out((case["T"],), "d.graph", torch.float64)
        de = g.out((case["T"],), "d.eager", torch.float64)
        assert div_call(v, we, he, de) == 0
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            assert call(v, w, h, n_iter=3) == 0
            assert div_call(v, w, h, d) == 0
        for _ in range(2):
            w.copy_(torch.from_numpy(W0)), h.copy_(torch.from_numpy(H0))
            d.fill_(-1.0)
            graph.replay()
            torch.cuda.synchronize()
            assert same_bits(w, we) and same_bits(h, he) and same_bits(d, de)
        g.check(written=["w.eager", "h.eager", "w.graph", "h.graph", "d.graph", "d.eager"])
