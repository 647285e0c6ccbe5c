"""GPU: maua_nmf_separate_f32 (csrc/separate.hip) called through the C ABI between red zones, over the case list of
tests/separate_ref.py, against the float64 definition there.  The tolerance is that of separate_ref.py: 4 x the error of an all-fp32
emulation over this same list, under the derived ceiling; never the kernel's."""
import ctypes

import numpy as np
import pytest
import torch

import separate_ref as sr
from maua_stylegan2_amd import _lib
from redzone import Guard

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

EINVAL = -22
CASES = sr.gpu_cases()


def call(ops, group, G, power, out_re, out_im, /, g0=0, n_out=None, **override):
    re, im, w, h = ops
    a = dict(re=re.data_ptr(), im=im.data_ptr(), w=w.data_ptr(), h=h.data_ptr(), F=re.shape[0], T=re.shape[1], K=w.shape[1], G=G, power=power,
             g0=g0, n_out=G - g0 if n_out is None else n_out, out_re=out_re.data_ptr(), out_im=out_im.data_ptr(), group=group)
    a.update(override)
    table = None if a["group"] is None else (ctypes.c_int32 * len(a["group"]))(*[int(x) for x in a["group"]])
    return _lib.load().maua_nmf_separate_f32(a["re"], a["im"], a["w"], a["h"], table, a["F"], a["T"], a["K"], a["G"], a["power"], a["g0"],
                                             a["n_out"], a["out_re"], a["out_im"], _lib.stream_ptr(re.device))


def operands(g, re, im, W, H, tag=""):
    return g.inp(re, f"re{tag}"), g.inp(im, f"im{tag}"), g.inp(W, f"w{tag}"), g.inp(H, f"h{tag}")


def outputs(g, n_out, F, T, tag):
    return g.out((n_out, F, T), f"out_re.{tag}"), g.out((n_out, F, T), f"out_im.{tag}")


def names(*tags):
    return [f"out_{part}.{tag}" for tag in tags for part in ("re", "im")]


def bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.ascontiguousarray(a)
    return a.view(np.int32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


@pytest.mark.parametrize("case", CASES, ids=sr.case_id)
def test_against_float64(gpu, case):
    """Against the definition at the tolerance of separate_ref.py; every element written; two runs bit-identical; G == 1 returns the
    input's bits; the stems add up to the input within (G + 2) u |input|."""
    re, im, W, H, group = sr.make_case(case)
    ref = sr.result(case)  # before the kernel runs
    F, T, G, power = case["F"], case["T"], case["G"], case["power"]
    with torch.cuda.device(gpu):
        g = Guard(gpu)
        ops = operands(g, re, im, W, H)
        runs = {}
        for rep in "ab":
            runs[rep] = outputs(g, G, F, T, rep)
            assert call(ops, group, G, power, *runs[rep]) == 0
        g.check(written=names("a", "b"))
    got = tuple(t.cpu().numpy() for t in runs["a"])
    assert same_bits(runs["a"][0], runs["b"][0]) and same_bits(runs["a"][1], runs["b"][1]), "two runs differ"
    tol = sr.tolerance(case)
    print(f"[{sr.case_id(case)}] worst relative error {sr.pair_error(got, ref):.3g} (tolerance {tol:.3g}, ceiling {sr.ceiling(case['K'], G, power):.3g})")
    assert sr.compare(got, ref, tol) == []
    if G == 1:
        assert same_bits(got[0][0], re) and same_bits(got[1][0], im), "G == 1 must return the input bit for bit"
    for out, x, what in ((got[0], re, "re"), (got[1], im, "im")):
        gap = np.abs(out.astype(np.float64).sum(axis=0) - x.astype(np.float64))
        bound = (G + 2) * sr.U * np.abs(x.astype(np.float64))
        print(f"    partition of unity ({what}): worst gap / bound {float((gap / np.maximum(bound, 1e-300)).max()):.3g}")
        assert (gap <= bound).all(), what


@pytest.mark.parametrize("case", [c for c in CASES if c["G"] > 1], ids=sr.case_id)
def test_every_window_gives_the_bits_of_the_full_call(gpu, case):
    re, im, W, H, group = sr.make_case(case)
    F, T, G, power = case["F"], case["T"], case["G"], case["power"]
    with torch.cuda.device(gpu):
        g = Guard(gpu)
        ops = operands(g, re, im, W, H)
        full = outputs(g, G, F, T, "full")
        assert call(ops, group, G, power, *full) == 0
        g.check(written=names("full"))
        for g0 in range(G):
            gw = Guard(gpu)  # (a fresh registry per start: the windows of one start are checked and released together)
            wins = {}
            for n_out in range(1, G - g0 + 1):
                wins[n_out] = outputs(gw, n_out, F, T, f"w{n_out}")
                assert call(ops, group, G, power, *wins[n_out], g0=g0, n_out=n_out) == 0
            gw.check(written=names(*[f"w{n}" for n in wins]))
            for n_out, (wr, wi) in wins.items():
                assert torch.equal(wr.view(torch.int32), full[0][g0:g0 + n_out].view(torch.int32)), (g0, n_out)
                assert torch.equal(wi.view(torch.int32), full[1][g0:g0 + n_out].view(torch.int32)), (g0, n_out)
        g.check()


@pytest.mark.parametrize("G,power", [(1, 1), (2, 2), (3, 1), (3, 2), (4, 2), (7, 1)])
def test_a_silent_column_is_split_equally(gpu, G, power):
    """All-zero columns of H (D == 0): every stem holds fl(1 / G) * re there — re / G exactly where G is a power of two — also in an
    empty group; a zero row of W does the same to its row."""
    case = dict(F=70, T=130, K=9, G=G, layout="interleaved", power=power, seed=41)
    re, im, W, H, group = sr.make_case(case)
    if G > 2:
        group = np.where(group == 1, 0, group).astype(np.int32)  # group 1 is empty
    silent = [0, 63, 64, 129]
    H[:, silent] = 0
    W[65] = 0
    with torch.cuda.device(gpu):
        g = Guard(gpu)
        out = outputs(g, G, 70, 130, "o")
        assert call(operands(g, re, im, W, H), group, G, power, *out) == 0
        g.check(written=names("o"))
    share = np.float32(1) / np.float32(G)
    for got, x in ((out[0].cpu().numpy(), re), (out[1].cpu().numpy(), im)):
        for s in range(G):
            assert same_bits(got[s][:, silent], share * x[:, silent]) and same_bits(got[s][65], share * x[65]), (s, G)
            if G in (1, 2, 4):
                assert same_bits(got[s][:, silent], x[:, silent] / np.float32(G))
    assert sr.compare(tuple(t.cpu().numpy() for t in out), sr.separate(re, im, W, H, group, G, power), sr.MASK_TOL) == []


@pytest.mark.parametrize("poison", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_a_non_finite_value_stays_in_its_column_and_row(gpu, poison):
    case = next(c for c in CASES if (c["F"], c["T"], c["K"], c["power"]) == (1025, 65, 8, 2))
    re, im, W, H, group = sr.make_case(case)
    F, T, G = case["F"], case["T"], case["G"]
    f0, t0 = 700, 64
    dirty = {"re": (re.copy(), im, W, H), "h": (re, im, W, H.copy()), "w": (re, im, W.copy(), H)}
    dirty["re"][0][f0, t0] = poison
    dirty["h"][3][5, t0] = poison
    dirty["w"][2][f0, 2] = poison
    with torch.cuda.device(gpu):
        g = Guard(gpu)
        clean = outputs(g, G, F, T, "clean")
        assert call(operands(g, re, im, W, H), group, G, 2, *clean) == 0
        outs = {}
        for name, arrays in dirty.items():
            outs[name] = outputs(g, G, F, T, name)
            assert call(operands(g, *arrays, tag=f".{name}"), group, G, 2, *outs[name]) == 0
        g.check(written=names("clean", *dirty), nonfinite_ok=names(*dirty))
    clean = [bits(t) for t in clean]
    other_cols, other_rows = np.arange(T) != t0, np.arange(F) != f0
    for part in (0, 1):
        got = {name: bits(outs[name][part]) for name in dirty}
        assert np.array_equal(got["re"][:, :, other_cols], clean[part][:, :, other_cols]) and np.array_equal(got["re"][:, other_rows], clean[part][:, other_rows])
        assert np.array_equal(got["h"][:, :, other_cols], clean[part][:, :, other_cols])
        assert np.array_equal(got["w"][:, other_rows], clean[part][:, other_rows])
        assert not np.array_equal(got["h"][:, :, t0], clean[part][:, :, t0]) and not np.array_equal(got["w"][:, f0], clean[part][:, f0])
    assert not np.array_equal(bits(outs["re"][0])[:, f0, t0], clean[0][:, f0, t0])


def test_refused_calls_leave_the_outputs_untouched(gpu):
    case = dict(F=8, T=70, K=3, G=2, layout="runs", power=2, seed=9)
    re, im, W, H, group = sr.make_case(case)
    refused = [dict(re=None), dict(im=None), dict(w=None), dict(h=None), dict(group=None), dict(F=0), dict(T=0), dict(K=0), dict(F=-1),
               dict(K=33, group=[0] * 33), dict(G=0), dict(G=33), dict(F=1 << 16, T=1 << 15), dict(power=0), dict(power=3), dict(g0=-1),
               dict(n_out=0), dict(g0=1, n_out=2), dict(g0=2, n_out=1), dict(n_out=3), dict(group=[0, 2, 1]), dict(group=[0, -1, 1]),
               dict(group=[0, 1, 1], G=1, n_out=1)]
    with torch.cuda.device(gpu):
        g = Guard(gpu)
        ops = operands(g, re, im, W, H)
        for i, kw in enumerate(refused):
            out = outputs(g, 2, 8, 70, f"r{i}")
            assert call(ops, group, 2, 2, *out, **kw) == EINVAL, kw
            assert g.untouched(f"out_re.r{i}") and g.untouched(f"out_im.r{i}"), kw
        for missing in ("out_re", "out_im"):
            out = outputs(g, 2, 8, 70, f"n.{missing}")
            assert call(ops, group, 2, 2, *out, **{missing: None}) == EINVAL
            assert g.untouched(f"out_re.n.{missing}") and g.untouched(f"out_im.n.{missing}")
        g.check()


def test_the_call_is_capturable(gpu):
    """The group table travels in the kernel arguments: a recorded launch replays without the host array, bit for bit."""
    case = next(c for c in CASES if (c["F"], c["T"], c["K"], c["power"]) == (7, 1000, 9, 1))
    re, im, W, H, group = sr.make_case(case)
    F, T, G = case["F"], case["T"], case["G"]
    with torch.cuda.device(gpu):
        g = Guard(gpu)
        ops = operands(g, re, im, W, H)
        eager, replayed = outputs(g, G, F, T, "eager"), outputs(g, G, F, T, "graph")
        assert call(ops, group, G, 1, *eager) == 0
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            assert call(ops, group, G, 1, *replayed) == 0
        for _ in range(2):
            replayed[0].fill_(-1.0), replayed[1].fill_(-1.0)
            graph.replay()
            torch.cuda.synchronize()
            assert same_bits(replayed[0], eager[0]) and same_bits(replayed[1], eager[1])
        g.check(written=names("eager", "graph"))
