"""GPU: the two entries of csrc/iir.hip called through the C ABI between red zones, over the case lists of tests/iir_ref.py.

maua_sosfilt_f64: n_sections in {1, 2, 4, 12, 16} x {one filter, a bank of three over one signal, a bank of three over three signals} x
chunk in {4, 64, default} x n around the chunk length (1, 2, chunk - 1, chunk, chunk + 1, 3 chunk + 5), 5000 and — for the default —
20 000, the six combinations of input and output type taking turns.  Every call runs twice into
separate windows and must give identical bits; the double output must lie within allow * max|y| of the long-double loop (iir_ref.allowance:
what the float64 algorithms themselves lose, times 4), the float output must be the double one rounded once.  Integer filters bit for bit.
Every instance — n_sections 1 .. 16 — runs a bank of integer cascades bit for bit and a bank of three Butterworth band-passes against
long double; every edge of the chunk grid (partial tiles, the carry's look-ahead, workgroups with one live chunk, chunks of 4096 and
65 536 samples, 64 filters with their own zi and zf) runs on integers, bit for bit.
Every case ends with Guard.check: red zones intact, every output element written."""
import numpy as np
import pytest
import torch

import iir_ref as q
from maua_stylegan2_amd import _lib
from redzone import Guard

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

EINVAL = -22


def sos_call(gpu, a):
    ptr = lambda k: None if a.get(k) is None else a[k].data_ptr()  # noqa: E731
    return _lib.load().maua_sosfilt_f64(ptr("sos"), a["F"], a["ns"], ptr("x32"), ptr("x64"), a["n_signals"], a["n"], a["chunk"], ptr("zi"),
                                        ptr("y64"), ptr("y32"), ptr("zf"), ptr("ws"), _lib.stream_ptr(gpu))


def windows(g, sos, x, inp, chunk, zi=None):
    """The operands of a call in guarded windows: sos [F, ns, 6]; x [n] (shared) or [F, n]."""
    F, ns = sos.shape[:2]
    n = x.shape[-1]
    a = dict(F=F, ns=ns, n=n, chunk=chunk, n_signals=1 if x.ndim == 1 else F, sos=g.inp(sos, "sos", torch.float64))
    a["x32" if inp == "f32" else "x64"] = g.inp(x, "x", torch.float32 if inp == "f32" else torch.float64)
    if zi is not None:
        a["zi"] = g.inp(zi, "zi", torch.float64)
    n_ws = _lib.load().maua_sosfilt_ws_doubles(F, ns, n, chunk)
    assert n_ws >= 1
    a["ws"] = g.out((n_ws,), "ws", torch.float64)
    return a


def run_twice(gpu, sos, x, inp="f64", outp="f64", chunk=0, zi=None, want_zf=False, nonfinite=False):
    """Two calls on the same operands into separate output windows: identical bits, red zones, everything written.
    -> dict of numpy arrays y64 / y32 / zf (those asked for)."""
    F, ns = sos.shape[:2]
    n = x.shape[-1]
    with torch.cuda.device(gpu):
        g = Guard(gpu)
        a = windows(g, sos, x, inp, chunk, zi)
        runs, names = [], []
        for tag in ("a", "b"):
            out = {}
            if outp in ("f64", "both"):
                out["y64"] = g.out((F, n), f"y64.{tag}", torch.float64)
            if outp in ("f32", "both"):
                out["y32"] = g.out((F, n), f"y32.{tag}", torch.float32)
            if want_zf:
                out["zf"] = g.out((F, ns, 2), f"zf.{tag}", torch.float64)
            assert sos_call(gpu, dict(a, **out)) == 0
            names += [f"{k}.{tag}" for k in out if n or k == "zf"]
            runs.append(out)
        g.check(written=names, nonfinite_ok=names if nonfinite else ())
        host = [{k: v.cpu().numpy() for k, v in out.items()} for out in runs]
    for k in host[0]:
        assert q.same_bits(host[0][k], host[1][k]), f"{k}: two runs differ"
    return host[0]


def judge(gpu, got, names, sig, n, chunk, inp, outp, sos, x):
    """The outputs of one call against the long-double reference and against each other."""
    refs = [q.longdouble(name, s)[:n] for name, s in zip(names, sig)]
    allows = [q.allowance(name, chunk, s, n) for name, s in zip(names, sig)]
    return judge_bank(gpu, got, names, refs, allows, n, chunk, inp, outp, sos, x)


def judge_bank(gpu, got, names, refs, allows, n, chunk, inp, outp, sos, x):
    """`judge` for any bank: refs[f] the long-double output of filter f, allows[f] its allowance.  -> the worst error / bound."""
    y64 = got.get("y64")
    if y64 is None:  # the double this float must be the rounding of: the same call with the double output
        y64 = run_twice(gpu, sos, x, inp, "f64", chunk)["y64"]
    worst = 0.0
    for f, (name, ref, allow) in enumerate(zip(names, refs, allows)):
        err = float(np.max(np.abs(y64[f].astype(np.longdouble) - ref)))
        bound = allow * float(np.max(np.abs(ref)))
        assert err <= bound, f"{name} n={n} chunk={chunk} {inp}->{outp}: |y - long double| = {err:.3e} > {bound:.3e}"
        worst = max(worst, err / bound)
    if "y32" in got:
        assert q.same_bits(got["y32"], y64.astype(np.float32)), f"n={n} {inp}->{outp}: the float output is not the rounded double"
    return worst


CASES = [(ns, mode, chunk) for ns in (1, 2, 12, 16) for mode in q.MODES for chunk in q.CHUNKS]


@pytest.mark.parametrize("ns,mode,chunk", CASES, ids=lambda v: str(v))
def test_sosfilt_against_long_double(gpu, ns, mode, chunk):
    names, sos, sig = q.bank(ns, mode)
    turn = CASES.index((ns, mode, chunk))
    for i, n in enumerate(q.lengths(chunk)):
        inp, outp = q.IO[(turn + i) % len(q.IO)]
        x = q.signals()[0, :n] if mode != "bank_own" else q.signals()[list(sig), :n]
        got = run_twice(gpu, sos, x, inp, outp, chunk)
        judge(gpu, got, names, sig, n, chunk, inp, outp, sos, x)


@pytest.mark.parametrize("chunk", q.CHUNKS)
def test_sosfilt_worst_conditioned_filter(gpu, chunk):
    """The 8th-order 20-200 Hz band-pass (4 sections): the filter whose chunked form loses most."""
    sos = q.filters()["bp20_200"][None]
    for i, n in enumerate((5000, q.N_REF)):
        inp, outp = q.IO[(2 * i + 2) % len(q.IO)]
        x = q.signals()[0, :n]
        judge(gpu, run_twice(gpu, sos, x, inp, outp, chunk), ("bp20_200",), (0,), n, chunk, inp, outp, sos, x)


@pytest.mark.parametrize("name", sorted(q.EXACT))
@pytest.mark.parametrize("chunk", [1, 4, 7, 64, 0])
def test_sosfilt_integer_filters_bit_for_bit(gpu, name, chunk):
    sos = q.EXACT[name][None]
    x = q.exact_signal(203)
    zi = np.arange(1, 2 * sos.shape[1] + 1, dtype=np.float64).reshape(1, -1, 2)
    for z in (None, zi):
        want, want_zf = q.sequential(sos, x, zi=z)
        got = run_twice(gpu, sos, x, "f32" if chunk % 2 else "f64", "both", chunk, zi=z, want_zf=True)
        assert q.same_bits(got["y64"], want) and q.same_bits(got["zf"], want_zf) and q.same_bits(got["y32"], want.astype(np.float32))
    if name == "running_sum":
        assert q.same_bits(run_twice(gpu, sos, x, chunk=chunk)["y64"][0], np.cumsum(x))


def test_sosfilt_default_chunk_beyond_its_minimum(gpu):
    """40 000 samples (the default chunk is 128, the last chunk is short) and 140 000 (256): the running sum of small integers and the
    two-section integer filter, bit for bit, shared and own signals."""
    for n in (40000, 140000):
        assert q.default_chunk(n) == (128 if n == 40000 else 256)
        x = np.stack([q.exact_signal(n, seed=1), q.exact_signal(n, seed=2)])
        got = run_twice(gpu, np.stack([q.EXACT["running_sum"]] * 2), x, "f32", "both", 0, want_zf=True)
        assert q.same_bits(got["y64"], np.cumsum(x, axis=1)) and q.same_bits(got["y32"], np.cumsum(x, axis=1).astype(np.float32))
    mix = np.stack([q.EXACT["mix"], q.EXACT["mix"][::-1]])
    want = np.cumsum(np.convolve(x[0], [1.0, 2.0, 1.0])[: x.shape[1]])  # (either order of the two sections: they commute from a zero state)
    got = run_twice(gpu, mix, x[0], "f64", "f64", 0)
    assert q.same_bits(got["y64"], np.stack([want, want]))


@pytest.mark.parametrize("name,chunk", [("rms", 64), ("pitch", 0), ("lp100", 4), ("wide16", 64)])
def test_sosfilt_split_in_two_calls(gpu, name, chunk):
    """x[:cut] with zf, then x[cut:] with zi = zf: the concatenation is the one call, within the allowance (the chunk grid differs)."""
    sos = q.filters()[name][None]
    n, cut = 5000, 1777
    x = q.signals()[0, :n]
    first = run_twice(gpu, sos, x[:cut], "f32", "f64", chunk, want_zf=True)
    second = run_twice(gpu, sos, x[cut:], "f32", "f64", chunk, zi=first["zf"], want_zf=True)
    whole = run_twice(gpu, sos, x, "f32", "f64", chunk, want_zf=True)
    ref = q.longdouble(name)[:n]
    bound = q.allowance(name, chunk, 0, n) * float(np.max(np.abs(ref)))
    joined = np.concatenate([first["y64"], second["y64"]], axis=1)
    assert float(np.max(np.abs(joined[0].astype(np.longdouble) - ref))) <= bound
    assert float(np.max(np.abs(whole["y64"][0].astype(np.longdouble) - ref))) <= bound
    ref_zf = q.sequential(sos, x, dtype=np.longdouble)[1]
    zf_bound = q.allowance(name, chunk, 0, n) * max(float(np.max(np.abs(ref))), float(np.max(np.abs(ref_zf))))
    assert float(np.max(np.abs(second["zf"] - ref_zf))) <= zf_bound and float(np.max(np.abs(whole["zf"] - ref_zf))) <= zf_bound


def test_sosfilt_split_is_exact_on_integers(gpu):
    sos, x = q.EXACT["mix"][None], q.exact_signal(203)
    zi = np.array([[[1.0, 2.0], [3.0, 4.0]]])
    first = run_twice(gpu, sos, x[:77], chunk=7, zi=zi, want_zf=True)
    second = run_twice(gpu, sos, x[77:], chunk=4, zi=first["zf"], want_zf=True)
    want, want_zf = q.sequential(sos, x, zi=zi)
    assert q.same_bits(np.concatenate([first["y64"], second["y64"]], axis=1), want) and q.same_bits(second["zf"], want_zf)


@pytest.mark.parametrize("at", [0, 1234, 64 * 20 - 1, 64 * 20, 4999])
def test_sosfilt_nan_reaches_forward_only(gpu, at):
    names, sos, sig = q.bank(12, "bank_shared")
    assert (sos[:, :, 0] != 0).all()
    n = 5000
    x = q.signals()[0, :n].copy()
    clean = run_twice(gpu, sos, x, "f32", "both", 64)
    x[at] = np.nan
    got = run_twice(gpu, sos, x, "f32", "both", 64, want_zf=True, nonfinite=True)
    for k in ("y64", "y32"):
        assert q.same_bits(got[k][:, :at], clean[k][:, :at]), f"{k}: an output before the NaN changed"
        assert np.isnan(got[k][:, at:]).all(), f"{k}: a finite output after the NaN"
    assert np.isnan(got["zf"]).all()


def test_sosfilt_empty_signal(gpu):
    """n == 0 with every pointer valid: success, zf = zi (0 without zi), y and the workspace untouched."""
    sos = q.filters()["lp100"][None]
    zi = np.array([[[1.0, 2.0], [3.0, 4.0]]])
    with torch.cuda.device(gpu):
        g = Guard(gpu)
        a = dict(windows(g, sos, np.ones(1), "f64", 0, zi), n=0)
        y, zf, zf0 = g.out((1, 1), "y64", torch.float64), g.out((1, 2, 2), "zf", torch.float64), g.out((1, 2, 2), "zf0", torch.float64)
        assert sos_call(gpu, dict(a, y64=y, zf=zf)) == 0 and sos_call(gpu, dict(a, y64=y, zf=zf0, zi=None)) == 0
        assert sos_call(gpu, dict(a, y64=y)) == 0
        g.check(written=["zf", "zf0"])
        assert g.untouched("y64") and g.untouched("ws")
        assert q.same_bits(zf.cpu().numpy(), zi) and q.same_bits(zf0.cpu().numpy(), np.zeros((1, 2, 2)))


def test_sosfilt_refusals_leave_the_outputs_untouched(gpu):
    lib = _lib.load()
    names, sos, _ = q.bank(2, "bank_shared")
    x = q.signals()[0, :300]
    with torch.cuda.device(gpu):
        g = Guard(gpu)
        a = windows(g, sos, x.astype(np.float64), "f64", 64)
        other = g.inp(x, "x.other", torch.float32)
        bad = [dict(ns=0), dict(ns=17), dict(F=0), dict(F=65), dict(n_signals=2), dict(n_signals=0), dict(n=-1), dict(chunk=-1),
               dict(chunk=65537), dict(x32=other), dict(x64=None), dict(y64=None), dict(sos=None), dict(ws=None)]
        for i, kw in enumerate(bad):
            out = dict(y64=g.out((3, 300), f"y64.{i}", torch.float64), zf=g.out((3, 2, 2), f"zf.{i}", torch.float64))
            assert sos_call(gpu, dict(dict(a, **out), **kw)) == EINVAL, kw
            assert g.untouched(f"y64.{i}") and g.untouched(f"zf.{i}") and g.untouched("ws"), kw
        g.check()
    assert lib.maua_sosfilt_ws_doubles(3, 0, 300, 64) == -1 and lib.maua_sosfilt_ws_doubles(65, 2, 300, 64) == -1
    assert lib.maua_sosfilt_ws_doubles(3, 2, 300, 64) == 3 * (16 + 2 * 5 * 4) and lib.maua_sosfilt_ws_doubles(3, 2, 0, 64) == 3 * 16
    lengths = (0, 1, 32768, 32769, 131073, 5292000, 1 << 30)
    assert [lib.maua_sosfilt_default_chunk(n) for n in lengths] == [q.default_chunk(n) for n in lengths] == [64, 64, 64, 128, 256, 1024, 4096]


def test_sosfilt_is_capturable(gpu):
    """Captured once and replayed twice on new input in the same buffers: each replay has the bits of the eager call."""
    names, sos, sig = q.bank(12, "bank_own")
    n, chunk = 5000, 64
    stream = torch.cuda.Stream(gpu)
    inputs = [q.signals()[:, :n], q.signals()[::-1, 7000:7000 + n].copy()]
    with torch.cuda.device(gpu):
        g = Guard(gpu)
        a = windows(g, sos, inputs[0], "f32", chunk)
        cap = dict(y64=g.out((3, n), "y64.graph", torch.float64), y32=g.out((3, n), "y32.graph", torch.float32),
                   zf=g.out((3, 12, 2), "zf.graph", torch.float64))
        assert sos_call(gpu, dict(a, **cap)) == 0
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            with _lib.HipGraph() as graph:
                rc = sos_call(gpu, dict(a, **cap))
            assert rc == 0
            replays = []
            for k, x in enumerate(inputs):
                a["x32"].copy_(torch.from_numpy(x).to(gpu))
                stream.synchronize()
                graph.replay()
                stream.synchronize()
                replays.append({key: v.cpu().numpy() for key, v in cap.items()})
                eager = dict(y64=g.out((3, n), f"y64.e{k}", torch.float64), y32=g.out((3, n), f"y32.e{k}", torch.float32),
                             zf=g.out((3, 12, 2), f"zf.e{k}", torch.float64))
                assert sos_call(gpu, dict(a, **eager)) == 0
                stream.synchronize()
                for key in cap:
                    assert q.same_bits(replays[-1][key], eager[key].cpu().numpy()), key
        torch.cuda.synchronize()
        g.check(written=[f"{key}.{tag}" for tag in ("graph", "e0", "e1") for key in ("y64", "y32", "zf")])
    assert not q.same_bits(replays[0]["y64"], replays[1]["y64"])
    for f, name in enumerate(names):
        ref = q.longdouble(name, f)[:n]
        assert float(np.max(np.abs(replays[0]["y64"][f].astype(np.longdouble) - ref))) <= q.allowance(name, chunk, f, n) * float(np.max(np.abs(ref)))


# --- every instance (n_sections 1 .. 16 have their own register arrays, v_readlane chains and strides) and every edge of the chunk grid;
# tests/test_iir_host.py proves through maua_sosfilt_plan that the lists reach them
@pytest.mark.parametrize("ns", q.ALL_NS)
def test_sosfilt_every_instance_on_integers(gpu, ns):
    """A bank of two rotations of the integer cascade over their own signals, with and without zi: y, its float rounding and zf have
    the bits of the sequential loop."""
    sos, x, zi = q.instance_case(ns)
    for z in (None, zi):
        want, want_zf = q.sequential(sos, x, zi=z)
        for i, chunk in enumerate(q.INSTANCE_CHUNKS):
            got = run_twice(gpu, sos, x, ("f32", "f64")[(ns + i) % 2], "both", chunk, zi=z, want_zf=True)
            assert q.same_bits(got["y64"], want), f"chunk {chunk}: y"
            assert q.same_bits(got["y32"], want.astype(np.float32)), f"chunk {chunk}: the float y"
            assert q.same_bits(got["zf"], want_zf), f"chunk {chunk}: zf"


@pytest.mark.parametrize("ns", q.ALL_NS)
def test_sosfilt_every_instance_against_long_double(gpu, ns):
    """The three Butterworth band-passes of n_sections sections over one signal and over their own, judged as `judge` does."""
    sos = q.bp_bank(ns)
    names = [f"butter({ns}, {list(band)})" for band in q.BP_BANDS]
    worst, turn = 0.0, ns
    for mode in q.BP_MODES:
        sig = q.bp_signals(mode)
        x = q.signals()[0, :q.BP_N] if mode == "bank_shared" else q.signals()[list(sig), :q.BP_N]
        refs = [q.bp_longdouble(ns, band, s) for band, s in enumerate(sig)]
        for chunk in q.BP_CHUNKS:
            inp, outp = q.IO[turn % len(q.IO)]
            turn += 1
            allows = [q.bp_allowance(ns, band, s, chunk) for band, s in enumerate(sig)]
            got = run_twice(gpu, sos, x, inp, outp, chunk)
            worst = max(worst, judge_bank(gpu, got, names, refs, allows, q.BP_N, chunk, inp, outp, sos, x))
    print(f"n_sections {ns}: worst |y - long double| / allowance = {worst:.3f}")


@pytest.mark.parametrize("name", list(q.GEOMETRY))
def test_sosfilt_chunk_grid(gpu, name):
    """One class of the chunk grid on integers, from a non-zero state where the class has one: both outputs and zf bit for bit; the
    class's turn of single output type as well."""
    case = q.GEOMETRY[name]
    sos, x, zi = q.geometry_operands(name)
    want, want_zf = q.geometry_reference(name)
    inp, outp = q.IO[list(q.GEOMETRY).index(name) % len(q.IO)]
    if name == "largest_chunk":  # (a serial walk of 65 536 samples per lane: one call pair)
        inp, outp = "f32", "both"
    for o in sorted({"both", outp}):
        got = run_twice(gpu, sos, x, inp, o, case["chunk"], zi=zi, want_zf=True)
        if "y64" in got:
            assert q.same_bits(got["y64"], want), f"{inp}->{o}: y"
        if "y32" in got:
            assert q.same_bits(got["y32"], want.astype(np.float32)), f"{inp}->{o}: the float y"
        assert q.same_bits(got["zf"], want_zf), f"{inp}->{o}: zf"


# ------------------------------------------------------------------------------------------------ maua_env_follow_f32
def follow_call(gpu, x, y, T, C, ca, cr, y0=None):
    return _lib.load().maua_env_follow_f32(None if x is None else x.data_ptr(), None if y0 is None else y0.data_ptr(),
                                           None if y is None else y.data_ptr(), T, C, ca, cr, _lib.stream_ptr(gpu))


def follow_twice(gpu, x, ca, cr, y0=None, nonfinite=False):
    T, C = x.shape
    with torch.cuda.device(gpu):
        g = Guard(gpu)
        xd = g.inp(x, "x")
        y0d = None if y0 is None else g.inp(y0, "y0")
        outs = [g.out((T, C), f"y.{tag}") for tag in ("a", "b")]
        for out in outs:
            assert follow_call(gpu, xd, out, T, C, ca, cr, y0d) == 0
        g.check(written=["y.a", "y.b"], nonfinite_ok=["y.a", "y.b"] if nonfinite else ())
        a, b = (o.cpu().numpy() for o in outs)
    assert q.same_bits(a, b)
    return a


@pytest.mark.parametrize("C", [1, 3, 64, 65])
@pytest.mark.parametrize("T", [1, 2, 1000])
def test_follower_bit_for_bit(gpu, T, C):
    rng = np.random.default_rng(T * 100 + C)
    x = np.abs(rng.standard_normal((T, C))).astype(np.float32)
    ca, cr = float(np.float32(0.6321205588)), float(np.float32(0.1175030974))
    assert q.same_bits(follow_twice(gpu, x, ca, cr), q.follower(x, ca, cr))
    y0 = rng.standard_normal(C).astype(np.float32)
    assert q.same_bits(follow_twice(gpu, x, ca, cr, y0), q.follower(x, ca, cr, y0))


def test_follower_step_response(gpu):
    """A step up and down with attack 1/2 and release 1/4: the values are exact binary fractions."""
    x = np.array([0, 1, 1, 0, 0], np.float32)[:, None].repeat(2, 1)
    y = follow_twice(gpu, x, 0.5, 0.25)
    assert y[:, 0].tolist() == [0.0, 0.5, 0.75, 0.5625, 0.421875] and q.same_bits(y[:, 0], y[:, 1])
    assert q.same_bits(follow_twice(gpu, x, 1.0, 1.0), x)
    assert follow_twice(gpu, x, 0.0, 0.0, np.array([3, -2], np.float32)).tolist() == [[3.0, -2.0]] * 5


def test_follower_nan_stays_in_its_column(gpu):
    x = np.abs(np.random.default_rng(8).standard_normal((100, 5))).astype(np.float32)
    clean = follow_twice(gpu, x, 0.5, 0.1)
    x[40, 2] = np.nan
    y = follow_twice(gpu, x, 0.5, 0.1, nonfinite=True)
    assert np.isnan(y[40:, 2]).all() and q.same_bits(y[:40], clean[:40])
    assert q.same_bits(np.delete(y, 2, axis=1), np.delete(clean, 2, axis=1))


def test_follower_refusals(gpu):
    with torch.cuda.device(gpu):
        g = Guard(gpu)
        x = g.inp(np.ones((4, 3), np.float32), "x")
        y = g.out((4, 3), "y")
        for kw in (dict(x=None), dict(y=None), dict(T=-1), dict(C=0), dict(ca=-0.1), dict(ca=1.5), dict(cr=float("nan")), dict(cr=2.0)):
            a = dict(dict(x=x, y=y, T=4, C=3, ca=0.5, cr=0.5), **kw)
            assert follow_call(gpu, a["x"], a["y"], a["T"], a["C"], a["ca"], a["cr"]) == EINVAL, kw
            assert g.untouched("y"), kw
        assert follow_call(gpu, x, y, 0, 3, 0.5, 0.5) == 0 and g.untouched("y")
        g.check()
