"""GPU: the two predominant-local-pulse entries (csrc/pulse.hip) called through the C ABI between red zones, over the case lists of
tests/pulse_ref.py.

maua_tempogram_peak_f32 against the float64 restatement on the same float32 operands: S, power and phase within 4 x the float32
emulation's error (asserted under the derived ceilings, printed per case), bins exact except on the frames — decided on the CPU before
the kernel runs, at most 2 % of a case — whose two best scores lie within twice the ceiling of each other; bit for bit on integer
operands; the shift property; a NaN reaches exactly the frames whose window covers it.  maua_pulse_synth_f32 on host-built (bin, phase)
against the float64 restatement.  Every case ends with Guard.check: red zones intact, every output element written; two runs agree bit
for bit; refusals leave the outputs untouched; both entries in one captured graph replay to the eager bits."""
import numpy as np
import pytest
import torch

import pulse_ref as q
from maua_stylegan2_amd import _lib
from redzone import Guard

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

EINVAL = -22
A_OUT = ("bin", "phase", "power")


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def host(out):
    return {k: (None if v is None else v.cpu().numpy()) for k, v in out.items()}


# ------------------------------------------------------------------------------------------------ entry A
def a_windows(g, n, n_tempi, tgram, tag):
    return {"bin": g.out((n,), f"bin.{tag}", torch.int32), "phase": g.out((n,), f"phase.{tag}"), "power": g.out((n,), f"power.{tag}"),
            "tgram": g.out((n, n_tempi), f"tgram.{tag}") if tgram else None}


def a_call(env, table, prior, out, n, win, n_tempi, null=None):
    ptr = lambda name, t: None if (t is None or null == name) else t.data_ptr()  # noqa: E731
    return _lib.load().maua_tempogram_peak_f32(ptr("env", env), n, ptr("table", table), win, n_tempi, ptr("prior", prior), ptr("bin", out["bin"]),
                                               ptr("phase", out["phase"]), ptr("power", out["power"]), ptr("tgram", out["tgram"]),
                                               _lib.stream_ptr(env.device))


def run_a(gpu, env, table, prior, tgram, runs=1, nonfinite=False):
    """The outputs of ``runs`` calls on guarded copies of the operands, checked for stray writes and unwritten elements."""
    n, (n_tempi, win, _) = len(env), table.shape
    with torch.cuda.device(gpu):
        g = Guard(gpu)
        env_d, table_d = g.inp(env, "env"), g.inp(table, "table")
        prior_d = None if prior is None else g.inp(prior, "prior")
        outs = []
        for i in range(runs):
            out = a_windows(g, n, n_tempi, tgram, str(i))
            assert a_call(env_d, table_d, prior_d, out, n, win, n_tempi) == 0
            outs.append(out)
        names = [f"{k}.{i}" for i in range(runs) for k in A_OUT + (("tgram",) if tgram else ())]
        g.check(written=names, nonfinite_ok=[f"tgram.{i}" for i in range(runs)] if nonfinite else ())
        return [host(o) for o in outs]


def check_a_case(gpu, case):
    env, table, prior, ref, tol = q.a_reference(case)  # (asserts the exempt cap with the reference alone)
    a, b = run_a(gpu, env, table, prior, bool(case.get("tgram")), runs=2)
    for key in A_OUT + ("tgram",):
        assert (a[key] is None and b[key] is None) or same_bits(a[key], b[key]), f"{key}: two runs differ"
    print(f"[{q.case_id(case)}] tolerance = 4 x {tol[0]:.3g} of the S ceiling, 4 x {tol[1]:.3g} of the phase ceiling + 4 x {tol[2]:.3g} rad; "
          f"{int(ref['exempt'].sum())} of {case['n']} frames exempt, {int((a['bin'] != ref['bin']).sum())} bins differ")
    assert q.compare_peak(a, ref, tol) == []


@pytest.mark.parametrize("case", q.a_cases(), ids=q.case_id)
def test_tempogram_peak_against_float64(gpu, case):
    check_a_case(gpu, case)


def test_tempogram_peak_twenty_thousand_frames(gpu):
    check_a_case(gpu, q.LONG_CASE)


@pytest.mark.parametrize("n,win,n_tempi,prior", [(2 * q.TILE + 5, 33, 6, False), (q.TILE, 384, 65, False), (q.TILE + 1, 384, 5, True), (7, 2, 2, False)])
def test_tempogram_peak_is_exact_on_integers(gpu, n, win, n_tempi, prior):
    """Integer envelope, a table of 0 and +-1 (window of ones, omega = 0 and pi / 2), a prior of powers of two: every float32 operation is
    exact, so S equals the float64 restatement bit for bit and the bins — ties included — are the definition's."""
    case = dict(n=n, win=win, n_tempi=n_tempi, kind="integer", seed=n + win, grid="integer")
    env, table = q.make_env(case), q.case_table(case)
    p = (2.0 ** -(np.arange(n_tempi) % 3)).astype(np.float32) if prior else None
    ref = q.tempogram_peak(env, table, p, exact=True)
    assert np.array_equal(q.emulate_peak(env, table, p)[2].astype(np.float64), ref["S"])
    (got,) = run_a(gpu, env, table, p, True)
    assert same_bits(got["tgram"], ref["S"].astype(np.float32))
    assert np.array_equal(got["bin"], ref["bin"]) and same_bits(got["power"], ref["power"].astype(np.float32))
    assert q.compare_peak(got, ref, q.peak_tolerances(env, table, p, ref)) == []


@pytest.mark.parametrize("shift", [1, q.TILE - 1, q.TILE + 1])
def test_tempogram_peak_shift_property(gpu, shift):
    """``shift`` zeros in front of the envelope move every frame's outputs by ``shift`` frames and change no bit of them: clipped taps
    are added as zeros, and a frame's order of summation does not depend on its place in the tile or the launch."""
    case = dict(n=2 * q.TILE + 5, win=33, n_tempi=65, kind="random", seed=50)
    env, table, prior = q.make_env(case), q.case_table(case), q.case_prior(dict(case, prior=True))
    (base,) = run_a(gpu, env, table, prior, True)
    (moved,) = run_a(gpu, np.concatenate([np.zeros(shift, np.float32), env]), table, prior, True)
    for key in A_OUT + ("tgram",):
        assert same_bits(moved[key][shift:], base[key]), key
    assert np.all(moved["bin"][: shift - 33 // 2 if shift > 33 // 2 else 0] == -1)  # frames that see nothing but the new zeros


def test_a_nan_invalidates_exactly_the_frames_whose_window_covers_it(gpu):
    case = dict(n=2 * q.TILE + 5, win=33, n_tempi=65, kind="nan", seed=51, nan_at=70)
    env, table = q.make_env(case), q.case_table(case)
    clean = env.copy()
    clean[70] = 0.25
    (got,) = run_a(gpu, env, table, None, True, nonfinite=True)
    (want,) = run_a(gpu, clean, table, None, True)
    t = np.arange(case["n"])
    covered = (t - 33 // 2 <= 70) & (70 <= t - 33 // 2 + 32)
    assert covered.sum() == 33
    assert np.all(got["bin"][covered] == -1) and np.all(got["power"][covered] == 0) and np.all(got["phase"][covered] == 0)
    assert np.isnan(got["tgram"][covered]).all()
    for key in A_OUT + ("tgram",):
        assert same_bits(got[key][~covered], want[key][~covered]), key


def test_tempogram_peak_refusals_leave_the_outputs_untouched(gpu):
    case = dict(n=10, win=33, n_tempi=5, kind="random", seed=52)
    env, table = q.make_env(case), q.case_table(case)
    refused = ([dict(null=k) for k in ("env", "table", "bin", "phase", "power")]
               + [dict(n=0), dict(n=-1), dict(n=(1 << 22) + 1), dict(win=1), dict(win=0), dict(win=2049), dict(n_tempi=0), dict(n_tempi=1025)])
    with torch.cuda.device(gpu):
        g = Guard(gpu)
        env_d, table_d = g.inp(env, "env"), g.inp(table, "table")
        for i, kw in enumerate(refused):
            out = a_windows(g, 10, 5, True, f"r{i}")
            args = dict(n=10, win=33, n_tempi=5)
            args.update(kw)
            assert a_call(env_d, table_d, None, out, **args) == EINVAL, kw
            assert all(g.untouched(f"{k}.r{i}") for k in A_OUT + ("tgram",)), kw
        g.check()


# ------------------------------------------------------------------------------------------------ entry B
def b_call(bins, phase, window, omega, out, n, win, n_tempi, null=None):
    ptr = lambda name, t: None if null == name else t.data_ptr()  # noqa: E731
    return _lib.load().maua_pulse_synth_f32(ptr("bin", bins), ptr("phase", phase), n, ptr("window", window), win, ptr("omega", omega), n_tempi,
                                            ptr("pulse", out), _lib.stream_ptr(bins.device))


def run_b(gpu, bins, phase, window, omega, runs=1):
    with torch.cuda.device(gpu):
        g = Guard(gpu)
        ops = (g.inp(bins, "bin", torch.int32), g.inp(phase, "phase"), g.inp(window, "window"), g.inp(omega, "omega"))
        outs = []
        for i in range(runs):
            out = g.out((len(bins),), f"pulse.{i}")
            assert b_call(*ops, out, len(bins), len(window), len(omega)) == 0
            outs.append(out)
        g.check(written=[f"pulse.{i}" for i in range(runs)])
        return [o.cpu().numpy() for o in outs]


@pytest.mark.parametrize("case", q.b_cases(), ids=q.case_id)
def test_pulse_synth_against_float64(gpu, case):
    bins, phase, w, om = q.b_operands(case)
    ref = q.pulse_synth(bins, phase, w, om)
    tol = q.synth_tolerance(bins, phase, w, om, ref)  # (asserted under the ceiling)
    a, b = run_b(gpu, bins, phase, w, om, runs=2)
    assert same_bits(a, b), "two runs differ"
    print(f"[{q.case_id(case)}] tolerance {tol:.3g} (ceiling {q.synth_ceiling(len(w), om):.3g}), worst {np.abs(a.astype(np.float64) - ref).max():.3g}, "
          f"{int((ref == 0).sum())} zeros, largest {ref.max():.3f}")
    assert a.min() >= 0
    assert q.compare_pulse(a, ref, tol) == []
    if case["kind"] == "none" or (case.get("window") == "zero_middle" and case["n"] <= case["win"] // 4):
        assert not a.any()  # no tempo anywhere; den = 0 everywhere


def test_pulse_synth_refusals_leave_the_output_untouched(gpu):
    case = dict(n=10, win=33, n_tempi=5, kind="random", seed=53)
    bins, phase, w, om = q.b_operands(case)
    refused = ([dict(null=k) for k in ("bin", "phase", "window", "omega", "pulse")]
               + [dict(n=0), dict(n=-1), dict(n=(1 << 22) + 1), dict(win=1), dict(win=2049), dict(n_tempi=0), dict(n_tempi=1025)])
    with torch.cuda.device(gpu):
        g = Guard(gpu)
        ops = (g.inp(bins, "bin", torch.int32), g.inp(phase, "phase"), g.inp(w, "window"), g.inp(om, "omega"))
        for i, kw in enumerate(refused):
            out = g.out((10,), f"pulse.r{i}")
            args = dict(n=10, win=33, n_tempi=5)
            args.update(kw)
            assert b_call(*ops, out, **args) == EINVAL, kw
            assert g.untouched(f"pulse.r{i}"), kw
        g.check()


# ------------------------------------------------------------------------------------------------ both entries under capture
def test_both_entries_in_one_captured_graph(gpu):
    """Envelope -> (bin, phase) -> pulse captured into one hipGraph and replayed on a new envelope in the same buffers: each replay equals
    the eager calls bit for bit."""
    case = dict(n=2 * q.TILE + 5, win=384, n_tempi=271, kind="click", seed=60)
    other = dict(case, kind="random", seed=61)
    table, prior = q.case_table(case), q.case_prior(dict(case, prior=True))
    w, om = q.case_window(case).astype(np.float32), q.case_omega(case).astype(np.float32)
    n, win, n_tempi = case["n"], case["win"], case["n_tempi"]
    stream = torch.cuda.Stream(gpu)
    with torch.cuda.device(gpu):
        g = Guard(gpu)
        env_d, table_d, prior_d = g.inp(q.make_env(case), "env"), g.inp(table, "table"), g.inp(prior, "prior")
        w_d, om_d = g.inp(w, "window"), g.inp(om, "omega")
        cap, cap_pulse = a_windows(g, n, n_tempi, True, "graph"), g.out((n,), "pulse.graph")
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            with _lib.HipGraph() as graph:
                rc_a = a_call(env_d, table_d, prior_d, cap, n, win, n_tempi)
                rc_b = b_call(cap["bin"], cap["phase"], w_d, om_d, cap_pulse, n, win, n_tempi)
            assert rc_a == 0 and rc_b == 0
            replays = []
            for i, c in enumerate((case, other)):
                env_d.copy_(torch.from_numpy(q.make_env(c)).to(gpu))
                stream.synchronize()
                graph.replay()
                stream.synchronize()
                replays.append((host(cap), cap_pulse.cpu().numpy()))
                eager, eager_pulse = a_windows(g, n, n_tempi, True, f"eager{i}"), g.out((n,), f"pulse.eager{i}")
                assert a_call(env_d, table_d, prior_d, eager, n, win, n_tempi) == 0
                assert b_call(eager["bin"], eager["phase"], w_d, om_d, eager_pulse, n, win, n_tempi) == 0
                stream.synchronize()
                for key in A_OUT + ("tgram",):
                    assert same_bits(replays[-1][0][key], host(eager)[key]), key
                assert same_bits(replays[-1][1], eager_pulse.cpu().numpy())
        torch.cuda.synchronize()
        g.check(written=[f"{k}.{tag}" for tag in ("graph", "eager0", "eager1") for k in A_OUT + ("tgram", "pulse")])
    assert not same_bits(replays[0][1], replays[1][1])
    env = q.make_env(other)
    ref = q.tempogram_peak(env, table, prior)
    assert int(ref["exempt"].sum()) <= q.max_exempt(n)
    assert q.compare_peak(replays[1][0], ref, q.peak_tolerances(env, table, prior, ref)) == []
    want = q.pulse_synth(replays[1][0]["bin"], replays[1][0]["phase"], w, om)
    assert q.compare_pulse(replays[1][1], want, q.synth_tolerance(replays[1][0]["bin"], replays[1][0]["phase"], w, om, want)) == []
