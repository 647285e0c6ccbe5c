"""GPU: maua_yin_f32 (csrc/pitch.hip) called through the C ABI between red zones, over the case list of tests/pitch_ref.py, against the
float64 definition there.

Every case runs three times into separate output windows — twice with the d' output (identical bits required, d' included), once with
cmndf = NULL (identical lag / tau_int / aperiodicity) — and ends with Guard.check: red zones intact, every output element written,
every output finite.  d' is compared at its tolerance with no element exempt; tau_int exactly, lag and aperiodicity at their tolerances,
on every frame whose pick the float64 reference decides by more than twice the d' tolerance (decided before the kernel runs; the host
test shows that at most one frame per case is exempt, and none on the exact signals).  The tolerances are those of pitch_ref.py: 4 x the
error of an all-fp32 emulation over this same list, never the kernel's."""
import numpy as np
import pytest
import torch

import pitch_ref as pr
from maua_stylegan2_amd import _lib
from redzone import Guard

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

EINVAL = -22
CASES = pr.gpu_cases()
OUTPUTS = ("lag", "aperiodicity", "tau_int")


def windows(g, case, tag, with_cmndf=True):
    """Fresh guarded output windows named ``<output>.<tag>``, of the size the valid call of ``case`` needs."""
    rows = 1 + case["n_samples"] // case["hop"]
    out = {"lag": g.out((rows,), f"lag.{tag}"), "aperiodicity": g.out((rows,), f"aperiodicity.{tag}"),
           "tau_int": g.out((rows,), f"tau_int.{tag}", torch.int32)}
    if with_cmndf:
        out["cmndf"] = g.out((rows, case["tau_max"] + 1), f"cmndf.{tag}")
    return out


def call(y_dev, case, out, **override):
    a = dict(case, **override)
    n = y_dev.numel()
    n_frames = a.get("n_frames", 1 + n // a["hop"] if a["hop"] > 0 else out["lag"].numel())
    return _lib.load().maua_yin_f32(y_dev.data_ptr(), n, a["frame"], a["hop"], a["tau_min"], a["tau_max"], a["threshold"], out["lag"].data_ptr(),
                                    out["aperiodicity"].data_ptr(), out["tau_int"].data_ptr(), _lib.ptr(out.get("cmndf")), n_frames,
                                    _lib.stream_ptr(y_dev.device))


def launch(g, y_dev, case, tag, with_cmndf=True, **override):
    """One call into fresh guarded windows -> (rc, {output: device view})."""
    out = windows(g, case, tag, with_cmndf)
    return call(y_dev, case, out, **override), out


def host(out):
    return {k: v.cpu().numpy() for k, v in out.items()}


def bits(a):
    return np.ascontiguousarray(a).view(np.int32)


@pytest.mark.parametrize("case", CASES, ids=pr.case_id)
def test_entry_against_float64(gpu, case):
    ref = pr.reference(case)  # (and with it which frames are unambiguous) before the kernel runs
    with torch.cuda.device(gpu):
        g = Guard(gpu)
        y = g.inp(pr.make_signal(case), "y")
        runs = []
        for tag, with_cmndf in (("a", True), ("b", True), ("null", False)):
            rc, out = launch(g, y, case, tag, with_cmndf)
            assert rc == 0, (tag, rc)
            runs.append(out)
        g.check(written=[f"{k}.{tag}" for tag, out in zip(("a", "b", "null"), runs) for k in out])
    a, b, null = (host(r) for r in runs)
    for key in OUTPUTS + ("cmndf",):
        assert np.array_equal(bits(a[key]), bits(b[key])), f"{key}: two runs differ"
    for key in OUTPUTS:
        assert np.array_equal(bits(a[key]), bits(null[key])), f"{key}: differs with cmndf = NULL"
    assert ((a["tau_int"] >= case["tau_min"]) & (a["tau_int"] <= case["tau_max"])).all()
    figures = pr.worst(a, ref, scaled=case["short"])
    print(f"[{pr.case_id(case)}] cmndf {figures[0]:.3g}  lag {figures[1]:.3g}  aperiodicity {figures[2]:.3g}  "
          f"({int((~pr.unambiguous(ref)).sum())} of {len(ref['lag'])} frames ambiguous)")
    if case["signal"] == "zeros":  # bit for bit
        assert (a["cmndf"] == 1).all() and (a["tau_int"] == case["tau_min"]).all() and (a["aperiodicity"] == 1).all()
        assert (a["lag"] == case["tau_min"]).all()
    assert pr.compare(a, ref, *pr.tolerances(case), scaled=case["short"]) == []


NONFINITE = [c for c in CASES if c["signal"] in pr.NOISY_SIGNALS and 1 + c["n_samples"] // c["hop"] >= 5][:4]


@pytest.mark.parametrize("case", NONFINITE, ids=pr.case_id)
@pytest.mark.parametrize("poison", [float("nan"), float("inf")], ids=["nan", "inf"])
def test_a_non_finite_sample_stays_inside_the_frames_that_cover_it(gpu, case, poison):
    y = pr.make_signal(case)
    at = (2 * len(y)) // 3
    bad = y.copy()
    bad[at] = poison
    span = case["frame"] + case["tau_max"]
    starts = np.arange(1 + len(y) // case["hop"], dtype=np.int64) * case["hop"] - span // 2
    clear = ~((starts <= at) & (at < starts + span))
    assert clear.any() and (~clear).any()
    with torch.cuda.device(gpu):
        g = Guard(gpu)
        rc0, clean = launch(g, g.inp(y, "y"), case, "clean")
        rc1, dirty = launch(g, g.inp(bad, "bad"), case, "dirty")
        assert rc0 == 0 and rc1 == 0
        g.check(written=[f"{k}.{tag}" for tag in ("clean", "dirty") for k in OUTPUTS + ("cmndf",)],
                nonfinite_ok=[f"{k}.dirty" for k in OUTPUTS + ("cmndf",)])
    clean, dirty = host(clean), host(dirty)
    assert ((dirty["tau_int"] >= case["tau_min"]) & (dirty["tau_int"] <= case["tau_max"])).all()
    for key in OUTPUTS + ("cmndf",):
        assert np.array_equal(bits(clean[key])[clear], bits(dirty[key])[clear]), f"{key}: a frame that does not cover the sample changed"


def test_refused_calls_leave_the_outputs_untouched(gpu):
    case = dict(frame=64, tau_min=2, tau_max=17, hop=7, n_samples=100, signal="tone20", threshold=0.1, seed=5, short=False)
    refused = [dict(frame=15), dict(frame=4097), dict(tau_min=0), dict(tau_min=17), dict(tau_max=2049), dict(hop=0), dict(threshold=-0.5),
               dict(threshold=float("nan")), dict(n_frames=14), dict(n_frames=16)]
    with torch.cuda.device(gpu):
        g = Guard(gpu)
        y = g.inp(pr.make_signal(case), "y")
        for i, kw in enumerate(refused):
            rc, _ = launch(g, y, case, f"r{i}", **kw)
            assert rc == EINVAL, kw
            for key in OUTPUTS + ("cmndf",):
                assert g.untouched(f"{key}.r{i}"), (kw, key)
        rc, _ = launch(g, y[:0], case, "empty", n_frames=1)  # n_samples = 0
        assert rc == EINVAL and all(g.untouched(f"{key}.empty") for key in OUTPUTS + ("cmndf",))
        g.check()


def test_the_call_is_capturable(gpu):
    """Captured into a hipGraph and replayed on new input in the same buffers: the replay equals the eager call bit for bit."""
    case = dict(frame=1000, tau_min=10, tau_max=340, hop=512, n_samples=4000, signal="tone20", threshold=0.1, seed=9, short=False)
    other = dict(case, seed=10, signal="glide")
    stream = torch.cuda.Stream(gpu)
    with torch.cuda.device(gpu):
        g = Guard(gpu)
        y = g.inp(pr.make_signal(case), "y")
        rc, eager_first = launch(g, y, case, "eager0")
        assert rc == 0
        captured = windows(g, case, "graph")
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            with _lib.HipGraph() as graph:
                rc = call(y, case, captured)
            assert rc == 0
            graph.replay()
            stream.synchronize()
            first = host(captured)
            y.copy_(torch.from_numpy(pr.make_signal(other)).to(gpu))
            graph.replay()
            stream.synchronize()
            second = host(captured)
        torch.cuda.synchronize()
        rc, eager_second = launch(g, y, other, "eager1")
        assert rc == 0
        g.check(written=[f"{k}.{tag}" for tag in ("eager0", "graph", "eager1") for k in OUTPUTS + ("cmndf",)])
    for got, want in ((first, host(eager_first)), (second, host(eager_second))):
        for key in OUTPUTS + ("cmndf",):
            assert np.array_equal(bits(got[key]), bits(want[key])), key
    assert not np.array_equal(first["lag"], second["lag"])
