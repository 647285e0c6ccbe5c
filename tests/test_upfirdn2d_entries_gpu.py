"""GPU: every instance of maua_upfirdn2d_f32 through the C ABI, between red zones, against the float64 reference.

The cases are tests/upfirdn_cases.py; tests/test_upfirdn2d_entries_host.py proves on the CPU, through maua_upfirdn2d_plan_instance, that they
reach all 16 kernels behind the entry (fir_tile_kernel<2 | 3 | 4 taps, WX 1 | 2 | 4>, fir_up2_kernel<WX>, fir_down2_kernel<WX>,
fir_generic_kernel), each tiled one with a second, partial tile row, a whole-tile height, a second plane of odd size and pad_x0 != pad_y0.
The tiled kernels address memory through raw buffer descriptors whose row offset is a scalar the range check does not see: only their own
row tests keep an access inside its plane, which is what the red zones (tests/redzone.py) and the canary-filled outputs are for.

Every case runs with two kinds of operands:
  integers  x in -8 .. 8, k in -4 .. 4: every product and partial sum is exact in fp32 (the host test proves sum |k||x| < 2^24), so the
            result must EQUAL the float64 reference, every element — tap flips, phases, pad parities, crops, seams, all-padding tiles;
  reals     x ~ N(0, 1), k ~ 0.5 N(0, 1): |got - want| <= (kh kw + 2) 2^-24 upfirdn_ref(|x|, |k|) elementwise (upfirdn_ref.py
            reference_and_bound: derived from the kernels' one fma chain per output, not measured).
Each runs twice into separate windows (identical bits), then Guard.check: red zones intact, every output written and finite.  The line
printed per case names the instance; the last test prints the worst error / bound per instance."""
import numpy as np
import pytest
import torch

from maua_stylegan2_amd import _lib
from redzone import CANARY_BITS, Guard
from upfirdn_cases import CASES, REFUSED, integer_operands, real_operands
from upfirdn_ref import reference_and_bound, upfirdn_out_shape

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

EINVAL = -22
WORST = {}  # instance -> (worst error / bound over the real-valued runs, case)
# one case per tiled family with three planes / for the skewed windows (up2: an even width, so the 8-byte stores sit on 4-byte
# aligned, not 8-byte aligned, addresses) / for the capture
THREE_PLANES = ["tile4_two_tile_rows_w64", "up2_34x130", "down2_17x65"]
SKEWED = ["tile3_wx2_rows", "up2_66x128", "down2_wx4_rows"]
CAPTURED = ["tile4_w257", "up2_wx2_rows", "down2_33x64"]


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def instance(case):
    rc, name, _, _ = _lib.planned_upfirdn2d_instance(*case)
    assert rc == 0, rc
    return name


def call(gpu, case, xt, kt, yt):
    return _lib.load().maua_upfirdn2d_f32(_lib.ptr(xt), _lib.ptr(kt), _lib.ptr(yt), *case, _lib.stream_ptr(gpu))


def skewed(g, shape, name, data=None):
    """A window that starts one float into a 16-byte aligned buffer; returns (window, whole buffer)."""
    n = int(np.prod(shape))
    full = g.out((n + 1,), name)
    assert full.data_ptr() % 16 == 0
    if data is not None:
        full[1:].copy_(torch.from_numpy(data.reshape(-1)))
    return full[1:].view(shape), full


def run(gpu, case, x, k, skew=False, nonfinite_ok=False):
    """Two launches into separate output windows: identical bits, red zones intact, everything written (and finite).  -> y as numpy."""
    shape = upfirdn_out_shape(case)
    g = Guard(gpu)
    kt = g.inp(k, "k")
    if skew:
        (xt, xfull), (y0, y0full), (y1, y1full) = skewed(g, x.shape, "x", x), skewed(g, shape, "y0"), skewed(g, shape, "y1")
        assert xt.data_ptr() % 16 == 4 and y0.data_ptr() % 16 == 4
    else:
        xt, y0, y1 = g.inp(x, "x"), g.out(shape, "y0"), g.out(shape, "y1")
    assert call(gpu, case, xt, kt, y0) == 0 and call(gpu, case, xt, kt, y1) == 0
    # (a skewed window is checked by hand: Guard would count the float in front of it as unwritten)
    g.check(written=() if skew else ("y0", "y1"), nonfinite_ok=("y0", "y1") if nonfinite_ok else ())
    got, again = y0.cpu().numpy(), y1.cpu().numpy()
    if skew:
        for full in (xfull, y0full, y1full):
            assert bool((full[:1].view(torch.int32) == CANARY_BITS).all()), "write in front of a skewed window"
        assert not (bits(got) == CANARY_BITS).any() and np.isfinite(got).all()
    assert np.array_equal(bits(got), bits(again)), "two runs of one call differ"
    return got


@pytest.mark.parametrize("name", list(CASES))
def test_integer_operands_equal_the_float64_reference(gpu, name):
    case = CASES[name]
    x, k = integer_operands(case)
    want, _ = reference_and_bound(x, k, case[6:])
    got = run(gpu, case, x, k)
    assert got.shape == want.shape
    bad = int((got.astype(np.float64) != want).sum())
    print(f"[upfirdn2d_f32] {name} {instance(case)} integers: {bad} of {want.size} outputs differ")
    assert bad == 0, (name, instance(case), bad, np.argwhere(got.astype(np.float64) != want)[:8].tolist())


@pytest.mark.parametrize("name", list(CASES))
def test_real_operands_within_the_derived_bound(gpu, name):
    case = CASES[name]
    x, k = real_operands(case)
    want, bound = reference_and_bound(x, k, case[6:])
    got = run(gpu, case, x, k)
    err = np.abs(got.astype(np.float64) - want)
    with np.errstate(divide="ignore", invalid="ignore"):
        ratio = np.where(bound > 0, err / bound, np.where(err > 0, np.inf, 0.0))
    worst, inst = float(ratio.max()), instance(case)
    if worst >= WORST.get(inst, (-1.0, None))[0]:
        WORST[inst] = (worst, name)
    print(f"[upfirdn2d_f32] {name} {inst} reals: worst error / bound {worst:.4f} (max error {float(err.max()):.3e})")
    assert worst <= 1.0, (name, inst, worst)


@pytest.mark.parametrize("name", THREE_PLANES)
def test_planes_are_isolated(gpu, name):
    """The middle plane of x all NaN: planes 0 and 2 of the output keep the bits of the clean run."""
    case = CASES[name]
    assert case[0] == 3 and instance(case) != "generic"
    x, k = real_operands(case)
    clean = run(gpu, case, x, k)
    x[1] = np.nan
    got = run(gpu, case, x, k, nonfinite_ok=True)
    assert np.array_equal(bits(got[0]), bits(clean[0])) and np.array_equal(bits(got[2]), bits(clean[2]))
    assert np.isfinite(got[0]).all() and np.isfinite(got[2]).all()


@pytest.mark.parametrize("name", SKEWED)
def test_four_byte_alignment_is_enough(gpu, name):
    """x and y each one float into a 16-byte aligned buffer: the bits of the aligned run, and the skipped floats keep the canary."""
    case = CASES[name]
    inst = instance(case)
    assert inst != "generic" and (not inst.startswith("up2") or upfirdn_out_shape(case)[2] % 2 == 0)
    for operands in (integer_operands, real_operands):
        x, k = operands(case)
        assert np.array_equal(bits(run(gpu, case, x, k, skew=True)), bits(run(gpu, case, x, k)))


def test_refusals_leave_the_output_untouched(gpu):
    good = CASES["tile4_tiny"]
    g = Guard(gpu)
    x, k = real_operands(good)
    xt, kt, y = g.inp(x, "x"), g.inp(k, "k"), g.out(upfirdn_out_shape(good), "y")
    assert call(gpu, good, None, kt, y) == EINVAL and call(gpu, good, xt, None, y) == EINVAL and call(gpu, good, xt, kt, None) == EINVAL
    for why, case in REFUSED.items():  # (pointers of a good call: a refused geometry reads and writes nothing)
        assert call(gpu, case, xt, kt, y) == EINVAL, why
    assert g.untouched("y")
    g.check()
    assert call(gpu, good, xt, kt, y) == 0  # (the same buffers do serve the good call)
    g.check(written=("y",))


@pytest.mark.parametrize("name", CAPTURED)
def test_the_call_is_capturable(gpu, name):
    """Captured into a hipGraph and replayed on new input in the same buffers: the replay equals the eager call bit for bit."""
    case = CASES[name]
    assert instance(case) != "generic"
    x, k = real_operands(case)
    other = np.ascontiguousarray(x[:, ::-1] * np.float32(0.75))
    shape = upfirdn_out_shape(case)
    stream = torch.cuda.Stream(gpu)
    with torch.cuda.device(gpu):
        g = Guard(gpu)
        xt, kt = g.inp(x, "x"), g.inp(k, "k")
        eager0, eager1, captured = g.out(shape, "eager0"), g.out(shape, "eager1"), g.out(shape, "graph")
        assert call(gpu, case, xt, kt, eager0) == 0
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            with _lib.HipGraph() as graph:
                rc = _lib.load().maua_upfirdn2d_f32(xt.data_ptr(), kt.data_ptr(), captured.data_ptr(), *case, _lib.stream_ptr())
            assert rc == 0
            graph.replay()
            stream.synchronize()
            first = captured.cpu().numpy()
            xt.copy_(torch.from_numpy(other).to(gpu))
            graph.replay()
            stream.synchronize()
            second = captured.cpu().numpy()
        torch.cuda.synchronize()
        assert call(gpu, case, xt, kt, eager1) == 0
        g.check(written=("eager0", "eager1", "graph"))
        assert np.array_equal(bits(first), bits(eager0.cpu().numpy())) and np.array_equal(bits(second), bits(eager1.cpu().numpy()))
    assert not np.array_equal(first, second)


def test_worst_ratio_per_instance_is_printed():
    """Runs last in the file: the table of the real-valued runs above (empty when they were deselected)."""
    for inst in sorted(WORST):
        print(f"[upfirdn2d_f32] worst error / bound of {inst}: {WORST[inst][0]:.4f} ({WORST[inst][1]})")
    assert all(w <= 1.0 for w, _ in WORST.values())
