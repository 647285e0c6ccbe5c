"""GPU: maua_feedback_f32 (csrc/feedback.hip) called through the C ABI between red zones (tests/redzone.py), against the numpy twin
tests/feedback_ref.py.

The definition fixes the order of every operation and fuses nothing, so the device is held to the float32 emulation BIT FOR BIT on dyadic
operands (image values on a 2^-8 grid, gains and tints powers of two, integer translations, quarter turns) and, on real operands, to
float64 within the allowance of feedback_ref (4 x the emulation's own error, a floor of 8 ulp of the value range; the host test holds it
under a derived ceiling).  No allowance is computed from the device's output."""
import ctypes
import itertools

import numpy as np
import pytest
import torch

import feedback_ref as fr
from maua_stylegan2_amd import _lib
from redzone import Guard

pytestmark = pytest.mark.gpu
F32, F64 = np.float32, np.float64
EINVAL, ENOSYS = -22, -38
COMBOS = list(itertools.product(fr.MODES, fr.BORDERS))


def _inp(g, a, name, skew=False):
    """``a`` in a guarded window; ``skew``: 4 bytes off a 16-byte boundary."""
    a = np.array(a, F32)  # (a copy: the shared operands are read-only)
    if not skew:
        t = g.inp(a, name)
        assert t.data_ptr() % 16 == 0
        return t
    return g.inp(np.concatenate([[F32(0)], a.reshape(-1)]), name)[1:].view(a.shape)


def _out(g, shape, name, skew=False):
    """An output window; ``skew``: one float further in, the float in front zeroed so that no canary is left once the rest is written."""
    if not skew:
        return g.out(shape, name)
    full = g.out((int(np.prod(shape)) + 1,), name)
    full[0] = 0
    return full[1:].view(shape)


def _bits(a):
    return np.ascontiguousarray(a, F32).view(np.uint32)


def _plan(batch, h, w, rows, img):
    plan = (ctypes.c_int * 8)()
    rows = np.ascontiguousarray(rows, F32)
    assert _lib.load().maua_feedback_plan(batch, h, w, rows.ctypes.data, rows.shape[1], img, ctypes.addressof(plan)) == 0
    return list(plan)


def _feedback(gpu, cur, rows, mode, border, splits=None, skew=False, in_place=False, state0=None, nonfinite=False):
    """Guarded calls over the frames cut at ``splits`` (the state carried in its buffer, state_valid 0 on the first call only unless
    ``state0`` is given) -> (out as numpy, the state as numpy, the launches planned per call)."""
    g = Guard(gpu)
    b, _, h, w = cur.shape
    rows = np.ascontiguousarray(rows, F32)
    img = _inp(g, cur, "img", skew)
    out = img if in_place else _out(g, cur.shape, "out", skew)
    state = _out(g, (3, h, w), "state", skew) if state0 is None else _inp(g, state0, "state", skew)
    edges = [0] + list(splits or ()) + [b]
    launches = []
    lib = _lib.load()
    for k, (lo, hi) in enumerate(zip(edges[:-1], edges[1:])):
        part = np.ascontiguousarray(rows[lo:hi])
        launches.append(_plan(hi - lo, h, w, part, img[lo].data_ptr())[:2])
        rc = lib.maua_feedback_f32(img[lo].data_ptr(), out[lo].data_ptr(), state.data_ptr(), int(k > 0 or state0 is not None), hi - lo, h, w,
                                   part.ctypes.data, part.shape[1], fr.MODES.index(mode), fr.BORDERS.index(border), _lib.stream_ptr())
        assert rc == 0, rc
    loose = ("out", "state", "img") if nonfinite else ()
    g.check(written=(() if in_place else ("out",)) + (("state",) if state0 is None else ()), nonfinite_ok=loose)
    return out.cpu().numpy(), state.cpu().numpy(), launches


def _expected_launches(rows):
    """(launches, still runs) of one call, as the header states them."""
    still = [bool(r[fr.STILL]) and fr.is_identity_matrix(r) for r in rows]
    runs = sum(1 for i, s in enumerate(still) if s and (i == 0 or not still[i - 1]))
    return [runs + still.count(False), runs]


@pytest.mark.parametrize("dyadic", (True, False), ids=("dyadic", "real"))
@pytest.mark.parametrize("kind", fr.KINDS)
@pytest.mark.parametrize("plane", fr.PLANES, ids=lambda p: "x".join(map(str, p)))
def test_every_mode_and_border_against_the_reference(gpu, plane, kind, dyadic):
    """Batches 1, 2 and 5 (the batch of 5 as two calls of 2 and 3 frames: the state crosses a call boundary) x every mode x every border.
    Dyadic operands: the emulation's bits.  Real operands: float64 within the allowance."""
    worst = 0.0
    for batch in fr.BATCHES:
        cur, rows = fr.case_operands(plane, batch, kind, dyadic)
        splits = (2,) if batch == 5 else None
        for mode, border in COMBOS:
            e32, e64, allow = fr.case_reference(plane, batch, kind, dyadic, mode, border, splits)
            got, state, launches = _feedback(gpu, cur, rows, mode, border, splits)
            edges = [0] + list(splits or ()) + [batch]
            assert launches == [_expected_launches(rows[lo:hi]) for lo, hi in zip(edges[:-1], edges[1:])]
            assert np.array_equal(_bits(state), _bits(got[-1])), (batch, mode, border)  # the dual store (or the copy)
            if dyadic:
                assert np.array_equal(_bits(got), _bits(e32)), (batch, mode, border, float(np.abs(got - e32).max()))
            else:
                err = float(np.abs(got.astype(F64) - e64).max())
                worst = max(worst, err / allow)
                assert err <= allow, (batch, mode, border, err, allow)
    if not dyadic:
        print(f"{plane} {kind}: largest device error / allowance {worst:.3f}")


def test_the_case_list_reaches_both_paths_both_instances_and_a_neutral_row():
    seen = set()
    for plane, batch, kind, dyadic in fr.cases():
        _, rows = fr.case_operands(plane, batch, kind, dyadic)
        launches, runs = _expected_launches(rows)
        seen.add(("still", runs > 0))
        seen.add(("warp", launches > runs))
        seen.add(("alternating", runs > 1 and launches > runs))
        seen.add(("vector", plane[1] % 4 == 0))
        seen.add(("neutral", any(fr.is_neutral(r) for r in rows)))
    assert seen == {(k, v) for k in ("still", "warp", "alternating", "vector", "neutral") for v in (True, False)}


@pytest.mark.parametrize("plane", ((17, 33), (64, 68)), ids=("17x33", "64x68"))
def test_still_rows_agree_bit_for_bit_through_both_paths(gpu, plane):
    """The register path against the warp path on the same still rows.  The warp path is forced in two ways: the still flag cleared on an
    identity matrix (the entry believes a cleared flag), and one matrix entry off by its last bit on a frame whose gain is 0 (that frame
    does not look at its taps, so the result must not change; the runs either side of it still take the register path)."""
    h, w = plane
    for dyadic in (True, False):
        cur, rows = fr.case_operands(plane, 5, "still", dyadic)
        for mode, border in COMBOS:
            e32 = fr.case_reference(plane, 5, "still", dyadic, mode, border, (2,))[0]
            fast, _, launches = _feedback(gpu, cur, rows, mode, border)
            assert launches == [[1, 1]] and np.array_equal(_bits(fast), _bits(e32))
            unflagged = rows.copy()
            unflagged[:, fr.STILL] = 0
            slow, _, launches = _feedback(gpu, cur, unflagged, mode, border)
            assert launches == [[5, 0]] and np.array_equal(_bits(slow), _bits(fast)), (mode, border)
    # gain 0 in the middle, its matrix one ulp off the identity
    cur, rows = fr.case_operands(plane, 5, "still", False)
    muted = rows.copy()
    muted[2, fr.GAIN], muted[2, fr.DRY] = 0, 0.75  # (dry != 1: the frame is combined, not passed through)
    nudged = muted.copy()
    nudged[2, fr.A] = np.nextafter(F32(1), F32(2))
    nudged[2, fr.STILL] = 0
    assert not fr.is_neutral(nudged[2])
    for mode, border in COMBOS:
        a, _, la = _feedback(gpu, cur, muted, mode, border)
        b, _, lb = _feedback(gpu, cur, nudged, mode, border)
        assert la == [[1, 1]] and lb == [[3, 2]] and np.array_equal(_bits(a), _bits(b)), (mode, border)
        assert np.array_equal(_bits(a), _bits(fr.run_calls(cur, muted, mode, border, dtype=F32)))


def test_state_carry_over_two_calls_and_a_given_state(gpu):
    """Two consecutive calls of 2 and 3 frames against ONE reference run of 5; state_valid 0 on the first call only.  Then a call that
    starts from a given state, a single moving frame among them (the frame that gathers from the state it replaces)."""
    plane = (17, 33)
    for kind in ("zoomrot", "mixed", "still"):
        cur, rows = fr.case_operands(plane, 5, kind, False)
        for mode, border in (("add", "mirror"), ("max", "wrap"), ("screen", "zero")):
            whole32 = fr.run(cur, rows, mode, border, dtype=F32)[0]
            whole64 = fr.run(cur, rows, mode, border, dtype=F64)[0]
            got, state, _ = _feedback(gpu, cur, rows, mode, border, splits=(2,))
            assert np.abs(got.astype(F64) - whole64).max() <= fr.allowance(whole32, whole64)
            assert np.array_equal(_bits(state), _bits(got[-1]))
            lost = fr.run_calls(cur, rows, mode, border, (2,), F64, defect="no carry")
            assert np.abs(lost - whole64).max() > fr.allowance(whole32, whole64)  # (what a lost state would look like)
    state0 = fr.image((1, 3, 17, 33), "state", True)[0]
    for batch in (1, 2):
        cur, rows = fr.case_operands(plane, batch, "zoomrot", True)
        for mode, border in COMBOS:
            want, want_state = fr.run(cur, rows, mode, border, state=state0, dtype=F32)
            got, state, _ = _feedback(gpu, cur, rows, mode, border, state0=state0)
            assert np.array_equal(_bits(got), _bits(want)) and np.array_equal(_bits(state), _bits(want_state)), (batch, mode, border)


def test_a_second_trip_of_the_grid_stride_loops(gpu):
    """A grid capped at 3 workgroups (maua_feedback_test_grid_cap, the entry's test hook) on planes of more than 3 x 256 items: the vector
    and the scalar instances of both kernels walk their items in two trips."""
    lib = _lib.load()
    assert lib.maua_feedback_test_grid_cap(3) == 0
    try:
        for plane in ((64, 68), (65, 63)):
            for kind in ("still", "mixed", "zoomrot"):
                cur, rows = fr.case_operands(plane, 5, kind, True)
                assert _plan(5, *plane, rows, 4096)[6] == 3 < -(-plane[0] * (plane[1] // 4 if plane[1] % 4 == 0 else plane[1]) // 256)
                for mode, border in (("add", "wrap"), ("screen", "mirror")):
                    e32 = fr.case_reference(plane, 5, kind, True, mode, border, (2,))[0]
                    assert np.array_equal(_bits(_feedback(gpu, cur, rows, mode, border)[0]), _bits(e32)), (plane, kind, mode, border)
    finally:
        assert lib.maua_feedback_test_grid_cap(0) == 3
    assert _plan(1, 64, 68, fr.make_row()[None], 4096)[6] == 5


def test_skewed_pointers_take_the_scalar_instances_to_the_same_bits(gpu):
    for plane in ((64, 68), (3, 5), (1, 1)):
        for kind in ("mixed", "neutral mid"):
            cur, rows = fr.case_operands(plane, 5, kind, True)
            for mode, border in (("add", "zero"), ("max", "mirror"), ("screen", "replicate")):
                e32 = fr.case_reference(plane, 5, kind, True, mode, border, (2,))[0]
                got, state, _ = _feedback(gpu, cur, rows, mode, border, skew=True)
                assert np.array_equal(_bits(got), _bits(e32)) and np.array_equal(_bits(state), _bits(e32[-1])), (plane, kind, mode, border)
    g = Guard(gpu)
    img = _inp(g, np.zeros((1, 3, 64, 68)), "img", skew=True)
    assert img.data_ptr() % 16 == 4 and _plan(1, 64, 68, fr.make_row()[None], img.data_ptr())[2] == 0 and _plan(1, 64, 68, fr.make_row()[None], 4096)[2] == 1


def test_in_place_is_what_the_render_uses(gpu):
    for plane in ((64, 68), (65, 63)):
        for kind in fr.KINDS:
            cur, rows = fr.case_operands(plane, 5, kind, True)
            for mode, border in (("add", "wrap"), ("max", "zero"), ("screen", "mirror")):
                e32 = fr.case_reference(plane, 5, kind, True, mode, border, (2,))[0]
                got, state, _ = _feedback(gpu, cur, rows, mode, border, splits=(2,), in_place=True)
                assert np.array_equal(_bits(got), _bits(e32)) and np.array_equal(_bits(state), _bits(e32[-1])), (plane, kind, mode, border)


def test_a_neutral_row_passes_nan_payloads_and_becomes_the_state(gpu):
    """Frame 1 of 3 is neutral and carries NaNs with a payload: it comes out in its own bits on both paths (among still rows: the register
    path; among moving rows: a launch of its own), and it is what frame 2 gathers from — finite wherever its taps are."""
    h, w = 17, 36
    for kind in ("still", "translate"):
        cur = fr.image((3, 3, h, w), kind, True)
        cur[1].view(np.uint32)[:, :4, :8] = 0x7FC12345
        rows = fr.rows_of(kind, 3, h, w, True)
        rows[1, fr.GAIN], rows[1, fr.DRY] = 0, 1
        for mode in fr.MODES:
            got, state, _ = _feedback(gpu, cur, rows, mode, "replicate", nonfinite=True)
            assert np.array_equal(_bits(got[1]), _bits(cur[1])), (kind, mode)
            want = fr.run(cur, rows, mode, "replicate", dtype=F32)[0]
            finite = np.isfinite(want)
            assert finite[2, :, 8:, 16:].all() and np.array_equal(_bits(got)[finite], _bits(want)[finite]) and np.array_equal(np.isfinite(got), finite)


def test_refusals_leave_the_outputs_untouched(gpu):
    lib, st = _lib.load(), _lib.stream_ptr()
    b, h, w = 2, 6, 8
    cur, rows = fr.image((b, 3, h, w), "refuse", True), np.ascontiguousarray(fr.rows_of("mixed", b, h, w, True))
    g = Guard(gpu)
    img, out, state = _inp(g, cur, "img"), _out(g, cur.shape, "out"), _out(g, (3, h, w), "state")
    names = ("img", "out", "state", "valid", "batch", "h", "w", "rows", "stride", "mode", "border", "stream")
    ok = (img.data_ptr(), out.data_ptr(), state.data_ptr(), 0, b, h, w, rows.ctypes.data, 16, 0, 0, st)
    call = lambda **kw: lib.maua_feedback_f32(*[kw.get(n, v) for n, v in zip(names, ok)])  # noqa: E731
    frame = 3 * h * w * 4
    for bad in (dict(img=None), dict(out=None), dict(state=None), dict(rows=None), dict(batch=0), dict(batch=-1), dict(h=0), dict(w=-1),
                dict(mode=-1), dict(mode=3), dict(border=-1), dict(border=4), dict(stride=15), dict(stride=0),
                dict(out=img.data_ptr() + 16), dict(out=img.data_ptr() - 16),
                dict(state=img.data_ptr()), dict(state=img.data_ptr() + frame), dict(state=img.data_ptr() + 2 * frame - 4),
                dict(state=out.data_ptr()), dict(state=out.data_ptr() + b * frame - 4), dict(state=out.data_ptr() - frame + 4)):
        assert call(**bad) == EINVAL, bad
    assert call(h=65536, w=32768) == ENOSYS
    assert g.untouched("out") and g.untouched("state")
    g.check()
    assert call() == 0
    g.check(written=("out", "state"))
    want, want_state = fr.run(cur, rows, "add", "zero", dtype=F32)
    assert np.array_equal(_bits(out.cpu().numpy()), _bits(want)) and np.array_equal(_bits(state.cpu().numpy()), _bits(want_state))


def test_captured_calls_replay_to_the_same_bytes(gpu):
    """A call of mixed still and moving rows (and one of a single moving frame with a valid state: the launch plus the copy) captured on a
    side stream and replayed twice from the same state: identical bits, the emulation's; the rows were read at capture."""
    lib = _lib.load()
    stream = torch.cuda.Stream(gpu)
    plane = (33, 52)
    state0 = fr.image((1, 3, *plane), "captured state", True)[0]
    for batch, kind in ((5, "mixed"), (1, "translate")):
        cur, rows = fr.image((batch, 3, *plane), "captured", True), np.ascontiguousarray(fr.rows_of(kind, batch, *plane, True))
        want, want_state = fr.run(cur, rows, "screen", "mirror", state=state0, dtype=F32)
        g = Guard(gpu)
        img, out, state = _inp(g, cur, "img"), _out(g, cur.shape, "out"), _inp(g, state0, "state")
        keep = state.clone()
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            with _lib.HipGraph() as graph:
                rc = lib.maua_feedback_f32(img.data_ptr(), out.data_ptr(), state.data_ptr(), 1, batch, *plane, rows.ctypes.data, 16, 2, 2, _lib.stream_ptr())
            assert rc == 0
            rows[:] = 0  # (the launches carry their rows by value)
            results = []
            for _ in range(2):
                state.copy_(keep)
                out.zero_()
                graph.replay()
                stream.synchronize()
                results.append((out.cpu().numpy(), state.cpu().numpy()))
        for got, got_state in results:
            assert np.array_equal(_bits(got), _bits(want)) and np.array_equal(_bits(got_state), _bits(want_state)), (batch, kind)
        g.check(written=("out",))
