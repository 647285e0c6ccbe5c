"""Host (no GPU): the definitions of tests/iir_ref.py are what they claim to be, the allowance the GPU tests use is honest, and four
deliberately wrong versions of the chunked algorithm are caught by the very comparisons the GPU tests make.  The case lists that
reach every instance (n_sections 1 .. 16) and every edge of the chunk grid: exact where they claim to be, their allowances capped, six
wrong versions caught, and — asked of the library's own maua_sosfilt_plan — complete.  Also the host-side halves
of audioreactive/filters.py: sosfiltfilt's padding rule against scipy, the coefficient mapping of ar.envelope, the band designs."""
import math

import numpy as np
import pytest
import scipy.signal

import iir_ref as q

EINVAL = -22

ALL_CHUNKS = (4, 64, 128)  # (the default is 64 for every length the GPU tests judge against the long-double loop)


def test_longdouble_is_wider_than_double():
    assert np.finfo(np.longdouble).eps < 2.0 ** -60, "np.longdouble is no reference on this machine"


@pytest.mark.parametrize("name", ["hp30", "lp100", "bp20_200", "rms", "pitch"])
def test_sequential_float64_is_scipy(name):
    sos = q.filters()[name]
    x = q.signals()[0, :3000].astype(np.float64)
    y, zf = q.sequential(sos, x)
    assert q.same_bits(y[0], scipy.signal.sosfilt(sos, x))
    zi = np.random.default_rng(5).standard_normal((len(sos), 2))
    want, want_zf = scipy.signal.sosfilt(sos, x, zi=zi)
    y, zf = q.sequential(sos, x, zi=zi[None])
    assert q.same_bits(y[0], want) and q.same_bits(zf[0], want_zf)


@pytest.mark.parametrize("name", sorted(q.EXACT))
@pytest.mark.parametrize("chunk", [1, 4, 7, 64])
def test_chunked_equals_sequential_on_integers(name, chunk):
    sos = q.EXACT[name]
    x = q.exact_signal(203)
    zi = np.arange(1, 2 * len(sos) + 1, dtype=np.float64).reshape(1, len(sos), 2)
    for z in (None, zi):
        want, want_zf = q.sequential(sos, x, zi=z)
        got, zf = q.chunked(sos, x, chunk, zi=z)
        assert q.same_bits(got, want) and q.same_bits(zf, want_zf)
    if name == "running_sum":
        assert q.same_bits(q.chunked(sos, x, chunk)[0][0], np.cumsum(x))


def test_default_chunk_restated():
    assert [q.default_chunk(n) for n in (0, 1, 32768, 32769, 131072, 131073, 5292000, 1 << 30)] == [64, 64, 64, 128, 128, 256, 1024, 4096]


@pytest.mark.parametrize("name", sorted(q.filters()))
def test_chunked_error_ceiling(name):
    """err_chunked_f64 <= 1e-10 for every filter of the case list and every chunk length the GPU tests use: the allowance derived from
    it cannot hide a broken kernel.  (Worst found: the 8th-order 20-200 Hz band-pass with 4-sample chunks.)"""
    for chunk in ALL_CHUNKS:
        err_c, err_s = q.errors(name, chunk)
        print(f"{name} chunk {chunk}: err_chunked {err_c:.2e} err_sequential {err_s:.2e} allow {q.allowance(name, chunk):.2e}")
        assert err_c <= 1e-10 and err_s <= 1e-10


@pytest.mark.parametrize("chunk", [4, 64, 2048])
def test_chunked_with_state_and_short_last_chunk(chunk):
    """zi, zf and a last chunk shorter than the others (or a single chunk) against the long-double loop."""
    sos = q.filters()["pitch"]
    n = 1531
    x = q.signals()[1, :n].astype(np.float64)
    zi = 1e-3 * np.random.default_rng(9).standard_normal((1, len(sos), 2))
    ref, ref_zf = q.sequential(sos, x, zi=zi, dtype=np.longdouble)
    got, zf = q.chunked(sos, x, chunk, zi=zi)
    scale = float(np.max(np.abs(ref)))
    assert q.rel_err(got, ref) <= 1e-10 and float(np.max(np.abs(zf - ref_zf))) <= 1e-10 * max(scale, float(np.max(np.abs(ref_zf))))


@pytest.mark.parametrize("variant", ["carry_dropped", "carry_late", "sections_reversed", "zi_swapped"])
def test_wrong_variants_are_caught(variant):
    """Each wrong version fails the comparison of the GPU tests (|y - long double| <= allow max|y|) on a filter of the case list, and
    the bit-for-bit comparison on the integer cases.  (Sections commute from a zero state: the state is what tells them apart.)"""
    name, chunk, n = "lp100", 64, 1000
    sos = q.filters()[name]
    x = q.signals()[0, :n].astype(np.float64)
    zi = np.random.default_rng(11).standard_normal((1, len(sos), 2)) * np.array([1.0, -0.7])
    ref, _ = q.sequential(sos, x, zi=zi, dtype=np.longdouble)
    allow = q.allowance(name, chunk)
    assert q.rel_err(q.chunked(sos, x, chunk, zi=zi)[0], ref) <= allow
    assert q.rel_err(q.chunked(sos, x, chunk, zi=zi, variant=variant)[0], ref) > 1e6 * allow
    mix, xi = q.EXACT["mix"], q.exact_signal(203)
    zi = np.array([[[1.0, 2.0], [3.0, 4.0]]])
    assert not q.same_bits(q.chunked(mix, xi, 7, zi=zi, variant=variant)[0], q.sequential(mix, xi, zi=zi)[0])


def test_follower_restatement():
    x = np.array([[0.0], [1.0], [1.0], [0.0], [0.0]], np.float32)
    y = q.follower(x, 0.5, 0.25)
    assert y[:, 0].tolist() == [0.0, 0.5, 0.75, 0.5625, 0.421875]
    assert q.follower(x, 1.0, 1.0).tolist() == x.tolist() and q.follower(x, 0.0, 0.0, y0=[3.0]).tolist() == [[3.0]] * 5
    x = np.array([[1.0, 1.0], [np.nan, 1.0], [2.0, 2.0]], np.float32)
    y = q.follower(x, 0.5, 0.5)
    assert np.isnan(y[1:, 0]).all() and y[:, 1].tolist() == [1.0, 1.0, 1.5]


# ------------------------------------------------------------------------------------------------ audioreactive/filters.py, host side
def test_filtfilt_padding_is_scipys():
    """With the padding length of ar.filtfilt_pad and the odd extension of filters._odd_ext, forward-flip-forward-flip through scipy's
    own sosfilt reproduces scipy.signal.sosfiltfilt bit for bit — for even and odd orders (a first-order section shortens the pad)."""
    import torch

    from maua_stylegan2_amd.audioreactive import filters as f

    x = q.signals()[0, :700].astype(np.float64)
    for sos in (q.filters()["lp100"], q.filters()["rms"], scipy.signal.butter(3, 500, "hp", fs=q.SR, output="sos"),
                scipy.signal.butter(5, [300, 900], "bp", fs=q.SR, output="sos"), f.bank_sos((None, 200), q.SR, 6)[0]):
        edge = f.filtfilt_pad(sos)
        ext = f._odd_ext(torch.from_numpy(x), edge).numpy()
        assert len(ext) == len(x) + 2 * edge
        zi = scipy.signal.sosfilt_zi(sos)
        y, _ = scipy.signal.sosfilt(sos, ext, zi=zi * ext[0])
        y, _ = scipy.signal.sosfilt(sos, y[::-1], zi=zi * y[-1])
        assert q.same_bits(np.ascontiguousarray(y[::-1][edge:-edge]), scipy.signal.sosfiltfilt(sos, x))


def test_envelope_coefficient_mapping():
    import maua_stylegan2_amd.audioreactive as ar

    smf = ar.signal.SMF
    try:
        ar.set_SMF(1)
        assert ar.envelope_coefficient(0) == 1.0 and ar.envelope_coefficient(-3) == 1.0 and ar.envelope_coefficient(math.inf) == 0.0
        assert ar.envelope_coefficient(float("nan")) == 1.0
        for tau in (0.5, 1, 8, 100):
            assert ar.envelope_coefficient(tau) == -math.expm1(-1.0 / tau)
        assert abs(ar.envelope_coefficient(1 / math.log(2)) - 0.5) < 1e-15
        ar.set_SMF(2)  # twice the frame rate: the same time constant is twice the frames
        assert ar.envelope_coefficient(4) == -math.expm1(-1.0 / 8) and ar.envelope_coefficient(0) == 1.0
    finally:
        ar.set_SMF(smf)


def test_band_designs():
    import maua_stylegan2_amd.audioreactive as ar

    edges = ar.band_edges(4, 20, 8000)
    assert len(edges) == 5 and edges[0] == 20.0 and edges[-1] == 8000.0
    assert np.allclose(np.diff(np.log(edges)), math.log(400) / 4)
    mel = ar.band_edges(3, 100, 4000, scale="mel")
    steps = np.diff(ar.signal._hz_to_mel(np.array(mel)))
    assert len(mel) == 4 and np.allclose(steps, steps[0])
    with pytest.raises(ValueError):
        ar.band_edges(3, scale="bark")
    sos = ar.bank_sos((None, 150, 600, None), q.SR, order=6)
    assert sos.shape == (3, 6, 6)
    assert q.same_bits(sos[1], scipy.signal.butter(6, [150, 600], "bp", fs=q.SR, output="sos"))
    assert q.same_bits(sos[0, :3], scipy.signal.butter(6, 150, "lp", fs=q.SR, output="sos")) and (sos[0, 3:] == q.IDENTITY).all()
    assert q.same_bits(sos[2, :3], scipy.signal.butter(6, 600, "hp", fs=q.SR, output="sos")) and (sos[2, 3:] == q.IDENTITY).all()
    assert q.same_bits(ar.butter_sos(12, [20, 8000], "bp", q.SR), q.filters()["rms"])


# ------------------------------------------------------------------------------------------------ every instance, every chunk-grid edge
NEW_VARIANTS = ("zi_of_filter_0", "last_chunk_full")
VARIANTS = ("carry_dropped", "carry_late", "sections_reversed", "zi_swapped") + NEW_VARIANTS


@pytest.mark.parametrize("ns", q.ALL_NS)
def test_integer_cascade_is_exact(ns):
    """The cascade of `ns` integer sections over 1100 samples from the state 1, 2, 3, ...: float64 has the bits of long double (nothing
    was rounded), |y| <= 2^10, and the chunked algorithm at 5, 17 and 100 has the bits of the loop, y and zf alike.  Likewise the bank of
    two rotations that the device test runs."""
    sos, x, zi = q.cascade(ns), q.exact_signal(1100), q.cascade_zi(1, ns)
    y, zf = q.sequential(sos, x, zi=zi)
    y_ld, zf_ld = q.sequential(sos, x, zi=zi, dtype=np.longdouble)
    assert np.array_equal(y.astype(np.longdouble), y_ld) and np.array_equal(zf.astype(np.longdouble), zf_ld)
    assert q.same_bits(y_ld.astype(np.float64), y) and q.same_bits(zf_ld.astype(np.float64), zf)
    assert float(np.max(np.abs(y))) <= 2.0 ** 10
    for chunk in (5, 17, 100):
        got, got_zf = q.chunked(sos, x, chunk, zi=zi)
        assert q.same_bits(got, y) and q.same_bits(got_zf, zf), chunk
    sos, x, zi = q.instance_case(ns)
    assert sos.shape == (2, ns, 6) and not np.array_equal(x[0], x[1]) and len(np.unique(zi)) == zi.size and zi.min() == 1
    assert all(np.array_equal(sos[1, s], q.PATTERN[(s + 1) % 8]) and np.array_equal(sos[0, s], q.PATTERN[s % 8]) for s in range(ns))
    for z in (None, zi):
        y, zf = q.sequential(sos, x, zi=z)
        y_ld, zf_ld = q.sequential(sos, x, zi=z, dtype=np.longdouble)
        assert q.same_bits(y_ld.astype(np.float64), y) and q.same_bits(zf_ld.astype(np.float64), zf)
        assert float(np.max(np.abs(y))) < 2.0 ** 24  # (the float output is exact as well)
        for chunk in q.INSTANCE_CHUNKS:
            got, got_zf = q.chunked(sos, x, chunk, zi=z)
            assert q.same_bits(got, y) and q.same_bits(got_zf, zf), chunk


@pytest.mark.parametrize("ns", q.ALL_NS)
def test_every_instance_case_catches_every_wrong_variant(ns):
    """The comparison of test_sosfilt_every_instance_on_integers (y and zf bit for bit, with zi) tells each wrong version from the right
    one at every chunk length it runs.  One exemption: reversing one section is the identity."""
    sos, x, zi = q.instance_case(ns)
    want, want_zf = q.sequential(sos, x, zi=zi)
    for chunk in q.INSTANCE_CHUNKS:
        assert q.INSTANCE_N % chunk, "the last chunk is short: last_chunk_full has something to get wrong"
        for variant in VARIANTS:
            got, got_zf = q.chunked(sos, x, chunk, zi=zi, variant=variant)
            caught = not (q.same_bits(got, want) and q.same_bits(got_zf, want_zf))
            assert caught != (variant == "sections_reversed" and ns == 1), (variant, chunk)


def test_the_new_wrong_variants_are_what_they_say():
    sos, x, zi = q.instance_case(3)
    want, want_zf = q.sequential(sos, x, zi=zi)
    y, zf = q.chunked(sos, x, 17, zi=zi, variant="zi_of_filter_0")  # filter 0 is right, filter 1 starts from the wrong state
    assert q.same_bits(y[0], want[0]) and q.same_bits(zf[0], want_zf[0]) and not q.same_bits(y[1], want[1])
    assert q.same_bits(y[1], q.sequential(sos[1], x[1], zi=zi[:1])[0][0])
    y, zf = q.chunked(sos, x, 17, zi=zi, variant="last_chunk_full")  # y is right, zf is the state 17 - 203 % 17 zero samples later
    assert q.same_bits(y, want) and not q.same_bits(zf, want_zf)
    pad = np.concatenate([x, np.zeros((2, 17 - q.INSTANCE_N % 17))], axis=1)
    assert q.same_bits(zf, q.sequential(sos, pad, zi=zi)[1])
    y, zf = q.chunked(sos, x[:, :34], 17, zi=zi, variant="last_chunk_full")  # a full last chunk: nothing to get wrong
    assert q.same_bits(zf, q.sequential(sos, x[:, :34], zi=zi)[1])


QUICK = [name for name, case in q.GEOMETRY.items() if case["chunk"] <= 100]


def test_geometry_list_is_the_one_the_issue_names():
    g = q.GEOMETRY
    tiles = {(c["chunk"], c["n"]) for name, c in g.items() if name.startswith("chunk") and c["chunk"] <= 100}
    assert tiles == {(ch, 2 * ch + last) for ch in (1, 15, 16, 17, 31, 33, 100) for last in (1, ch - 1, ch) if last >= 1}
    assert {(c["chunk"], -(-c["n"] // c["chunk"]), c["n"] % c["chunk"]) for name, c in g.items() if name.startswith("nc")} == \
        {(5, nc, 3) for nc in (1, 2, 8, 9, 10, 16, 17, 18, 64, 65, 66, 128, 129, 130)} | {(17, nc, 3) for nc in (9, 65, 66)}
    assert (g["chunk4096"]["n"], g["chunk4096"]["chunk"]) == (3 * 4096 + 5, 4096) and g["chunk4096"]["zi"] is not None
    assert g["chunk4096_zero_state"]["n"] == 3 * 4096 + 5 and np.array_equal(g["chunk4096"]["sos"][0], q.EXACT["mix"])
    big = g["largest_chunk"]
    assert big["n"] == 2 * big["chunk"] + 3 and big["F"] == 1 and np.array_equal(big["sos"][0], q.EXACT["running_sum"])
    assert big["chunk"] & (big["chunk"] - 1) == 0 and big["chunk"] <= q.MAX_CHUNK
    for name in ("filters64_shared", "filters64_own"):
        c = g[name]
        assert (c["F"], c["ns"], c["chunk"], c["n"]) == (64, 3, 17, 203) and len(np.unique(c["zi"])) == 64 * 6
        assert q.geometry_operands(name)[1].ndim == (1 if c["shared"] else 2)
    plain = [c for name, c in g.items() if c["chunk"] <= 100 and c["F"] == 2]
    assert len(plain) == len(QUICK) - 2 and {c["ns"] for c in plain} == {3, 5}
    assert all(not c["shared"] and c["zi"] is not None and c["zi"].min() >= 1 for c in plain)


@pytest.mark.parametrize("name", QUICK)
def test_geometry_classes_are_exact_and_catch_the_new_variants(name):
    """Every class of the chunk grid: the chunked algorithm has the bits of the loop (so the device may be held to them), filter 1 started
    from filter 0's state is caught, and a short last chunk walked to its full length is caught."""
    case = q.GEOMETRY[name]
    sos, x, zi = q.geometry_operands(name)
    want, want_zf = q.geometry_reference(name)
    ref_ld = q.sequential(sos, x, zi=zi, dtype=np.longdouble)
    assert q.same_bits(ref_ld[0].astype(np.float64), want) and q.same_bits(ref_ld[1].astype(np.float64), want_zf)
    got, got_zf = q.chunked(sos, x, case["chunk"], zi=zi)
    assert q.same_bits(got, want) and q.same_bits(got_zf, want_zf)
    y, zf = q.chunked(sos, x, case["chunk"], zi=zi, variant="zi_of_filter_0")
    assert not q.same_bits(y, want) and not q.same_bits(zf, want_zf)
    if case["F"] == 64:  # every filter but the first is caught (on y: a cascade of FIR sections alone forgets its first state)
        assert all(not q.same_bits(y[f], want[f]) for f in range(1, 64)) and q.same_bits(y[0], want[0])
        if not case["shared"]:
            assert len({want_zf[f].tobytes() for f in range(64)}) == 64, "a zf written to another filter's slot would go unseen"
    y, zf = q.chunked(sos, x, case["chunk"], zi=zi, variant="last_chunk_full")
    assert q.same_bits(zf, want_zf) == (case["n"] % case["chunk"] == 0), "a short last chunk walked too far must show in zf"


def test_long_chunk_references_are_the_loop():
    """chunk4096: cumsum(convolve(x, [1, 2, 1])) is the loop from the zero state, in either order of the two sections; with a state the
    reference is the loop itself.  largest_chunk: cumsum is the loop over a prefix, and its last value is the state (z2 = 0 x - 0 y)."""
    sos, x, zi = q.geometry_operands("chunk4096_zero_state")
    assert zi is None and x.shape == (2, 3 * 4096 + 5)
    y, zf = q.geometry_reference("chunk4096_zero_state")
    loop = q.sequential(sos, x)
    assert q.same_bits(y, loop[0]) and q.same_bits(zf, loop[1]) and float(np.max(np.abs(y))) < 2.0 ** 24
    sos, x, zi = q.geometry_operands("chunk4096")
    y, zf = q.geometry_reference("chunk4096")
    assert float(np.max(np.abs(y))) < 2.0 ** 24 and not q.same_bits(y, q.sequential(sos, x)[0])
    got, got_zf = q.chunked(sos, x, 4096, zi=zi)
    assert q.same_bits(got, y) and q.same_bits(got_zf, zf)
    assert not q.same_bits(q.chunked(sos, x, 4096, zi=zi, variant="last_chunk_full")[1], zf)
    sos, x, zi = q.geometry_operands("largest_chunk")
    y, zf = q.geometry_reference("largest_chunk")
    assert x.shape == (2 * q.LARGEST_CHUNK + 3,) and float(np.max(np.abs(y))) < 2.0 ** 24
    head, head_zf = q.sequential(sos, x[:500])
    assert q.same_bits(head, y[:, :500]) and q.same_bits(head_zf[0, 0, 0], y[0, 499]) and head_zf[0, 0, 1] == 0 == zf[0, 0, 1]


def test_butterworth_allowances_stay_under_their_cap():
    """No device comparison of test_sosfilt_every_instance_against_long_double can become vacuous: every allowance of the list — 16
    orders, three bands, shared and own signals, the three chunk settings — is at most 1e-10, and none is below the floor of the rule."""
    worst = {}
    for ns in q.ALL_NS:
        assert q.bp_bank(ns).shape == (3, ns, 6)
        for chunk in q.BP_CHUNKS:
            for mode in q.BP_MODES:
                for band, sig in enumerate(q.bp_signals(mode)):
                    allow = q.bp_allowance(ns, band, sig, chunk)
                    assert 64 * q.EPS <= allow <= 1e-10, (ns, q.BP_BANDS[band], sig, chunk, allow)
                    worst[band] = max(worst.get(band, 0.0), allow)
    print("largest allowance per band: " + ", ".join(f"{q.BP_BANDS[b]} Hz {v:.2e}" for b, v in sorted(worst.items())))
    assert q.default_chunk(q.BP_N) == 64
    ref = q.bp_longdouble(6, 1, 1)  # the one-walk reference is the plain long-double loop of the filter alone
    assert np.array_equal(ref, q.sequential(q.bp_bank(6)[1], q.signals()[1, :q.BP_N], dtype=np.longdouble)[0][0])
    assert q.errors_sos(q.bp_bank(6)[1], q.signals()[1, :q.BP_N], 17, ref) == q._bp_errors(6, 17)[(1, 1)]


# --- what the device case lists reach, asked of the library (maua_sosfilt_plan: the entry's own constants and checks, no launch)
def numpy_plan(F, ns, n, chunk):
    """maua_sosfilt_plan restated from the documented constants; None where the entry refuses the shape."""
    if not (1 <= F <= q.MAX_FILTERS and 1 <= ns <= 16 and n >= 0 and 0 <= chunk <= q.MAX_CHUNK):
        return None
    chunk = chunk or q.default_chunk(n)
    nc = -(-n // chunk)
    groups = lambda k: -(-k // q.SOS_LANES)  # noqa: E731
    return dict(chunk=chunk, nc=nc, launches=1 if n == 0 else 2 if nc == 1 else 4, zero_groups=groups(nc - 1) if n else 0,
                final_groups=groups(nc), tiles=-(-chunk // q.SOS_TILE), last_tile=(chunk - 1) % q.SOS_TILE + 1,
                last_chunk=n - (nc - 1) * chunk if n else 0)


@pytest.fixture(scope="module")
def plan(built_lib):
    from maua_stylegan2_amd import _lib

    def ask(F, ns, n, chunk):
        rc, p = _lib.planned_sosfilt(F, ns, n, chunk)
        assert rc == 0, (F, ns, n, chunk, rc)
        return p

    return ask


def device_cases():
    """(list, F, ns, n, chunk) of every call the three new device tests make."""
    for ns in q.ALL_NS:
        for chunk in q.INSTANCE_CHUNKS:
            yield "integers", 2, ns, q.INSTANCE_N, chunk
        for chunk in q.BP_CHUNKS:
            yield "butterworth", 3, ns, q.BP_N, chunk
    for name, c in q.GEOMETRY.items():
        yield "geometry", c["F"], c["ns"], c["n"], c["chunk"]


def test_plan_entry_is_its_restatement(plan):
    from maua_stylegan2_amd import _lib

    for _, F, ns, n, chunk in device_cases():
        assert plan(F, ns, n, chunk) == numpy_plan(F, ns, n, chunk), (F, ns, n, chunk)
    rng = np.random.default_rng(7)
    shapes = [(1, 1, 0, 0), (64, 16, 0, 65536), (1, 1, 1, 0), (3, 6, 1, 1), (2, 2, 65536, 65536), (2, 2, 65537, 65536), (1, 12, 5292000, 0),
              (1, 1, 2 ** 31 - 1, 0), (1, 1, 2 ** 31 - 1, 1), (1, 1, 2 ** 31 - 1, 65536), (4, 8, 1 << 30, 4096)]
    shapes += [(int(rng.integers(1, 65)), int(rng.integers(1, 17)), int(rng.integers(0, 200000)), int(rng.integers(0, 300))) for _ in range(300)]
    for F, ns, n, chunk in shapes:
        p = plan(F, ns, n, chunk)
        assert p == numpy_plan(F, ns, n, chunk), (F, ns, n, chunk)
        assert _lib.load().maua_sosfilt_ws_doubles(F, ns, n, chunk) == F * (4 * ns * ns + 2 * p["nc"] * 2 * ns)
    assert plan(1, 1, 0, 0) == dict(chunk=64, nc=0, launches=1, zero_groups=0, final_groups=0, tiles=4, last_tile=16, last_chunk=0)
    assert plan(2, 3, 203, 17) == dict(chunk=17, nc=12, launches=4, zero_groups=1, final_groups=1, tiles=2, last_tile=1, last_chunk=16)


def test_plan_entry_refuses_what_the_call_refuses(built_lib):
    """The shape refusals documented for maua_sosfilt_f64 (include/maua_hip.h): n_sections outside 1 .. 16, F outside 1 .. 64, n < 0, chunk < 0
    or > 65536 — from the plan, from the workspace size and from the entry itself (refused before any launch: no device needed) — and
    the plan's own: a null out.  n_signals and the pointers are no shape arguments."""
    import ctypes

    from maua_stylegan2_amd import _lib

    lib = _lib.load()
    fake = ctypes.c_void_p(256)  # never dereferenced: the call is refused before any launch
    good = dict(F=3, ns=2, n=300, chunk=64)
    bad = [dict(ns=0), dict(ns=17), dict(ns=-1), dict(F=0), dict(F=65), dict(F=-1), dict(n=-1), dict(chunk=-1), dict(chunk=65537)]
    for kw in bad:
        a = dict(good, **kw)
        assert numpy_plan(a["F"], a["ns"], a["n"], a["chunk"]) is None
        assert _lib.planned_sosfilt(a["F"], a["ns"], a["n"], a["chunk"]) == (EINVAL, None), kw
        assert lib.maua_sosfilt_ws_doubles(a["F"], a["ns"], a["n"], a["chunk"]) == -1, kw
        assert lib.maua_sosfilt_f64(fake, a["F"], a["ns"], None, fake, 1, a["n"], a["chunk"], None, fake, None, None, fake, None) == EINVAL, kw
    for kw in (dict(ns=1), dict(ns=16), dict(F=1), dict(F=64), dict(n=0), dict(chunk=0), dict(chunk=65536)):
        a = dict(good, **kw)
        assert _lib.planned_sosfilt(a["F"], a["ns"], a["n"], a["chunk"])[0] == 0, kw
    assert lib.maua_sosfilt_plan(3, 2, 300, 64, None) == EINVAL
    out = (ctypes.c_int32 * 9)(*[-7] * 9)
    assert lib.maua_sosfilt_plan(3, 2, 300, 64, out) == 0 and list(out) == [64, 5, 4, 1, 1, 4, 16, 44, -7]  # eight values, not nine
    assert lib.maua_sosfilt_plan(3, 0, 300, 64, out) == EINVAL and list(out)[:2] == [64, 5]                  # a refusal writes nothing


def test_device_case_lists_cover_every_instance_and_every_grid_edge(plan):
    """The three lists of tests/test_iir_gpu.py together, through the library's own plan: all 16 instances on integers and on Butterworth
    banks, and every edge of the chunk grid that csrc/iir.hip has a predicate for."""
    plans = {}
    for kind, F, ns, n, chunk in device_cases():
        plans.setdefault(kind, []).append(dict(plan(F, ns, n, chunk), F=F, ns=ns))
    assert {p["ns"] for p in plans["integers"]} == {p["ns"] for p in plans["butterworth"]} == set(range(1, 17))
    every = [p for group in plans.values() for p in group]
    geometry = plans["geometry"]

    def alone_in_last_group(live, groups):  # `live` lanes in all: the last workgroup has exactly one
        return groups >= 1 and live - q.SOS_LANES * (groups - 1) == 1

    need = {
        "a partial last tile behind a full one": lambda p: p["tiles"] >= 2 and 1 < p["last_tile"] < q.SOS_TILE,
        "a one-sample last tile behind a full one": lambda p: p["tiles"] >= 2 and p["last_tile"] == 1,
        "a one-sample chunk": lambda p: p["chunk"] == 1 and p["nc"] > 1,
        "one tile, not full": lambda p: p["tiles"] == 1 and 1 < p["last_tile"] < q.SOS_TILE and p["nc"] > 1,
        "whole tiles only": lambda p: p["tiles"] >= 1 and p["last_tile"] == q.SOS_TILE and p["nc"] > 1,
        "the largest default chunk": lambda p: p["chunk"] == 4096 and p["nc"] > 1,
        "the largest chunk of the list": lambda p: p["chunk"] == q.LARGEST_CHUNK and p["nc"] > 1,
        "64 filters": lambda p: p["F"] == q.MAX_FILTERS and p["nc"] > 1,
        "two launches": lambda p: p["launches"] == 2,
        "four launches": lambda p: p["launches"] == 4,
    }
    for groups in (1, 2, 3):
        need[f"a zero-state pass of {groups} workgroups, the last with one live chunk"] = \
            lambda p, g=groups: p["zero_groups"] == g and alone_in_last_group(p["nc"] - 1, g)
        need[f"a final pass of {groups} workgroups, the last with one live chunk"] = \
            lambda p, g=groups: p["final_groups"] == g and alone_in_last_group(p["nc"], g)
        if groups < 3:
            need[f"a final pass of {groups} full workgroups"] = lambda p, g=groups: p["nc"] == q.SOS_LANES * g
    for edge in (q.SOS_AHEAD, 2 * q.SOS_AHEAD):  # the carry fetches Z eight chunks ahead: c0 + 8 + u < nc - 1
        for side in (-1, 0, 1):
            need[f"nc - 1 = {edge + side}"] = lambda p, v=edge + side: p["nc"] - 1 == v
    for what, last in (("1", lambda p: 1), ("chunk - 1", lambda p: p["chunk"] - 1), ("chunk", lambda p: p["chunk"])):
        for ch in q.TILE_CHUNKS:
            if what != "chunk - 1" or ch - 1 > 1:
                need[f"chunk {ch}, three chunks, the last {what} long"] = \
                    lambda p, ch=ch, last=last: p["chunk"] == ch and p["nc"] == 3 and p["last_chunk"] == last(p)
    missing = [what for what, has in need.items() if not any(has(p) for p in geometry)]
    assert not missing, missing
    for ns in q.ALL_NS:  # every instance walks a partial second tile and a default-length chunk
        assert any(p["ns"] == ns and p["chunk"] == 17 for p in every) and any(p["ns"] == ns and p["chunk"] == 64 and p["nc"] > 1 for p in every)
