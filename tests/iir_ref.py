"""Definitions behind csrc/iir.hip, restated in numpy (no GPU): the sequential biquad cascade in any float type, the chunked algorithm of
include/maua_hip.h in float64 in its defined order, the float32 envelope follower, and the case lists of the IIR tests.

Every function is vectorised over a leading axis of filters (and, for the chunked one, over the chunks): the loops over time and sections
are plain Python.  Where the device fuses a multiply and an add into one rounding (fma) the restatement rounds twice; that is the only
arithmetic difference, and the allowance of :func:`allowance` has a factor 4 for it."""
import functools

import numpy as np
import scipy.signal

SR = 22050
N_REF = 20000
EPS = 2.0 ** -53
IDENTITY = np.array([1.0, 0, 0, 1, 0, 0])


# ------------------------------------------------------------------------------------------------ the recurrences
def as_bank(sos):
    sos = np.asarray(sos, dtype=np.float64)
    return sos[None] if sos.ndim == 2 else sos


def sequential(sos, x, zi=None, dtype=np.float64):
    """scipy.signal.sosfilt's transposed direct form II, sample by sample in ``dtype`` (np.float64 or np.longdouble).  sos [F, ns, 6]
    (or [ns, 6]); x [n] (shared) or [F, n]; zi [F, ns, 2].  -> (y [F, n], zf [F, ns, 2]) in ``dtype``."""
    sos = as_bank(sos).astype(dtype)
    F, ns = sos.shape[:2]
    x = np.asarray(x).astype(dtype)
    x = np.broadcast_to(x, (F, x.shape[-1]))
    z = np.zeros((F, ns, 2), dtype) if zi is None else np.array(zi, dtype=dtype).reshape(F, ns, 2)
    y = np.empty(x.shape, dtype)
    b0, b1, b2, a1, a2 = (np.ascontiguousarray(sos[:, :, k].T) for k in (0, 1, 2, 4, 5))  # [ns, F]
    z1, z2 = np.ascontiguousarray(z[:, :, 0].T), np.ascontiguousarray(z[:, :, 1].T)
    for t in range(x.shape[1]):
        v = x[:, t]
        for s in range(ns):
            w = b0[s] * v + z1[s]
            z1[s] = b1[s] * v - a1[s] * w + z2[s]
            z2[s] = b2[s] * v - a2[s] * w
            v = w
        y[:, t] = v
    return y, np.stack([z1.T, z2.T], axis=-1)


def _walk(co, v_in, z1, z2, steps, out=None):
    """``steps`` samples of the cascade over arrays of any common shape; v_in(t) gives the input at step t, the lists z1 / z2 hold the
    states per section and receive the new ones (a shorter last chunk is the caller's business)."""
    b0, b1, b2, a1, a2 = co
    for t in range(steps):
        v = v_in(t)
        for s in range(len(b0)):
            w = b0[s] * v + z1[s]
            z1[s] = b1[s] * v - a1[s] * w + z2[s]
            z2[s] = b2[s] * v - a2[s] * w
            v = w
        if out is not None:
            out[..., t] = v


def chunked(sos, x, chunk, zi=None, variant=None):
    """The chunked algorithm of maua_sosfilt_f64 in float64, in the defined order: transition matrix from unit states, zero-state pass,
    carry with every dot product summed in ascending index order, final pass.  -> (y [F, n], zf [F, ns, 2]).
    ``variant`` names a deliberately WRONG version (the host test shows that the comparisons catch each): "carry_dropped",
    "carry_late", "sections_reversed", "zi_swapped", "zi_of_filter_0" (every filter starts from filter 0's state), "last_chunk_full"
    (a short last chunk is walked on, over zeros, to the full length before zf is taken)."""
    sos = as_bank(sos)
    F, ns = sos.shape[:2]
    D = 2 * ns
    x = np.asarray(x, dtype=np.float64)
    x = np.broadcast_to(x, (F, x.shape[-1]))
    n = x.shape[1]
    z0 = np.zeros((F, ns, 2)) if zi is None else np.array(zi, dtype=np.float64).reshape(F, ns, 2)
    if variant == "zi_swapped":
        z0 = z0[:, :, ::-1]
    elif variant == "zi_of_filter_0":
        z0 = np.repeat(z0[:1], F, axis=0)
    if n == 0:
        return np.empty((F, 0)), z0.copy()
    order = range(ns - 1, -1, -1) if variant == "sections_reversed" else range(ns)
    co = [[sos[:, s, k][:, None] for s in order] for k in (0, 1, 2, 4, 5)]  # per section [F, 1]
    nc = -(-n // chunk)
    # 1. transition matrix: unit states, zero input, a full chunk
    unit = np.broadcast_to(np.eye(D), (F, D, D))  # [F, state i, start j]
    z1 = [unit[:, 2 * s, :].copy() for s in range(ns)]
    z2 = [unit[:, 2 * s + 1, :].copy() for s in range(ns)]
    zero = np.zeros((F, D))
    _walk(co, lambda t: zero, z1, z2, chunk if nc > 1 else 0)
    A = np.empty((F, D, D))
    for s in range(ns):
        A[:, 2 * s, :], A[:, 2 * s + 1, :] = z1[s], z2[s]
    # 2. zero-state pass over the full chunks before the last
    xp = np.zeros((F, nc * chunk))
    xp[:, :n] = x
    xc = xp.reshape(F, nc, chunk)
    z1 = [np.zeros((F, nc - 1)) for _ in range(ns)]
    z2 = [np.zeros((F, nc - 1)) for _ in range(ns)]
    _walk(co, lambda t: xc[:, :-1, t], z1, z2, chunk if nc > 1 else 0)
    Z = np.empty((F, nc - 1, D))
    for s in range(ns):
        Z[:, :, 2 * s], Z[:, :, 2 * s + 1] = z1[s], z2[s]
    # 3. carry
    S = np.empty((F, nc, D))
    S[:, 0] = z0.reshape(F, D)
    for c in range(nc - 1):
        acc = np.zeros((F, D))
        for j in range(D):
            acc = acc + A[:, :, j] * S[:, c, j][:, None]
        S[:, c + 1] = acc + Z[:, c]
    if variant == "carry_dropped":
        S[:, 1:] = 0.0
    elif variant == "carry_late":
        S[:, 1:] = S[:, :-1].copy()
    # 4. final pass; the last chunk may be shorter: its lane stops at its own length
    y = np.empty((F, nc, chunk))
    z1 = [S[:, :, 2 * s].copy() for s in range(ns)]
    z2 = [S[:, :, 2 * s + 1].copy() for s in range(ns)]
    last = chunk if variant == "last_chunk_full" else n - (nc - 1) * chunk
    _walk(co, lambda t: xc[:, :, t], z1, z2, last, out=y)
    if last < chunk:
        full1, full2 = [a[:, :-1] for a in z1], [a[:, :-1] for a in z2]
        end1, end2 = [a[:, -1].copy() for a in z1], [a[:, -1].copy() for a in z2]
        for t in range(last, chunk):  # the chunks before the last go on alone
            v = xc[:, :-1, t]
            for s in range(ns):
                w = co[0][s] * v + full1[s]
                full1[s][...] = co[1][s] * v - co[3][s] * w + full2[s]
                full2[s][...] = co[2][s] * v - co[4][s] * w
                v = w
            y[:, :-1, t] = v
    else:
        end1, end2 = [a[:, -1] for a in z1], [a[:, -1] for a in z2]
    zf = np.stack([np.stack(end1, 1), np.stack(end2, 1)], axis=-1)
    if variant == "sections_reversed":
        zf = zf[:, ::-1]
    return y.reshape(F, nc * chunk)[:, :n], zf


def default_chunk(n):
    """maua_sosfilt_default_chunk restated: the smallest power of two p in [64, 4096] with 8 p^2 >= n."""
    p = 64
    while p < 4096 and 8 * p * p < n:
        p *= 2
    return p


def follower(x, ca, cr, y0=None):
    """maua_env_follow_f32 in numpy float32, every operation rounded once: x [T, C] -> y [T, C]."""
    x = np.asarray(x, dtype=np.float32)
    ca, cr = np.float32(ca), np.float32(cr)
    prev = (x[0] if y0 is None else np.asarray(y0, dtype=np.float32)).copy()
    y = np.empty_like(x)
    with np.errstate(invalid="ignore"):
        for t in range(x.shape[0]):
            d = x[t] - prev
            k = np.where(x[t] > prev, ca, cr).astype(np.float32)
            prev = (prev + (k * d).astype(np.float32)).astype(np.float32)
            y[t] = prev
    return y


# ------------------------------------------------------------------------------------------------ the cases
def _butter(order, band, btype):
    return scipy.signal.butter(order, band, btype, fs=SR, output="sos")


@functools.lru_cache(maxsize=None)
def filters():
    """name -> sos [ns, 6].  The five filters the project uses or is likely to (rms, pitch, hp30, lp100, bp20_200) and enough neighbours
    of the same length to make banks of three at 1, 2, 12 and 16 sections."""
    return {
        "hp30": _butter(2, 30, "hp"), "hp100_1": _butter(2, 100, "hp"), "lp100_1": _butter(2, 100, "lp"),
        "lp100": _butter(4, 100, "lp"), "hp30_2": _butter(4, 30, "hp"), "bp20_200_2": _butter(2, [20, 200], "bp"),
        "bp20_200": _butter(4, [20, 200], "bp"),
        "rms": _butter(12, [20, 8000], "bp"), "pitch": _butter(12, [65, 2100], "bp"), "mid12": _butter(12, [200, 2000], "bp"),
        "wide16": _butter(16, [20, 8000], "bp"), "pitch16": _butter(16, [65, 2100], "bp"), "mid16": _butter(16, [300, 3000], "bp"),
    }


BANKS = {1: ("hp30", "hp100_1", "lp100_1"), 2: ("lp100", "hp30_2", "bp20_200_2"), 12: ("rms", "pitch", "mid12"),
         16: ("wide16", "pitch16", "mid16")}
CHUNKS = (4, 64, 0)  # 0: the default
MODES = ("one", "bank_shared", "bank_own")  # F = 1; F = 3 over one signal; F = 3 over three signals
IO = [(i, o) for i in ("f32", "f64") for o in ("f32", "f64", "both")]


@functools.lru_cache(maxsize=None)
def signals():
    """Three noise signals of N_REF float32 samples (a float sample widens exactly: both input types carry the same numbers)."""
    return np.random.default_rng(20).standard_normal((3, N_REF)).astype(np.float32)


def bank(ns, mode):
    """(names, sos [F, ns, 6], signal index per filter) of a case."""
    names = BANKS[ns][:1] if mode == "one" else BANKS[ns]
    sig = tuple(range(len(names))) if mode == "bank_own" else (0,) * len(names)
    return names, np.stack([filters()[k] for k in names]), sig


def lengths(chunk):
    """The sample counts a (bank, chunk) case runs: around the chunk length, several chunks, 5000 and — for the default — all N_REF
    samples (the default is 64 up to 32 768 samples; test_sosfilt_default_chunk_beyond_its_minimum goes further, on integers)."""
    c = chunk or default_chunk(5000)
    return [1, 2, c - 1, c, c + 1, 3 * c + 5, 5000] + ([] if chunk else [N_REF])


@functools.lru_cache(maxsize=None)
def _longdouble_all():
    """Every (filter, signal) pair the cases need through the long-double loop in ONE walk: the filters padded to 16 sections with
    identity sections (y = 1 x + 0: exact)."""
    pairs = sorted({(name, s) for ns in BANKS for mode in MODES for name, s in zip(bank(ns, mode)[0], bank(ns, mode)[2])}
                   | {("bp20_200", 0)})
    sos = np.stack([np.concatenate([filters()[k], np.tile(IDENTITY, (16 - len(filters()[k]), 1))]) for k, _ in pairs])
    x = np.stack([signals()[s] for _, s in pairs])
    y, _ = sequential(sos, x, dtype=np.longdouble)
    return {p: y[i] for i, p in enumerate(pairs)}


def longdouble(name, sig=0):
    """The long-double output of filter ``name`` over signal ``sig`` [N_REF]; a prefix of it is the output of the shorter signal."""
    return _longdouble_all()[(name, sig)]


def rel_err(y, ref):
    ref = np.asarray(ref)
    return float(np.max(np.abs(np.asarray(y).astype(np.longdouble) - ref)) / np.max(np.abs(ref)))


@functools.lru_cache(maxsize=None)
def errors(name, chunk, sig=0, n=N_REF):
    """(err_chunked_f64, err_sequential_f64) of a filter over the first n samples of a signal against the long-double result, relative
    to max |y|; the sequential one is scipy's own."""
    ref = longdouble(name, sig)[:n]
    x = signals()[sig, :n].astype(np.float64)
    return rel_err(chunked(filters()[name], x, chunk)[0][0], ref), rel_err(scipy.signal.sosfilt(filters()[name], x), ref)


def allowance(name, chunk, sig=0, n=N_REF):
    """allow = 4 max(err_chunked_f64, err_sequential_f64, 16 * 2^-53) of the case itself (filter, signal, length, chunk; 0: the default
    for that length): the device may differ from the long-double result by what the float64 algorithms themselves do, times 4 for its
    fused roundings."""
    return 4.0 * max(*errors(name, chunk or default_chunk(n), sig, n), 16 * EPS)


# exact cases: small integers stay integers, so every order of summation gives the same bits
EXACT = {
    "running_sum": np.array([[1.0, 0, 0, 1, -1, 0]]),
    "every_other": np.array([[1.0, 0, 0, 1, 0, -1]]),
    "fir_121": np.array([[1.0, 2, 1, 1, 0, 0]]),
    "mix": np.array([[1.0, 2, 1, 1, 0, 0], [1.0, 0, 0, 1, -1, 0]]),
}


def exact_signal(n, seed=3):
    return np.random.default_rng(seed).integers(-8, 9, n).astype(np.float64)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


# ------------------------------------------------------------------------------------------------ every instance, every chunk-grid edge
# maua_sosfilt_f64 dispatches on n_sections to 16 template instances with their own register arrays and strides; the lists below reach
# each of them, and every edge of the chunk grid, on purpose (tests/test_iir_host.py proves it through maua_sosfilt_plan).
ALL_NS = tuple(range(1, 17))

# Integer sections [b0 b1 b2 1 a1 a2]: three FIRs of two taps or three, two integrators (one over every other sample) and three
# differences that keep the integrators from growing.  Small integers stay integers: every order of summation gives the same bits.
PATTERN = np.array([[1.0, 2, 1, 1, 0, 0], [1, -1, 0, 1, 0, 0], [1, 0, 0, 1, -1, 0], [1, 1, 0, 1, 0, 0],
                    [1, 0, -1, 1, 0, 0], [1, 0, 0, 1, 0, -1], [2, -1, 1, 1, 0, 0], [1, -2, 1, 1, 0, 0]])


def cascade(ns, F=1):
    """sos [F, ns, 6]: section s of filter f is PATTERN[(s + f) % 8] — filter f is the pattern rotated by f."""
    return np.stack([PATTERN[(np.arange(ns) + f) % len(PATTERN)] for f in range(F)])


def cascade_zi(F, ns):
    """zi [F, ns, 2] = 1, 2, 3, ... over the whole array: every filter, section and state starts from another number."""
    return np.arange(1, 2 * F * ns + 1, dtype=np.float64).reshape(F, ns, 2)


def exact_signals(F, n, seed=3):
    return np.random.default_rng(seed).integers(-8, 9, (F, n)).astype(np.float64)


INSTANCE_N = 203
INSTANCE_CHUNKS = (5, 17, 64)


def instance_case(ns):
    """(sos [2, ns, 6], x [2, INSTANCE_N], zi [2, ns, 2]) of test_sosfilt_every_instance_on_integers[ns]."""
    return cascade(ns, 2), exact_signals(2, INSTANCE_N, seed=100 + ns), cascade_zi(2, ns)


# Butterworth band-passes of n_sections sections (order n_sections: a band-pass doubles it), the bands of `pitch`, `mid12` and `mid16`.
BP_BANDS = ((65, 2100), (200, 2000), (300, 3000))
BP_N = 3000
BP_CHUNKS = (17, 64, 0)
BP_MODES = ("bank_shared", "bank_own")
_BP_PAIRS = ((0, 0), (1, 0), (2, 0), (1, 1), (2, 2))  # (band, signal): the bank over signal 0 and over its own signals


@functools.lru_cache(maxsize=None)
def bp_bank(ns):
    """sos [3, ns, 6]: butter(ns, band, "bp") for the three bands."""
    return np.stack([_butter(ns, list(band), "bp") for band in BP_BANDS])


def bp_signals(mode):
    return (0, 0, 0) if mode == "bank_shared" else (0, 1, 2)


@functools.lru_cache(maxsize=None)
def _bp_longdouble_all():
    """Every (n_sections, band, signal) of the list through the long-double loop in ONE walk over BP_N samples, the filters padded to 16
    sections with identity sections (exact)."""
    keys = [(ns, b, s) for ns in ALL_NS for b, s in _BP_PAIRS]
    sos = np.stack([np.concatenate([bp_bank(ns)[b], np.tile(IDENTITY, (16 - ns, 1))]) for ns, b, _ in keys])
    x = np.stack([signals()[s, :BP_N] for _, _, s in keys])
    y, _ = sequential(sos, x, dtype=np.longdouble)
    return {k: y[i] for i, k in enumerate(keys)}


def bp_longdouble(ns, band, sig):
    return _bp_longdouble_all()[(ns, band, sig)]


def errors_sos(sos, x, chunk, ref):
    """`errors` for any filter: (err_chunked_f64, err_sequential_f64) of sos [ns, 6] over x against the long-double result ``ref``,
    relative to max |ref|; the sequential one is scipy's own."""
    x = np.asarray(x, dtype=np.float64)
    return rel_err(chunked(sos, x, chunk)[0][0], ref), rel_err(scipy.signal.sosfilt(sos, x), ref)


@functools.lru_cache(maxsize=None)
def _bp_errors(ns, chunk):
    """(band, signal) -> (err_chunked_f64, err_sequential_f64) over BP_N samples; the five filters of an order in one chunked walk."""
    sos = np.stack([bp_bank(ns)[b] for b, _ in _BP_PAIRS])
    x = np.stack([signals()[s, :BP_N] for _, s in _BP_PAIRS]).astype(np.float64)
    y = chunked(sos, x, chunk)[0]
    return {(b, s): (rel_err(y[i], bp_longdouble(ns, b, s)), rel_err(scipy.signal.sosfilt(sos[i], x[i]), bp_longdouble(ns, b, s)))
            for i, (b, s) in enumerate(_BP_PAIRS)}


def bp_allowance(ns, band, sig, chunk):
    """The rule of `allowance`, unchanged, for a filter of this list: 4 max(err_chunked_f64, err_sequential_f64, 16 * 2^-53) of the case
    itself (0: the default chunk for BP_N samples), from the numpy restatements alone."""
    return 4.0 * max(*_bp_errors(ns, chunk or default_chunk(BP_N))[(band, sig)], 16 * EPS)


# The chunk grid.  Every class is a bank of two integer cascades (3 or 5 sections) over their own signals from a non-zero state, unless
# it says otherwise: name -> dict(ns, F, n, chunk, shared, sos, zi), the signal from `geometry_operands`.
SOS_TILE, SOS_LANES, SOS_AHEAD = 16, 64, 8  # the documented constants of csrc/iir.hip
MAX_CHUNK, MAX_FILTERS = 65536, 64          # MAUA_SOS_MAX_CHUNK, MAUA_SOS_MAX_FILTERS
LARGEST_CHUNK = MAX_CHUNK                   # the chunk of the largest-chunk class (profiles/iir.md records the time of its call)
TILE_CHUNKS = (1, 15, 16, 17, 31, 33, 100)
NC_AT_5 = (1, 2, 8, 9, 10, 16, 17, 18, 64, 65, 66, 128, 129, 130)
NC_AT_17 = (9, 65, 66)


def _geometry():
    g = {}
    for chunk in TILE_CHUNKS:  # three chunks, the last 1, chunk - 1 or chunk samples long
        for last in sorted({1, chunk} | ({chunk - 1} if chunk - 1 > 1 else set())):
            g[f"chunk{chunk}_last{last}"] = dict(chunk=chunk, n=2 * chunk + last)
    for chunk, counts in ((5, NC_AT_5), (17, NC_AT_17)):  # the carry's look-ahead and the workgroup counts; the last chunk 3 long
        for nc in counts:
            g[f"nc{nc}_chunk{chunk}"] = dict(chunk=chunk, n=(nc - 1) * chunk + 3)
    for turn, (name, case) in enumerate(g.items()):
        ns = (3, 5)[turn % 2]
        case.update(ns=ns, F=2, shared=False, sos=cascade(ns, 2), zi=cascade_zi(2, ns))
    mix = np.stack([EXACT["mix"], EXACT["mix"][::-1]])
    g["chunk4096"] = dict(chunk=4096, n=3 * 4096 + 5, ns=2, F=2, shared=False, sos=mix, zi=cascade_zi(2, 2))
    g["chunk4096_zero_state"] = dict(chunk=4096, n=3 * 4096 + 5, ns=2, F=2, shared=False, sos=mix, zi=None)
    g["largest_chunk"] = dict(chunk=LARGEST_CHUNK, n=2 * LARGEST_CHUNK + 3, ns=1, F=1, shared=True, sos=EXACT["running_sum"][None], zi=None)
    for shared in (True, False):
        g[f"filters64_{'shared' if shared else 'own'}"] = dict(chunk=17, n=203, ns=3, F=MAX_FILTERS, shared=shared,
                                                               sos=cascade(3, MAX_FILTERS), zi=cascade_zi(MAX_FILTERS, 3))
    return g


GEOMETRY = _geometry()


def geometry_operands(name):
    """(sos [F, ns, 6], x [n] or [F, n], zi or None) of a class."""
    case = GEOMETRY[name]
    x = exact_signals(case["F"], case["n"], seed=sorted(GEOMETRY).index(name))
    return case["sos"], (x[0] if case["shared"] else x), case["zi"]


@functools.lru_cache(maxsize=None)
def geometry_reference(name):
    """(y [F, n], zf [F, ns, 2]) in float64, exact: the sequential loop (on these integers it has the bits of the long-double one), but
    for the two classes that start from the zero state y is the vectorised cumsum(convolve(x, [1, 2, 1])) (either order of the two
    sections: they commute from a zero state) and cumsum(x), and the state behind the longest chunk is the sum itself."""
    sos, x, zi = geometry_operands(name)
    if name == "largest_chunk":
        y = np.cumsum(x)[None]
        return y, np.array([[[y[0, -1], 0.0]]])
    if name == "chunk4096_zero_state":
        return np.stack([np.cumsum(np.convolve(row, [1.0, 2.0, 1.0])[: len(row)]) for row in x]), sequential(sos, x)[1]
    return sequential(sos, x, zi=zi)
