"""GPU: every C entry of csrc/signal.hip called directly through the C ABI, at the shapes and edges its kernels have separate code for,
between red zones, against a float64 reference of the same operation.

Each call allocates all device operands through redzone.Guard, runs twice into separate output windows (identical bits required) and
ends with Guard.check: red zones intact, every output element written, every output finite.

Tolerances are NOT taken from the kernels.  For each floating-point entry the same operation is computed on the CPU twice over the case
lists of this module, in float64 and with every operand and intermediate rounded to float32 (numpy float32, scipy.fft keeps float32); the
largest error of the float32 run relative to the stated scale, times 4, is the tolerance (`PYTHONPATH=. python tests/test_signal_entries_gpu.py`
prints the figures without a GPU, the constants below are those rounded up to two digits; fp64-accumulating entries round input and output only):

    entry                scale                       float32 run   tolerance (x4)
    stft_complex         peak                        1.6e-07       6.4e-07
    stft_power           peak                        3.0e-07       1.2e-06
    istft                peak                        3.2e-07       1.3e-06
    roundtrip            peak, hop <= n_fft/4        1.3e-06       5.2e-06
    roundtrip_half       peak, hop == n_fft/2        1.2e-02       4.8e-02
    softmask_apply       peak                        9.6e-08       3.8e-07
    filterbank           per element (rtol)          4.9e-07       2.0e-06
    chroma_cens          absolute (unit L2 frames)   9.2e-08       3.7e-07
    cqt_mag              peak, in/out rounding       5.7e-08       2.3e-07
    resample_f64         peak, in/out rounding       9.1e-08       3.6e-07
    temporal_fir         sum |tap| |x| (rtol)        3.1e-07       1.2e-06
    perlin3d             peak                        4.2e-07       1.7e-06
    affine_reflect_warp  peak                        1.2e-05       4.8e-05

Scales: `peak` = largest |expected| of the call; `filterbank` = |expected| per element (floor 1e-30), in dB max(|expected|, 1 dB);
`temporal_fir` = sum_k |taps[k]| |x[t + k]| per element, which is rtol for operands of one sign and stays meaningful for the signed
random taps used here (plain rtol is ill-conditioned where a signed sum cancels).
Exact-selection results (median filter, nn-median, identity / integer warps, unit-tap FIR, refused calls) are compared bit for bit.
CENS quantises and nn-median selects by order: their inputs are constructed so that the float64 reference is unambiguous (checked before
the kernel runs), and the comparison exempts no element.

cqt_mag on a clip of one or two samples under a 3000-sample filter is a sum that cancels to 1e-11 of its terms; there the float64
reference itself is off by up to 1e-5 of the result's peak (measured against a long-double restatement: 2.0e-6 and 1.1e-5 for the two
failing rows, the very differences the kernel showed).  The comparison therefore adds the reference's own worst-case fp64 bound,
2 eps64 (n + pi f n / sr) sum |y w| / sqrt(n) per bin, to the float32 tolerance: ~1e-14 absolute, nothing for a well-conditioned bin.

cqt_mag with a filter of one sample: the periodic Hann window of one sample is identically zero, so its L1 normalisation is 0 / 0; the
reference here defines the transform under an all-zero window as 0, which is also what the kernel's closed-form window sum gives."""
import numpy as np
import pytest
import scipy.fft
import scipy.ndimage
import scipy.signal
import torch
from hypothesis import given, settings, strategies as st
from numpy.lib.stride_tricks import sliding_window_view

from maua_stylegan2_amd import _lib
from oracle import signal_oracle as so
from redzone import Guard
from test_property_gpu import COMMON

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

EINVAL, ENOSYS = -22, -38
TINY32 = float(np.finfo(np.float32).tiny)
F32, F64 = np.float32, np.float64

# measured float32-vs-float64 figure per entry (see the module docstring); the tolerance is 4 x this
MEASURED = {
    "stft_complex": 1.6e-07,
    "stft_power": 3.0e-07,
    "istft": 3.2e-07,
    "roundtrip": 1.3e-06,  # hop <= n_fft / 4
    "roundtrip_half": 1.2e-02,  # hop == n_fft / 2: the last samples lie under ONE frame's tail, y w / w^2 with w ~ (2 pi / n_fft)^2
    "softmask_apply": 9.6e-08,
    "filterbank": 4.9e-07,
    "chroma_cens": 9.2e-08,
    "cqt_mag": 5.7e-08,
    "resample_f64": 9.1e-08,
    "temporal_fir": 3.1e-07,
    "perlin3d": 4.2e-07,
    "affine_reflect_warp": 1.2e-05,
}
TOL = {k: 4.0 * v for k, v in MEASURED.items()}

# ---------------------------------------------------------------------------------------------------------- calling convention
_TORCH = {np.dtype(F32): torch.float32, np.dtype(F64): torch.float64, np.dtype(np.int32): torch.int32}


class Out:
    def __init__(self, shape, dtype=torch.float32):
        self.shape, self.dtype = tuple(int(s) for s in np.atleast_1d(shape)), dtype


def _materialise(g, spec, tag, cache):
    """spec: [(name, value)] in C order; ndarray -> guarded input (once per Guard), Out -> fresh guarded output, None -> NULL."""
    args, outs = [], {}
    for name, v in spec:
        if isinstance(v, np.ndarray):
            if name not in cache:
                cache[name] = g.inp(v, name, _TORCH[v.dtype])
            args.append(cache[name].data_ptr())
        elif isinstance(v, Out):
            t = g.out(v.shape, name + tag, v.dtype)
            outs[name] = t
            args.append(t.data_ptr())
        else:
            args.append(v)
    return args, outs


def _bits(t):
    return t.reshape(-1).view(torch.int32)


def _run(gpu, entry, spec, nonfinite_ok=False):
    """Call ``entry`` twice on the same guarded inputs into separate output windows: rc == 0, red zones, every output element written and
    finite, identical bits.  Returns {output name: numpy array}."""
    lib = _lib.load()
    g, cache = Guard(gpu), {}
    runs = []
    for tag in ("", "'"):
        args, outs = _materialise(g, spec, tag, cache)
        rc = getattr(lib, entry)(*args, _lib.stream_ptr(gpu))
        assert rc == 0, f"{entry} returned {rc}"
        runs.append(outs)
    names = [n + tag for tag in ("", "'") for n in runs[0]]
    g.check(written=names, nonfinite_ok=names if nonfinite_ok else ())
    for n in runs[0]:
        assert torch.equal(_bits(runs[0][n]), _bits(runs[1][n])), f"{entry}: two runs differ in {n}"
    return {n: t.cpu().numpy() for n, t in runs[0].items()}


def _refused(gpu, entry, spec, rows):
    """Every (override, code) of ``rows`` is refused with that code before anything launches (outputs still all canary), and the valid
    call that follows succeeds (no sticky error state)."""
    lib = _lib.load()
    for over, code in rows:
        g = Guard(gpu)
        args, outs = _materialise(g, [(n, over.get(n, v) if n in over else v) for n, v in spec], "", {})
        rc = getattr(lib, entry)(*args, _lib.stream_ptr(gpu))
        assert rc == code, f"{entry}{over}: returned {rc}, expected {code}"
        for n in outs:
            assert g.untouched(n), f"{entry}{over}: refused, but {n} was written"
        g.check()
    return _run(gpu, entry, spec)


def _rel_peak(got, want):
    want = np.asarray(want)
    peak = float(np.abs(want).max())
    return float(np.abs(np.asarray(got, dtype=want.dtype) - want).max()) / (peak if peak > 0 else 1.0)


def _rng(*key):
    return np.random.default_rng([abs(int(k)) for k in key])


# ---------------------------------------------------------------------------------------------------------- STFT family
N_FFTS = [64, 128, 256, 512, 1024, 2048, 4096]
_PRIME_NEAR_5 = {64: 317, 128: 641, 256: 1279, 512: 2557, 1024: 5119, 2048: 10243, 4096: 20479}


def _stft_cases():
    """(n_fft, hop, n_samples, n_frames): every n_fft x every n_samples kind; the hop kinds and the one-frame form rotate through them so
    that each appears with every n_fft (a hop of 1 or 7 on a long clip is replaced by n_fft / 4: the CPU reference would hold tens of
    thousands of frames)."""
    cases = []
    for i, n_fft in enumerate(N_FFTS):
        ns = [1, 2, 3, n_fft // 2 - 1, n_fft // 2, n_fft // 2 + 1, n_fft, _PRIME_NEAR_5[n_fft]]
        for j, n in enumerate(ns):
            hop = [1, 7, n_fft // 4, n_fft, 3 * n_fft][(i + j) % 5]
            if (1 + n // hop) * n_fft > (1 << 22):
                hop = n_fft // 4
            n_frames = 1 if (i + 2 * j) % 3 == 0 else 1 + n // hop
            cases.append((n_fft, hop, n, n_frames))
    return cases


STFT_CASES = _stft_cases()


def _stft_inputs(case):
    n_fft, hop, n, n_frames = case
    r = _rng(1, *case)
    return r.standard_normal(n).astype(F32), r.uniform(0.1, 1.0, n_fft).astype(F32)  # a non-Hann window: an index slip shows


def _stft_emul(y, win, n_fft, hop, n_frames, dt):
    ypad = np.pad(y.astype(dt), n_fft // 2, mode="reflect")
    fr = sliding_window_view(ypad, n_fft)[::hop][:n_frames].T * win.astype(dt)[:, None]
    return scipy.fft.rfft(fr, axis=0)


def _power(spec):
    return spec.real * spec.real + spec.imag * spec.imag


def _gpu_stft_complex(gpu, y, win, n_fft, hop, n_frames):
    o = _run(gpu, "maua_stft_complex_f32", [("y", y), ("n", len(y)), ("win", win), ("n_fft", n_fft), ("hop", hop),
                                            ("re", Out((n_fft // 2 + 1, n_frames))), ("im", Out((n_fft // 2 + 1, n_frames))),
                                            ("n_frames", n_frames)])
    return o["re"].astype(F64) + 1j * o["im"].astype(F64)


def _gpu_stft_power(gpu, y, win, n_fft, hop, n_frames):
    return _run(gpu, "maua_stft_power_f32", [("y", y), ("n", len(y)), ("win", win), ("n_fft", n_fft), ("hop", hop),
                                             ("p", Out((n_fft // 2 + 1, n_frames))), ("n_frames", n_frames)])["p"]


@pytest.mark.parametrize("case", STFT_CASES, ids=lambda c: "-".join(map(str, c)))
def test_stft_complex_vs_oracle(gpu, case):
    n_fft, hop, n, n_frames = case
    y, win = _stft_inputs(case)
    want = so.stft_complex(y, n_fft, hop, window=win, n_frames=n_frames)
    got = _gpu_stft_complex(gpu, y, win, n_fft, hop, n_frames)
    err = _rel_peak(got, want)
    print(f"stft_complex {case}: err/peak {err:.3e}")
    assert err <= TOL["stft_complex"]


@pytest.mark.parametrize("case", STFT_CASES, ids=lambda c: "-".join(map(str, c)))
def test_stft_power_vs_oracle_and_parseval(gpu, case):
    n_fft, hop, n, n_frames = case
    y, win = _stft_inputs(case)
    want = so.stft_power(y, n_fft, hop, window=win, n_frames=n_frames)
    got = _gpu_stft_power(gpu, y, win, n_fft, hop, n_frames)
    err = _rel_peak(got, want)
    print(f"stft_power {case}: err/peak {err:.3e}")
    assert err <= TOL["stft_power"]
    # Parseval per frame, a witness independent of any FFT: sum_k c_k |X_k|^2 = n_fft sum_i (y_i w_i)^2, c = 1 at DC / Nyquist, else 2
    ypad = np.pad(y.astype(F64), n_fft // 2, mode="reflect")
    fr = sliding_window_view(ypad, n_fft)[::hop][:n_frames].T * win.astype(F64)[:, None]
    c = np.full(n_fft // 2 + 1, 2.0)
    c[0] = c[-1] = 1.0
    energy = n_fft * (fr ** 2).sum(axis=0)
    # the weighted sum of n_fft / 2 + 1 bins, each within TOL * peak
    assert np.abs((c[:, None] * got.astype(F64)).sum(axis=0) - energy).max() <= TOL["stft_power"] * float(want.max()) * n_fft


ISTFT_CASES = [(n_fft, hop, nf, length) for n_fft in N_FFTS
               for hop, nf in [(7, 40), (n_fft // 4, 6), (n_fft, 3), (3 * n_fft, 3)]
               for length in ["short", "cover", "long"]]


def _istft_inputs(case):
    n_fft, hop, nf, length = case
    r = _rng(2, n_fft, hop, nf, len(length))
    cover = n_fft + hop * (nf - 1) - n_fft // 2  # samples the frames reach
    n = {"short": max(cover // 3, 1), "cover": cover, "long": cover + 300}[length]
    # a random complex spectrum: imaginary parts at DC and Nyquist included (an inverse real FFT ignores them)
    re = r.standard_normal((n_fft // 2 + 1, nf)).astype(F32)
    im = r.standard_normal((n_fft // 2 + 1, nf)).astype(F32)
    return re, im, r.uniform(0.1, 1.0, n_fft).astype(F32), n


def _istft_emul(re, im, win, n_fft, hop, length, dt):
    nf = re.shape[1]
    spec = (re.astype(dt) + 1j * im.astype(dt)).astype(np.complex64 if dt == F32 else np.complex128)
    w = win.astype(dt)
    fr = scipy.fft.irfft(spec, n=n_fft, axis=0).astype(dt) * w[:, None]
    total = max(n_fft + hop * (nf - 1), n_fft // 2 + length)
    y, wss = np.zeros(total, dt), np.zeros(total, dt)
    for t in range(nf):
        y[t * hop: t * hop + n_fft] += fr[:, t]
        wss[t * hop: t * hop + n_fft] += w * w
    ok = wss > TINY32
    y[ok] /= wss[ok]
    return y[n_fft // 2: n_fft // 2 + length]


def _gpu_istft(gpu, re, im, win, n_fft, hop, n):
    nf = re.shape[1]
    return _run(gpu, "maua_istft_f32", [("re", re), ("im", im), ("win", win), ("n_fft", n_fft), ("hop", hop), ("n_frames", nf),
                                        ("frames_ws", Out((nf, n_fft))), ("y", Out((n,))), ("n", n)])["y"]


@pytest.mark.parametrize("case", ISTFT_CASES, ids=lambda c: "-".join(map(str, c)))
def test_istft_vs_oracle(gpu, case):
    n_fft, hop, nf, _ = case
    re, im, win, n = _istft_inputs(case)
    assert np.abs(im[0]).min() > 0 and np.abs(im[-1]).min() > 0
    want = so.istft(re.astype(F64) + 1j * im.astype(F64), n, n_fft, hop, window=win)
    got = _gpu_istft(gpu, re, im, win, n_fft, hop, n)
    err = _rel_peak(got, want)
    print(f"istft {case}: err/peak {err:.3e}")
    assert err <= TOL["istft"]
    reached = np.zeros(n + n_fft, bool)
    for t in range(nf):
        reached[max(t * hop - n_fft // 2, 0): max(t * hop + n_fft - n_fft // 2, 0)] = True
    assert np.all(got[~reached[:n]] == 0.0)  # samples no frame reaches (beyond the cover, gaps when hop > n_fft): the wss floor


ROUNDTRIP_CASES = [(n_fft, hop, n) for n_fft in N_FFTS for hop in (1, 7, n_fft // 4, n_fft // 2)
                   for n in (1, 2, 3, n_fft // 2 - 1, n_fft // 2, n_fft // 2 + 1, n_fft, _PRIME_NEAR_5[n_fft])
                   if (1 + n // hop) * n_fft <= (1 << 20)]


def _roundtrip_emul(y, n_fft, hop, dt):
    win = so.hann_periodic(n_fft).astype(F32)
    spec = _stft_emul(y, win, n_fft, hop, 1 + len(y) // hop, dt)
    return _istft_emul(spec.real, spec.imag, win, n_fft, hop, len(y), dt)


@pytest.mark.parametrize("n_fft", N_FFTS)
def test_istft_inverts_stft(gpu, n_fft):
    """istft(stft_complex(y)) == y with the periodic Hann window for every hop <= n_fft / 2 and clip length of the case list."""
    win = so.hann_periodic(n_fft).astype(F32)
    for _, hop, n in [c for c in ROUNDTRIP_CASES if c[0] == n_fft]:
        y = _rng(3, n_fft, hop, n).standard_normal(n).astype(F32)
        nf = 1 + n // hop
        spec = _gpu_stft_complex(gpu, y, win, n_fft, hop, nf)
        back = _gpu_istft(gpu, spec.real.astype(F32), spec.imag.astype(F32), win, n_fft, hop, n)
        err = _rel_peak(back, y.astype(F64))
        print(f"roundtrip {(n_fft, hop, n)}: err/peak {err:.3e}")
        assert err <= TOL["roundtrip_half" if hop == n_fft // 2 else "roundtrip"], (n_fft, hop, n)


def test_stft_family_refusals(gpu):
    y, win = _rng(4).standard_normal(300).astype(F32), np.ones(128, F32)
    bad = [({"n_fft": v}, EINVAL) for v in (0, -128, 32, 96, 100, 127, 129, 8192)]
    bad += [({"n": 0}, EINVAL), ({"hop": 0}, EINVAL), ({"hop": -1}, EINVAL), ({"n_frames": 0}, EINVAL), ({"y": None}, EINVAL),
            ({"win": None}, EINVAL)]
    spec = [("y", y), ("n", 300), ("win", win), ("n_fft", 128), ("hop", 32), ("p", Out((65, 10))), ("n_frames", 10)]
    _refused(gpu, "maua_stft_power_f32", spec, bad + [({"p": None}, EINVAL)])
    spec = spec[:5] + [("re", Out((65, 10))), ("im", Out((65, 10))), ("n_frames", 10)]
    _refused(gpu, "maua_stft_complex_f32", spec, bad + [({"re": None}, EINVAL), ({"im": None}, EINVAL)])
    re = _rng(5).standard_normal((65, 10)).astype(F32)
    spec = [("re", re), ("im", re[::-1].copy()), ("win", win), ("n_fft", 128), ("hop", 32), ("n_frames", 10),
            ("frames_ws", Out((10, 128))), ("y", Out((300,))), ("n", 300)]
    _refused(gpu, "maua_istft_f32", spec, [b for b in bad if "y" not in b[0]] +
             [({"re": None}, EINVAL), ({"im": None}, EINVAL), ({"frames_ws": None}, EINVAL), ({"y": None}, EINVAL)])


# ---------------------------------------------------------------------------------------------------------- median filter
MEDIAN_SIZES = [3, 5, 9, 17, 31]


def _median_ref(x, size, axis):
    """scipy.ndimage 'reflect' where the axis is at least size // 2 long; below that a sliding median over numpy's periodic symmetric
    padding (d c b a | a b c d | d c b a, any number of folds), which scipy does not follow reliably there."""
    if x.shape[axis] >= size // 2:
        return scipy.ndimage.median_filter(x, size=(size, 1) if axis == 0 else (1, size), mode="reflect")
    pad = [(0, 0), (0, 0)]
    pad[axis] = (size // 2, size // 2)
    win = sliding_window_view(np.pad(x, pad, mode="symmetric"), size, axis=axis)
    return np.sort(win, axis=-1)[..., size // 2]


def _median_input(rows, cols, seed, special=True):
    r = _rng(6, rows, cols, seed)
    x = (np.round(r.standard_normal((rows, cols)) * 4) / 2).astype(F32)  # multiples of 0.5: heavy ties
    if special and x.size >= 8:
        flat = x.reshape(-1)
        idx = r.choice(x.size, size=max(x.size // 16, 4), replace=False)
        flat[idx] = r.choice(np.array([0.0, -0.0, np.inf, -np.inf], F32), size=len(idx))
    return x


def _gpu_median(gpu, x, size, axis):
    rows, cols = x.shape
    return _run(gpu, "maua_median_filter_f32", [("x", x), ("y", Out(x.shape)), ("rows", rows), ("cols", cols), ("size", size),
                                                ("axis", axis)], nonfinite_ok=True)["y"]


def _same_bits(got, want):
    """Bit for bit, except that the sign of a zero median is free (the order of tied +0.0 and -0.0 is not defined)."""
    want = np.asarray(want, dtype=F32)
    return got.shape == want.shape and np.array_equal(got, want) and np.array_equal(got.view(np.int32)[want != 0], want.view(np.int32)[want != 0])


MEDIAN_SHAPES = [(1, 1), (1, 37), (37, 1), (29, 31), (70, 45)] + [(n, 19) for n in (1, 2, 3, 14, 15, 16)] + \
    [(19, n) for n in (2, 3, 14, 15, 16)]


@pytest.mark.parametrize("size", MEDIAN_SIZES)
@pytest.mark.parametrize("axis", [0, 1])
def test_median_filter_every_size_and_short_axes(gpu, size, axis):
    for rows, cols in MEDIAN_SHAPES:
        x = _median_input(rows, cols, size)
        assert _same_bits(_gpu_median(gpu, x, size, axis), _median_ref(x, size, axis)), (rows, cols, size, axis)


@pytest.mark.parametrize("size,axis", [(3, 0), (17, 1), (31, 0)])
def test_median_filter_second_grid_stride_trip(gpu, size, axis):
    rows, cols = 1031, 2039  # primes; rows * cols > 8192 workgroups * 256 threads
    assert rows * cols > 8192 * 256
    x = _median_input(rows, cols, size)
    assert _same_bits(_gpu_median(gpu, x, size, axis), _median_ref(x, size, axis))


@settings(max_examples=25, **COMMON)
@given(rows=st.integers(1, 40), cols=st.integers(1, 40), size=st.sampled_from(MEDIAN_SIZES), axis=st.integers(0, 1),
       seed=st.integers(0, 1 << 16))
def test_median_filter_random_calls(gpu, rows, cols, size, axis, seed):
    x = _median_input(rows, cols, seed)
    assert _same_bits(_gpu_median(gpu, x, size, axis), _median_ref(x, size, axis))


@pytest.mark.parametrize("size", MEDIAN_SIZES)
def test_median_filter_constant_and_ramp(gpu, size):
    const = np.full((23, 41), 1.25, F32)
    ramp = (np.arange(41, dtype=F32) * 0.5 - 3)[None, :].repeat(23, 0)
    for axis in (0, 1):
        assert np.array_equal(_gpu_median(gpu, const, size, axis), const)
    got = _gpu_median(gpu, ramp, size, 1)
    h = size // 2
    assert np.array_equal(got[:, h: 41 - h], ramp[:, h: 41 - h])  # the interior of a monotone ramp is its own median
    assert np.array_equal(_gpu_median(gpu, ramp, size, 0), ramp)  # constant along the other axis


def test_median_filter_refusals(gpu):
    x = _median_input(9, 11, 0, special=False)
    spec = [("x", x), ("y", Out(x.shape)), ("rows", 9), ("cols", 11), ("size", 5), ("axis", 1)]
    _refused(gpu, "maua_median_filter_f32", spec,
             [({"size": s}, ENOSYS) for s in (7, 33, 4, 0, -3, 1)] +
             [({"rows": 0}, EINVAL), ({"cols": -1}, EINVAL), ({"axis": 2}, EINVAL), ({"axis": -1}, EINVAL), ({"x": None}, EINVAL),
              ({"y": None}, EINVAL)])


# ---------------------------------------------------------------------------------------------------------- soft mask
SOFTMASK_N = 4096 * 256 + 77
SOFTMASK_CASES = [(p, m, s) for p in (1.0, 2.0, 0.5) for m in (1.0, 4.0) for s in (0, 1)]


def _softmask_inputs(n=SOFTMASK_N):
    r = _rng(7, n)
    xs, xr = np.abs(r.standard_normal(n)).astype(F32), np.abs(r.standard_normal(n)).astype(F32)
    edge = [(0, 0), (1e-40, 1e-40), (1e-40, 0), (0, 1e-40), (0, 1.5), (1.5, 0), (1e-40, 2.0), (3.0, 1e-40), (1e-30, 1e-30), (1e-38, 0.0)]
    for i, (a, b) in enumerate(edge):  # both zero / denormal / one zero, at both ends of the array
        xs[i], xr[i] = a, b
        xs[n - 1 - i], xr[n - 1 - i] = b, a
    return r.standard_normal(n).astype(F32), r.standard_normal(n).astype(F32), xs, xr


def _softmask_emul(re, im, xs, xr, margin, power, split, dt):
    a, b = xs.astype(dt), xr.astype(dt) * dt(margin)
    z = np.maximum(a, b)
    bad = z < TINY32
    z = np.where(bad, dt(1), z)
    pa, pb = (a / z) ** dt(power), (b / z) ** dt(power)
    m = np.where(bad, dt(0.5 if split else 0.0), pa / np.where(bad, dt(1), pa + pb))
    return re.astype(dt) * m, im.astype(dt) * m


def _softmask_want(re, im, xs, xr, margin, power, split):
    m = so.softmask(xs.astype(F64), xr.astype(F64) * margin, power, bool(split))
    return re.astype(F64) * m, im.astype(F64) * m


def _gpu_softmask(gpu, re, im, xs, xr, margin, power, split):
    n = len(re)
    o = _run(gpu, "maua_softmask_apply_f32", [("re", re), ("im", im), ("x", xs), ("x_ref", xr), ("margin", margin), ("power", power),
                                              ("split", split), ("out_re", Out((n,))), ("out_im", Out((n,))), ("n", n)])
    return o["out_re"], o["out_im"]


@pytest.mark.parametrize("power,margin,split", SOFTMASK_CASES)
def test_softmask_apply_vs_oracle(gpu, power, margin, split):
    re, im, xs, xr = _softmask_inputs()
    want = np.stack(_softmask_want(re, im, xs, xr, margin, power, split))
    got = np.stack(_gpu_softmask(gpu, re, im, xs, xr, margin, power, split))
    err = _rel_peak(got, want)
    print(f"softmask {(power, margin, split)}: err/peak {err:.3e}")
    assert err <= TOL["softmask_apply"]
    # where both medians underflow the mask is exactly 0.5 (split) or 0; where one is zero it is exactly 0 or 1
    k = 6
    assert np.array_equal(got[:, :k], want[:, :k].astype(F32)) and np.array_equal(got[:, -k:], want[:, -k:].astype(F32))


@pytest.mark.parametrize("power", [1.0, 2.0, 0.5])
def test_softmask_pair_sums_to_one(gpu, power):
    re, im, xs, xr = _softmask_inputs(70001)
    a = np.stack(_gpu_softmask(gpu, re, im, xs, xr, 1.0, power, 1)).astype(F64)
    b = np.stack(_gpu_softmask(gpu, re, im, xr, xs, 1.0, power, 1)).astype(F64)
    d = np.stack([re, im]).astype(F64)
    assert np.abs(a + b - d).max() <= 2 * TOL["softmask_apply"] * np.abs(d).max()


def test_softmask_refusals(gpu):
    re, im, xs, xr = _softmask_inputs(333)
    spec = [("re", re), ("im", im), ("x", xs), ("x_ref", xr), ("margin", 1.0), ("power", 2.0), ("split", 0), ("out_re", Out((333,))),
            ("out_im", Out((333,))), ("n", 333)]
    _refused(gpu, "maua_softmask_apply_f32", spec, [({"n": 0}, EINVAL), ({"n": -5}, EINVAL)] +
             [({k: None}, EINVAL) for k in ("re", "im", "x", "x_ref", "out_re", "out_im")])


# ---------------------------------------------------------------------------------------------------------- filterbank
AMIN = 1e-10
FILTERBANK_CASES = [(m, k, n, db) for (m, k, n) in [(1, 1, 1), (128, 1025, 1), (12, 252, 257), (24, 1025, 1000)] for db in (0, 1)]


def _filterbank_inputs(case):
    m, k, n, _ = case
    r = _rng(8, m, k, n)
    fb = (r.random((m, k)) * (r.random((m, k)) < 0.3)).astype(F32)  # sparse and non-negative, as mel / chroma banks are
    if m * k == 1:
        fb[:] = 0.75
    p = (r.random((k, n)) ** 4 * 100).astype(F32)
    if n >= 8:
        p[:, 3] = 0.0  # a column that sums to zero
        p[:, 5] *= F32(1e-16)  # ... and one below amin
    return fb, p


def _filterbank_emul(fb, p, db, dt):
    acc = fb.astype(dt) @ p.astype(dt)
    return dt(10) * np.log10(np.maximum(dt(AMIN), acc)) if db else acc


def _filterbank_err(got, want, db):
    want = np.asarray(want, F64)
    return float((np.abs(np.asarray(got, F64) - want) / np.maximum(np.abs(want), 1.0 if db else 1e-30)).max())


@pytest.mark.parametrize("case", FILTERBANK_CASES, ids=lambda c: "-".join(map(str, c)))
def test_filterbank_vs_float64_matmul(gpu, case):
    m, k, n, db = case
    fb, p = _filterbank_inputs(case)
    want = _filterbank_emul(fb, p, db, F64)
    got = _run(gpu, "maua_filterbank_f32", [("fb", fb), ("p", p), ("out", Out((m, n))), ("m", m), ("k", k), ("n", n), ("to_db", db),
                                            ("amin", AMIN)])["out"]
    err = _filterbank_err(got, want, db)
    print(f"filterbank {case}: rel err {err:.3e}")
    assert err <= TOL["filterbank"]
    if n >= 8 and not db:
        assert np.all(got[:, 3] == 0.0)


def test_filterbank_refusals(gpu):
    fb, p = _filterbank_inputs((3, 7, 9, 0))
    spec = [("fb", fb), ("p", p), ("out", Out((3, 9))), ("m", 3), ("k", 7), ("n", 9), ("to_db", 0), ("amin", AMIN)]
    _refused(gpu, "maua_filterbank_f32", spec, [({k: v}, EINVAL) for k in "mkn" for v in (0, -1)] +
             [({k: None}, EINVAL) for k in ("fb", "p", "out")])


# ---------------------------------------------------------------------------------------------------------- CENS
CENS_STEPS = (0.05, 0.1, 0.2, 0.4)
CENS_CASES = sorted({(b, w, t) for b in (1, 12, 32) for w in (1, 3, 41, 255) for t in (1, 2, w // 2, 255, 256, 257, 1000) if t >= 1})


def _cens_unambiguous(ch):
    l1 = np.abs(ch.astype(F64)).sum(axis=0, keepdims=True)
    c = ch.astype(F64) / np.where(l1 > TINY32, l1, 1.0)
    return np.min(np.abs(c[..., None] - np.array(CENS_STEPS)), axis=-1) > 1e-5


def _cens_input(case):
    """|N(0,1)| chromagram with all-zero frames, nudged until no L1-normalised value lies within 1e-5 of a quantiser step (about 100
    float32 ulps at 0.1, against the ~32 a float32 L1 sum over 32 bins can move it)."""
    b, w, t = case
    r = _rng(9, b, w, t)
    ch = np.abs(r.standard_normal((b, t))).astype(F32)
    if t >= 2:
        ch[:, r.choice(t, size=max(t // 10, 1), replace=False)] = 0.0
    for _ in range(8):
        ok = _cens_unambiguous(ch)
        if ok.all():
            break
        ch = np.where(ok, ch, ch * F32(1.001)).astype(F32)
    return ch


def _cens_emul(ch, win_len, dt):
    ch = ch.astype(dt)
    l1 = np.abs(ch).sum(axis=0, keepdims=True, dtype=dt)
    c = ch / np.where(l1 > TINY32, l1, dt(1))
    q = np.zeros_like(c)
    for thr in (0.4, 0.2, 0.1, 0.05):
        q += dt(0.25) * (c > dt(thr))
    n = win_len + 2
    win = (dt(0.5) - dt(0.5) * np.cos(dt(2 * np.pi) * np.arange(n, dtype=dt) / dt(n - 1)))[1:-1]
    win = (win / win.sum(dtype=dt)).astype(dt)
    half = win_len // 2
    padded = np.pad(q, ((0, 0), (half, half)))
    sm = (sliding_window_view(padded, win_len, axis=1) * win[::-1]).sum(axis=-1, dtype=dt)
    l2 = np.sqrt((sm * sm).sum(axis=0, keepdims=True, dtype=dt))
    return sm / np.where(l2 > TINY32, l2, dt(1))


def _gpu_cens(gpu, ch, win_len):
    b, t = ch.shape
    return _run(gpu, "maua_chroma_cens_f32", [("ch", ch), ("out", Out((b, t))), ("n_bins", b), ("n_frames", t), ("win_len", win_len)])["out"]


@pytest.mark.parametrize("case", CENS_CASES, ids=lambda c: "-".join(map(str, c)))
def test_chroma_cens_vs_oracle(gpu, case):
    b, w, t = case
    ch = _cens_input(case)
    assert _cens_unambiguous(ch).all()  # the reference's quantisation does not depend on float32 rounding
    want = so.cens_from_chroma(ch, win_len=w)
    got = _gpu_cens(gpu, ch, w)
    err = float(np.abs(got - want).max())
    print(f"chroma_cens {case}: abs err {err:.3e}")
    assert err <= TOL["chroma_cens"]


def test_chroma_cens_hand_built_levels(gpu):
    """One frame whose L1-normalised values 0.02 / 0.07 / 0.15 / 0.3 / 0.46 sit well inside the five quantiser levels."""
    ch = (np.array([0.02, 0.07, 0.15, 0.3, 0.46]) * 8).astype(F32)[:, None]
    q = np.array([0.0, 0.25, 0.5, 0.75, 1.0])
    got = _gpu_cens(gpu, ch, 1)
    assert np.abs(got[:, 0] - q / np.sqrt((q ** 2).sum())).max() <= TOL["chroma_cens"]
    # the same frame among zero frames under a 3-tap window: its neighbours get the same direction, everything else stays zero
    seq = np.zeros((5, 9), F32)
    seq[:, 4] = ch[:, 0]
    got = _gpu_cens(gpu, seq, 3)
    want = np.zeros((5, 9))
    want[:, 3:6] = (q / np.sqrt((q ** 2).sum()))[:, None]
    assert np.abs(got - want).max() <= TOL["chroma_cens"]


def test_chroma_cens_refusals(gpu):
    ch = _cens_input((12, 41, 50))
    spec = [("ch", ch), ("out", Out((12, 50))), ("n_bins", 12), ("n_frames", 50), ("win_len", 41)]
    _refused(gpu, "maua_chroma_cens_f32", spec,
             [({"n_bins": v}, EINVAL) for v in (0, -1, 33)] + [({"win_len": v}, EINVAL) for v in (0, -1, 2, 40, 256, 257)] +
             [({"n_frames": 0}, EINVAL), ({"ch": None}, EINVAL), ({"out": None}, EINVAL)])


# ---------------------------------------------------------------------------------------------------------- nn-median
def _nn_cases():
    cases = []
    for b in (1, 12, 32):
        for t in (2, 3, 257):
            ks = {2: [1], 3: [1, 2], 257: [1, 2, 33, 256]}[t]
            for k in ks:
                for width in (1, 3, t // 2 + 2):
                    cases.append((b, t, k, width))
    return cases


NN_CASES = _nn_cases()


def _nn_input(case):
    b, t, k, width = case
    r = _rng(10, *case)
    if b == 1:  # signed powers of two: every cosine similarity is exactly +-1 on both sides, the index rule decides
        ch = (r.choice([-1.0, 1.0], size=(1, t)) * 2.0 ** r.integers(-3, 4, size=(1, t))).astype(F32)
    else:
        ch = r.standard_normal((b, t)).astype(F32)
    if t >= 3:  # duplicate frames: exact similarity ties, the lower index wins
        ch[:, t - 1] = ch[:, 0]
    if t > 100:
        ch[:, 40:44] = ch[:, 7:8]
        ch[:, 200] = ch[:, 100]
    return ch


def _nn_unambiguous(ch, k, width):
    """For every frame the k-th and (k+1)-th best admissible similarity differ by more than 1e-12 (both sides compute them in fp64; only
    the summation order differs), unless the two frames are exact copies (either choice gives the same values) or there is one bin
    (each similarity is a single exact product of +-1)."""
    ch = ch.astype(F64)
    b, t = ch.shape
    unit = ch / np.sqrt((ch ** 2).sum(axis=0))
    sim = unit.T @ unit
    idx = np.arange(t)
    for i in range(t):
        s = sim[i].copy()
        s[np.abs(idx - i) < width] = -np.inf
        order = np.argsort(-s, kind="stable")
        if k >= t:
            continue
        a, c = order[k - 1], order[k]
        if s[a] == -np.inf or s[a] - s[c] > 1e-12 or b == 1 or np.array_equal(ch[:, a], ch[:, c]):
            continue
        return False
    return True


@pytest.mark.parametrize("case", NN_CASES, ids=lambda c: "-".join(map(str, c)))
def test_nn_median_vs_oracle_both_paths(gpu, case):
    b, t, k, width = case
    ch = _nn_input(case)
    assert _nn_unambiguous(ch, k, width)
    want = so.nn_filter_median(ch, width=width, k=k).astype(F32)
    spec = [("ch", ch), ("out", Out((b, t))), ("n_bins", b), ("n_frames", t), ("k", k), ("width", width), ("ws", None)]
    lds = _run(gpu, "maua_nn_median_f32", spec)["out"]
    spec[-1] = ("ws", Out((min(t, 1024), t), torch.float64))
    wsp = _run(gpu, "maua_nn_median_f32", spec, nonfinite_ok=True)["out"]  # (the workspace holds -inf for excluded frames)
    assert np.array_equal(lds.view(np.int32), wsp.view(np.int32)), "LDS path and workspace path differ"
    assert np.array_equal(lds.view(np.int32), want.view(np.int32))


def test_nn_median_refusals(gpu):
    ch = _nn_input((12, 50, 5, 1))
    spec = [("ch", ch), ("out", Out((12, 50))), ("n_bins", 12), ("n_frames", 50), ("k", 5), ("width", 1), ("ws", None)]
    _refused(gpu, "maua_nn_median_f32", spec,
             [({"n_bins": v}, EINVAL) for v in (0, 33)] + [({"k": v}, EINVAL) for v in (0, -1, 50, 51, 4000)] +
             [({"n_frames": 1}, EINVAL), ({"n_frames": 0}, EINVAL), ({"width": 0}, EINVAL), ({"ch": None}, EINVAL), ({"out": None}, EINVAL),
              ({"n_frames": 30000, "k": 5}, EINVAL)])  # a similarity row beyond LDS needs the caller's workspace


# ---------------------------------------------------------------------------------------------------------- constant-Q magnitude
CQT_SR = 22050.0
CQT_EDGE_LENGTHS = [1, 255, 256, 257, 3000]
CQT_CASES = [(b, n, hop) for b in (1, 36) for n in (1, 2, 1000) for hop in (1, 512)]


def _cqt_inputs(case, j=0):
    b, n, hop = case
    r = _rng(11, b, n, hop, j)
    y = r.standard_normal(n).astype(F32)
    freqs = r.uniform(30.0, 8000.0, b).astype(F32)
    if b == 1:
        lengths = np.array([CQT_EDGE_LENGTHS[j]], np.int32)
    else:
        lengths = np.concatenate([CQT_EDGE_LENGTHS, r.integers(2, 600, b - len(CQT_EDGE_LENGTHS))]).astype(np.int32)
    return y, freqs, lengths


def _cqt_ref(y, freqs, lengths, hop, n_frames):
    """so.cqt_magnitude's definition with the filter lengths as an argument (float64; freqs and sr are the float32 values the entry
    receives).  An all-zero window (one sample of a periodic Hann) has no L1 normalisation: that bin is 0."""
    y = y.astype(F64)
    pad = int(lengths.max()) // 2 + 1
    ypad = np.pad(y, pad, mode="reflect")
    out, slack = np.zeros((len(lengths), n_frames)), np.zeros((len(lengths), 1))
    for k, n in enumerate(int(v) for v in lengths):
        m = np.arange(n)
        win = 0.5 - 0.5 * np.cos(2.0 * np.pi * m / n)
        if win.sum() == 0.0:
            continue
        cyc = float(freqs[k]) / float(F32(CQT_SR))
        kern = win / win.sum() * np.exp(-2j * np.pi * cyc * (m - n // 2))
        idx = pad - n // 2 + hop * np.arange(n_frames)[:, None] + m[None, :]
        out[k] = np.abs(ypad[idx] @ kern) / np.sqrt(n)
        # fp64's own error in an n-term sum with phases up to pi cyc n, relative to the sum of |terms| (reference and kernel each)
        slack[k] = 2 * np.finfo(F64).eps * (n + np.pi * cyc * n) * (np.abs(ypad[idx]) @ np.abs(kern)).max() / np.sqrt(n)
    return out, slack


@pytest.mark.parametrize("case", CQT_CASES, ids=lambda c: "-".join(map(str, c)))
def test_cqt_mag_vs_definition(gpu, case):
    b, n, hop = case
    n_frames = 1 + n // hop
    for j in range(len(CQT_EDGE_LENGTHS) if b == 1 else 1):
        y, freqs, lengths = _cqt_inputs(case, j)
        want, slack = _cqt_ref(y, freqs, lengths, hop, n_frames)
        got = _run(gpu, "maua_cqt_mag_f32", [("y", y), ("n", n), ("freqs", freqs), ("lengths", lengths), ("n_bins", b), ("hop", hop),
                                             ("sr", CQT_SR), ("out", Out((b, n_frames))), ("n_frames", n_frames)])["out"]
        err = _rel_peak(got, want)
        print(f"cqt_mag {case} lengths[0]={lengths[0]}: err/peak {err:.3e}")
        assert np.all(np.abs(got - want) <= TOL["cqt_mag"] * want.max() + slack), (case, j)


def test_cqt_mag_refusals(gpu):
    y, freqs, lengths = _cqt_inputs((36, 1000, 512))
    spec = [("y", y), ("n", 1000), ("freqs", freqs), ("lengths", lengths), ("n_bins", 36), ("hop", 512), ("sr", CQT_SR),
            ("out", Out((36, 2))), ("n_frames", 2)]
    _refused(gpu, "maua_cqt_mag_f32", spec,
             [({"n": 0}, EINVAL), ({"n_bins": 0}, EINVAL), ({"n_bins": 65536}, EINVAL), ({"hop": 0}, EINVAL), ({"sr": 0.0}, EINVAL),
              ({"sr": -1.0}, EINVAL), ({"n_frames": 0}, EINVAL)] + [({k: None}, EINVAL) for k in ("y", "freqs", "lengths", "out")])


# ---------------------------------------------------------------------------------------------------------- resample
RESAMPLE_CASES = [(n, num, f) for (n, num) in [(1, 5), (5, 1), (2, 3), (3, 2), (2, 2), (1293, 900), (900, 1293), (7, 4096)]
                  for f in (1, 15, 16, 17, 33)]


def _resample_input(case):
    n, num, f = case
    return _rng(12, *case).standard_normal((n, f))


@pytest.mark.parametrize("case", RESAMPLE_CASES, ids=lambda c: "-".join(map(str, c)))
def test_resample_f64_vs_scipy(gpu, case):
    n, num, f = case
    x = _resample_input(case)
    want = so.resample(x, num)
    assert np.isfinite(want).all()
    got = _run(gpu, "maua_resample_f64", [("x", x), ("n", n), ("features", f), ("y", Out((num, f), torch.float64)), ("num", num)])["y"]
    err = _rel_peak(got, want)
    print(f"resample {case}: err/peak {err:.3e}")
    assert err <= TOL["resample_f64"]


def test_resample_refusals(gpu):
    x = _resample_input((6, 4, 3))
    spec = [("x", x), ("n", 6), ("features", 3), ("y", Out((4, 3), torch.float64)), ("num", 4)]
    _refused(gpu, "maua_resample_f64", spec,
             [({"n": 0}, EINVAL), ({"num": 0}, EINVAL), ({"features": 0}, EINVAL), ({"n": 1 << 21, "num": (1 << 20) + 1}, EINVAL),
              ({"features": 65536 * 16}, EINVAL), ({"x": None}, EINVAL), ({"y": None}, EINVAL)])


# ---------------------------------------------------------------------------------------------------------- temporal FIR
FIR_TS = [1, 2, 31, 32, 33, 65]
FIR_FEATURES = [1, 255, 256, 257]


def _fir_radii(T):
    return sorted({0, 1, 15, 16, 17, 47, 48, max(T - 1, 0), T, T + 1, 2 * T, 3 * T})


def _fir_inputs(T, radius, F):
    r = _rng(13, T, radius, F)
    return r.standard_normal((T, F)).astype(F32), r.uniform(-1.0, 1.0, 2 * radius + 1).astype(F32)  # arbitrary, asymmetric taps


def _fir_emul(x, taps, radius, dt):
    """y[t] = sum_k taps[k] xpad[t + k], xpad[i] = x[(i - radius) mod T] within one wrap either side (-T <= i - radius < 2 T), 0 beyond
    (the kernel's comment; so.gaussian_filter pads the same way).  Returns (y, sum_k |taps[k]| |xpad[t + k]|)."""
    T = x.shape[0]
    i = np.arange(T)[:, None] + np.arange(2 * radius + 1)[None, :] - radius
    inside = (i >= -T) & (i < 2 * T)
    g = x.astype(dt)[np.where(inside, i % T, 0)] * inside[..., None].astype(dt)  # [T, taps, F]
    t = taps.astype(dt)
    return np.einsum("k,tkf->tf", t, g), np.einsum("k,tkf->tf", np.abs(t), np.abs(g))


def _fir_err(got, want, scale):
    return float((np.abs(np.asarray(got, F64) - want) / np.maximum(scale, 1e-30)).max())


def _gpu_fir(gpu, x, taps, radius, nonfinite_ok=False):
    T, F = x.shape
    return _run(gpu, "maua_temporal_fir_f32", [("x", x), ("taps", taps), ("y", Out((T, F))), ("T", T), ("F", F), ("radius", radius)],
                nonfinite_ok=nonfinite_ok)["y"]


@pytest.mark.parametrize("T", FIR_TS)
def test_temporal_fir_arbitrary_taps(gpu, T):
    worst = 0.0
    for radius in _fir_radii(T):
        for F in FIR_FEATURES:
            x, taps = _fir_inputs(T, radius, F)
            want, scale = _fir_emul(x, taps, radius, F64)
            err = _fir_err(_gpu_fir(gpu, x, taps, radius), want, scale)
            worst = max(worst, err)
            assert err <= TOL["temporal_fir"], (T, radius, F, err)
    print(f"temporal_fir T={T}: worst err/scale {worst:.3e}")


@pytest.mark.parametrize("T", [5, 32, 33])
def test_temporal_fir_unit_tap_is_a_shift(gpu, T):
    """A single unit tap at offset d moves every sample by d, bit for bit: circular inside one wrap, zero beyond it."""
    x = _rng(14, T).standard_normal((T, 70)).astype(F32)
    for d in sorted({0, 1, -1, T - 1, -(T - 1), T, -T, T + 1, -(T + 2), 2 * T, -2 * T, 3 * T - 1}):
        radius = abs(d) + 1
        taps = np.zeros(2 * radius + 1, F32)
        taps[radius + d] = 1.0
        src = np.arange(T) + d
        want = np.where(((src >= -T) & (src < 2 * T))[:, None], x[src % T], F32(0))
        assert np.array_equal(_gpu_fir(gpu, x, taps, radius), want), (T, d)


def test_temporal_fir_radius_limit_and_refusals(gpu):
    T, F, radius = 5, 3, 8143  # the largest radius whose padded taps fit 64 KB of LDS
    x, taps = _fir_inputs(T, radius, F)
    want, scale = _fir_emul(x, taps, radius, F64)
    assert _fir_err(_gpu_fir(gpu, x, taps, radius), want, scale) <= TOL["temporal_fir"]
    spec = [("x", x), ("taps", taps), ("y", Out((T, F))), ("T", T), ("F", F), ("radius", radius)]
    _refused(gpu, "maua_temporal_fir_f32", spec,
             [({"radius": 8144}, EINVAL), ({"radius": -1}, EINVAL), ({"radius": 100000}, EINVAL), ({"T": 0}, EINVAL), ({"F": 0}, EINVAL),
              ({"F": -1}, EINVAL), ({"F": 1 << 40}, EINVAL)] + [({k: None}, EINVAL) for k in ("x", "taps", "y")])


# ---------------------------------------------------------------------------------------------------------- Perlin noise
PERLIN_CASES = [(4, 4, 4, 4, 4, 4), (8, 6, 10, 1, 1, 1), (12, 8, 20, 3, 2, 5), (6, 6, 6, 6, 3, 1), (64, 64, 64, 4, 8, 2)]


def _perlin_inputs(case):
    res = case[3:]
    r = _rng(15, *case)
    shp = tuple(v + 1 for v in res)
    return 2 * np.pi * r.random(shp), 2 * np.pi * r.random(shp)


def _perlin_grad(theta, phi):
    g = np.stack([np.sin(phi) * np.cos(theta), np.sin(phi) * np.sin(theta), np.cos(phi)], axis=3)
    g[-1] = g[0]  # tileable along the first axis, as so.perlin_noise defaults to
    return g


def _perlin_emul(grad, shape, res, dt):
    g = grad.astype(dt)
    d = [shape[i] // res[i] for i in range(3)]
    idx = np.meshgrid(*[np.arange(s) for s in shape], indexing="ij")
    cell = [idx[i] // d[i] for i in range(3)]
    fr = [((idx[i] - cell[i] * d[i]).astype(dt) / dt(d[i])).astype(dt) for i in range(3)]

    def corner(o):
        gv = g[cell[0] + o[0], cell[1] + o[1], cell[2] + o[2]]
        return (fr[0] - dt(o[0])) * gv[..., 0] + (fr[1] - dt(o[1])) * gv[..., 1] + (fr[2] - dt(o[2])) * gv[..., 2]

    t = [f * f * f * (f * (f * dt(6) - dt(15)) + dt(10)) for f in fr]
    one = dt(1)
    n00 = corner((0, 0, 0)) * (one - t[0]) + t[0] * corner((1, 0, 0))
    n10 = corner((0, 1, 0)) * (one - t[0]) + t[0] * corner((1, 1, 0))
    n01 = corner((0, 0, 1)) * (one - t[0]) + t[0] * corner((1, 0, 1))
    n11 = corner((0, 1, 1)) * (one - t[0]) + t[0] * corner((1, 1, 1))
    m0 = (one - t[1]) * n00 + t[1] * n10
    m1 = (one - t[1]) * n01 + t[1] * n11
    return ((one - t[2]) * m0 + t[2] * m1) * dt(2) - one


@pytest.mark.parametrize("case", PERLIN_CASES, ids=lambda c: "-".join(map(str, c)))
def test_perlin3d_vs_oracle(gpu, case):
    shape, res = case[:3], case[3:]
    theta, phi = _perlin_inputs(case)
    want = so.perlin_noise(shape, res, theta, phi)
    grad = _perlin_grad(theta, phi).astype(F32)
    got = _run(gpu, "maua_perlin3d_f32", [("grad", grad), ("out", Out(shape))] + [(f"a{i}", v) for i, v in enumerate(case)])["out"]
    err = _rel_peak(got, want)
    print(f"perlin3d {case}: err/peak {err:.3e}")
    assert err <= TOL["perlin3d"]


def test_perlin3d_refusals(gpu):
    case = (12, 8, 20, 3, 2, 5)
    grad = _perlin_grad(*_perlin_inputs(case)).astype(F32)
    names = ["n0", "n1", "n2", "r0", "r1", "r2"]
    spec = [("grad", grad), ("out", Out(case[:3]))] + list(zip(names, case))
    _refused(gpu, "maua_perlin3d_f32", spec,
             [({"r0": 5}, EINVAL), ({"r1": 3}, EINVAL), ({"r2": 3}, EINVAL), ({"r0": 24}, EINVAL)] + [({k: 0}, EINVAL) for k in names] +
             [({"n0": -12}, EINVAL), ({"grad": None}, EINVAL), ({"out": None}, EINVAL)])


# ---------------------------------------------------------------------------------------------------------- affine warp
def _warp_emul(x, maps, pads, noise, dt):
    """so.affine_reflect_warp for one pad, every operand and intermediate in ``dt``."""
    pl, pr, pt, pb = pads
    b, c, h, w = x.shape
    canvas = np.pad(x.astype(dt), ((0, 0), (0, 0), (pt, pb), (pl, pr)), mode="reflect")
    if noise is not None:
        canvas = canvas + noise.astype(dt).reshape(1, 1, h + pt + pb, w + pl + pr)
    ch, cw = canvas.shape[-2:]
    oy, ox = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    cy, cx = (oy + (ch - h) // 2).astype(dt), (ox + (cw - w) // 2).astype(dt)
    out = np.zeros(x.shape, dt)
    for i in range(b):
        a = maps[i].astype(dt)
        sx, sy = a[0] * cx + a[1] * cy + a[2], a[3] * cx + a[4] * cy + a[5]
        x0, y0 = np.floor(sx), np.floor(sy)
        fx, fy = sx - x0, sy - y0
        x0, y0 = x0.astype(np.int64), y0.astype(np.int64)
        for dy in (0, 1):
            for dx in (0, 1):
                yy, xx = y0 + dy, x0 + dx
                ok = (yy >= 0) & (yy < ch) & (xx >= 0) & (xx < cw)
                wgt = ((fy if dy else dt(1) - fy) * (fx if dx else dt(1) - fx) * ok).astype(dt)
                out[i] += wgt[None] * canvas[i][:, np.clip(yy, 0, ch - 1), np.clip(xx, 0, cw - 1)]
    return out


# (batch, channels, h, w, (pad_l, pad_r, pad_t, pad_b), add_noise)
WARP_CASES = [(1, 1, 1, 1, (0, 0, 0, 0), False), (4, 3, 1, 1, (2, 3, 1, 4), True), (1, 3, 9, 13, (0, 0, 0, 0), False),
              (4, 1, 9, 13, (3, 2, 5, 1), True), (1, 1, 3, 4, (11, 7, 8, 9), False), (4, 3, 16, 16, (16, 16, 16, 16), True),
              (1, 3, 17, 33, (40, 35, 20, 19), True), (4, 3, 64, 48, (5, 5, 7, 7), False)]


def _warp_inputs(case):
    b, c, h, w, pads, noisy = case
    r = _rng(16, b, c, h, w, *pads)
    x = r.standard_normal((b, c, h, w)).astype(F32)
    ang, sc = r.uniform(-0.5, 0.5, b), r.uniform(0.7, 1.4, b)
    cw, ch = w + pads[0] + pads[1], h + pads[2] + pads[3]
    maps = np.zeros((b, 6), F32)
    for i in range(b):  # rotation and scale about the canvas centre plus a shift: some taps fall outside the canvas
        co, si = sc[i] * np.cos(ang[i]), sc[i] * np.sin(ang[i])
        tx, ty = r.uniform(-0.3, 0.3) * cw, r.uniform(-0.3, 0.3) * ch
        maps[i] = [co, -si, cw / 2 - co * cw / 2 + si * ch / 2 + tx, si, co, ch / 2 - si * cw / 2 - co * ch / 2 + ty]
    noise = r.standard_normal((ch, cw)).astype(F32) if noisy else None
    return x, maps, noise


def _fold_tables(h, w, pads):
    """Canvas pixel -> source pixel for ONE reflection pad, from numpy's own reflect padding of the index ranges."""
    pl, pr, pt, pb = pads
    return np.pad(np.arange(w), (pl, pr), mode="reflect").astype(np.int32), np.pad(np.arange(h), (pt, pb), mode="reflect").astype(np.int32)


def _gpu_warp(gpu, x, maps, pads, noise, mapped):
    b, c, h, w = x.shape
    spec = [("x", x), ("m", maps), ("y", Out(x.shape)), ("batch", b), ("channels", c), ("h", h), ("w", w), ("pad_l", pads[0]),
            ("pad_r", pads[1]), ("pad_t", pads[2]), ("pad_b", pads[3]), ("add_noise", noise)]
    if mapped:
        xmap, ymap = _fold_tables(h, w, pads)
        spec += [("xmap", xmap), ("ymap", ymap), ("src", None)]
    return _run(gpu, "maua_affine_reflect_warp_mapped_f32" if mapped else "maua_affine_reflect_warp_f32", spec)["y"]


@pytest.mark.parametrize("case", WARP_CASES, ids=lambda c: "-".join(map(str, c[:4])) + "-pad" + "_".join(map(str, c[4])) + ("-noise" if c[5] else ""))
def test_affine_reflect_warp_vs_oracle(gpu, case):
    pads = case[4]
    x, maps, noise = _warp_inputs(case)
    want = so.affine_reflect_warp(x, maps, pads, noise)
    got = _gpu_warp(gpu, x, maps, pads, noise, False)
    err = _rel_peak(got, want)
    print(f"affine_reflect_warp {case}: err/peak {err:.3e}")
    assert err <= TOL["affine_reflect_warp"]
    # the table path agrees with the single fold bit for bit when there is one pad (pads larger than the image included)
    assert np.array_equal(_gpu_warp(gpu, x, maps, pads, noise, True).view(np.int32), got.view(np.int32))


@pytest.mark.parametrize("mapped", [False, True])
@pytest.mark.parametrize("b,c,h,w,pad", [(1, 1, 1, 1, 0), (4, 3, 9, 13, 0), (1, 3, 9, 13, 4), (4, 1, 5, 6, 17)])
def test_affine_warp_identity_and_integer_shifts(gpu, b, c, h, w, pad, mapped):
    pads = (pad, pad, pad, pad)
    x = _rng(17, b, c, h, w, pad).standard_normal((b, c, h, w)).astype(F32)
    ident = np.tile(np.array([1, 0, 0, 0, 1, 0], F32), (b, 1))
    assert np.array_equal(_gpu_warp(gpu, x, ident, pads, None, mapped).view(np.int32), x.view(np.int32))  # identity: the input, bit for bit
    for tx, ty in [(w + 2 * pad + 1, 0), (0, -(h + 2 * pad + 1)), (-(2 * w + 2 * pad + 5), 3 * h + 2 * pad)]:
        far = ident.copy()
        far[:, 2], far[:, 5] = tx, ty
        assert not _gpu_warp(gpu, x, far, pads, None, mapped).any()  # every tap is outside the canvas: zeros
    shift = ident.copy()  # an integer shift inside the canvas reads the reflected source exactly
    shift[:, 2], shift[:, 5] = min(pad, 2), -min(pad, 1)
    want = so.affine_reflect_warp(x, shift, pads).astype(F32)
    assert np.array_equal(_gpu_warp(gpu, x, shift, pads, None, mapped), want)


def test_affine_warp_refusals(gpu):
    case = (2, 3, 5, 6, (1, 2, 3, 4), True)
    x, maps, noise = _warp_inputs(case)
    xmap, ymap = _fold_tables(5, 6, case[4])
    spec = [("x", x), ("m", maps), ("y", Out(x.shape)), ("batch", 2), ("channels", 3), ("h", 5), ("w", 6), ("pad_l", 1), ("pad_r", 2),
            ("pad_t", 3), ("pad_b", 4), ("add_noise", noise)]
    bad = [({k: v}, EINVAL) for k in ("batch", "channels", "h", "w") for v in (0, -1)] + \
        [({k: -1}, EINVAL) for k in ("pad_l", "pad_r", "pad_t", "pad_b")] + \
        [({"channels": 65536}, EINVAL), ({"batch": 65536}, EINVAL)] + [({k: None}, EINVAL) for k in ("x", "m", "y")]
    _refused(gpu, "maua_affine_reflect_warp_f32", spec, bad)
    _refused(gpu, "maua_affine_reflect_warp_mapped_f32", spec + [("xmap", xmap), ("ymap", ymap), ("src", None)], bad)


# ---------------------------------------------------------------------------------------------------------- the tolerance table
def measure():
    """The float32-vs-float64 figure of every floating-point entry over this module's case lists, on the CPU."""
    fig = {k: 0.0 for k in MEASURED}

    def up(k, v):
        fig[k] = max(fig[k], float(v))

    for case in STFT_CASES:
        n_fft, hop, n, nf = case
        y, win = _stft_inputs(case)
        want, lo = so.stft_complex(y, n_fft, hop, window=win, n_frames=nf), _stft_emul(y, win, n_fft, hop, nf, F32)
        up("stft_complex", _rel_peak(lo, want))
        up("stft_power", _rel_peak(_power(lo), so.stft_power(y, n_fft, hop, window=win, n_frames=nf)))
    for case in ISTFT_CASES:
        n_fft, hop, nf, _ = case
        re, im, win, n = _istft_inputs(case)
        want = so.istft(re.astype(F64) + 1j * im.astype(F64), n, n_fft, hop, window=win)
        up("istft", _rel_peak(_istft_emul(re, im, win, n_fft, hop, n, F32), want))
    for n_fft, hop, n in ROUNDTRIP_CASES:
        y = _rng(3, n_fft, hop, n).standard_normal(n).astype(F32)
        up("roundtrip_half" if hop == n_fft // 2 else "roundtrip", _rel_peak(_roundtrip_emul(y, n_fft, hop, F32), y.astype(F64)))
    re, im, xs, xr = _softmask_inputs()
    for power, margin, split in SOFTMASK_CASES:
        want = np.stack(_softmask_want(re, im, xs, xr, margin, power, split))
        up("softmask_apply", _rel_peak(np.stack(_softmask_emul(re, im, xs, xr, margin, power, split, F32)), want))
    for case in FILTERBANK_CASES:
        fb, p = _filterbank_inputs(case)
        up("filterbank", _filterbank_err(_filterbank_emul(fb, p, case[3], F32), _filterbank_emul(fb, p, case[3], F64), case[3]))
    for case in CENS_CASES:
        ch = _cens_input(case)
        assert _cens_unambiguous(ch).all(), case
        up("chroma_cens", np.abs(_cens_emul(ch, case[1], F32) - so.cens_from_chroma(ch, win_len=case[1])).max())
    for case in NN_CASES:
        assert _nn_unambiguous(_nn_input(case), case[2], case[3]), case
    for case in CQT_CASES:
        for j in range(len(CQT_EDGE_LENGTHS) if case[0] == 1 else 1):
            y, freqs, lengths = _cqt_inputs(case, j)
            want = _cqt_ref(y, freqs, lengths, case[2], 1 + case[1] // case[2])[0]
            up("cqt_mag", _rel_peak(want.astype(F32), want))  # fp64 accumulation: the float32 output rounding only
    for case in RESAMPLE_CASES:
        x = _resample_input(case)
        up("resample_f64", _rel_peak(so.resample(x.astype(F32).astype(F64), case[1]).astype(F32), so.resample(x, case[1])))
    for T in FIR_TS:
        for radius in _fir_radii(T):
            for F in FIR_FEATURES:
                x, taps = _fir_inputs(T, radius, F)
                want, scale = _fir_emul(x, taps, radius, F64)
                up("temporal_fir", _fir_err(_fir_emul(x, taps, radius, F32)[0], want, scale))
    for case in PERLIN_CASES:
        theta, phi = _perlin_inputs(case)
        lo = _perlin_emul(_perlin_grad(theta, phi), case[:3], case[3:], F32)
        up("perlin3d", _rel_peak(lo, so.perlin_noise(case[:3], case[3:], theta, phi)))
    for case in WARP_CASES:
        x, maps, noise = _warp_inputs(case)
        up("affine_reflect_warp", _rel_peak(_warp_emul(x, maps, case[4], noise, F32), so.affine_reflect_warp(x, maps, case[4], noise)))
    return fig


if __name__ == "__main__":
    for name, v in measure().items():
        print(f"    {name:<22s} float32 run {v:.2e}   tolerance {4 * v:.2e}   (module constant {MEASURED[name]:.2e})")
