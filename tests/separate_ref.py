"""Reference for the soft masks of the source separation (csrc/separate.hip, maua_nmf_separate_f32): the definition of
include/maua_hip.h restated in float64 numpy, an all-float32 emulation of it in the order the header gives (the fmaf chain of a group,
the square, the sum over the groups, the division, the product; every intermediate rounded to fp32), the comparison helper the GPU test
uses, the shared case list, deliberately wrong variants, and the whole chain of ``ar.separate`` in float64 (STFT, KL-NMF, masks,
inverse STFT) on the clip of tests/test_separate_features_gpu.py.

    PYTHONPATH=. python tests/separate_ref.py

prints, without a GPU, the emulation's worst relative error against float64 over the GPU case list, from which MASK_TOL is derived
(4 x the figure, rounded up to two digits; never taken from the kernel), and the float64 chain's SDR figures.

The worst-case bound of one output element (the ceiling).  u = 2^-24 is the unit round-off of fp32.  The cases hold positive W and H,
so every sum below has positive terms and a relative error of the terms bounds that of the sum.
  P_g: at most K fused multiply-adds, one rounding each:                          K u
  q_g: power 1 nothing more; power 2 doubles the error and rounds once:           p K u + (p - 1) u        (p = power)
  D:   the terms carry that; G additions from 0, the first exact:                 + (G - 1) u
  m_g = q_g / D: both errors and one rounding:                                    2 (p K + p - 1) u + (G - 1) u + u
  out = m_g * re: one rounding:                                                   + u
      (2 p K + 2 p + G - 1) u,   asserted as   CEILING = (2 p K + 2 p + G + 7) u
  (the 8 u of slack cover the second-order terms: the first-order figure stays below 170 u for K, G <= 32, and (170 u)^2 << u).
Partition of unity (the GPU test): sum_g out[g] against re.  sum_g m_g = (sum_g q_g (1 + d_g)) / D with |d_g| <= u for the division and
D = (sum_g q_g) (1 + e), |e| <= (G - 1) u; every product m_g re rounds once more: |sum_g out[g] - re| <= (G + 1) u |re| to first
order, asserted as (G + 2) u |re| with the sum taken in float64.  Where D == 0 the masks are 1 / G rounded to fp32, G of them: the
same bound covers G |fl(1 / G) - 1 / G| <= G u / G."""
import numpy as np

import nmf_ref as nr

U = 2.0 ** -24

# Measured by `python tests/separate_ref.py`: the fp32 emulation against float64 over gpu_cases(), worst relative error of any element.
MASK_TOL = 1.7e-6  # 4 x 4.25e-7 (worst case F=1025 T=1 K=32 G=32 power 2; ceiling there 1.02e-5), rounded up to two digits


# ------------------------------------------------------------------------------------------------ the definition
def _fma32(a, b, c):
    """fl32(a * b + c) of float32 arrays: the product of two fp32 numbers is exact in float64 (48 bits); the float64 addition rounds at
    2^-53 before the rounding to fp32, a double rounding that moves a result only when the float64 sum lands within 2^-29 (relative)
    of a tie of fp32."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


def group_models(W, H, group, G, dtype=np.float64, power_per_component=0):
    """q [G, F, T] before the power (``power_per_component`` = 0): P_g = sum over k ascending with group[k] == g of W[f,k] H[k,t],
    chained from 0.  float32: every step a fused multiply-add.  ``power_per_component`` = p (a deliberate defect): sum_k (W H)^p."""
    W, H = np.asarray(W, dtype), np.asarray(H, dtype)
    P = np.zeros((G, W.shape[0], H.shape[1]), dtype)
    for k in range(W.shape[1]):
        g = int(group[k])
        w, h = W[:, k:k + 1], H[k:k + 1, :]
        if power_per_component:
            P[g] = P[g] + (w * h) ** power_per_component
        elif dtype == np.float32:
            P[g] = _fma32(np.broadcast_to(w, P[g].shape), np.broadcast_to(h, P[g].shape), P[g])
        else:
            P[g] = P[g] + w * h
    return P


def masks(W, H, group, G, power, dtype=np.float64, window=None, power_per_component=False):
    """m [G, F, T] in ``dtype``: q_g = P_g ** power, D = q_0 + q_1 + ... from 0 in that order, m_g = q_g / D where D > 0, else 1 / G.
    ``window`` = (g0, n_out): D summed over the window only (a deliberate defect)."""
    P = group_models(W, H, group, G, dtype, power if power_per_component else 0)
    q = P if power == 1 or power_per_component else (P * P).astype(dtype)
    lo, hi = (0, G) if window is None else (window[0], window[0] + window[1])
    D = np.zeros(q.shape[1:], dtype)
    for g in range(lo, hi):
        D = (D + q[g]).astype(dtype)
    with np.errstate(all="ignore"):
        m = np.where(D > 0, q / np.where(D > 0, D, dtype(1))[None], dtype(1) / dtype(G))
    return m.astype(dtype)


def separate(re, im, W, H, group, G, power, dtype=np.float64, **defect):
    """(out_re, out_im) [G, F, T] in ``dtype``: m_g * re, m_g * im."""
    m = masks(W, H, group, G, power, dtype, **defect)
    return (m * np.asarray(re, dtype)[None]).astype(dtype), (m * np.asarray(im, dtype)[None]).astype(dtype)


def ceiling(K, G, power):
    return (2 * power * K + 2 * power + G + 7) * U


def tolerance(case):
    """What the GPU test allows against float64: MASK_TOL, and never more than the case's own ceiling (K = G = 1 lies below it)."""
    return min(MASK_TOL, ceiling(case["K"], case["G"], case["power"]))


def compare(got, ref, tol=MASK_TOL, what="out"):
    """List of complaints (empty = the pair ``got`` agrees with the float64 pair ``ref``): every element of out_re and out_im within
    ``tol`` relative, none exempt; where the reference is exactly 0 the value must be exactly 0."""
    return nr.compare(got[0], ref[0], tol, f"{what}_re") + nr.compare(got[1], ref[1], tol, f"{what}_im")


def pair_error(got, ref):
    return max(nr.rel_error(got[0], ref[0]), nr.rel_error(got[1], ref[1]))


# ------------------------------------------------------------------------------------------------ the GPU case list
FS = (1, 7, 1025)
TS = (1, 63, 64, 65, 1000)
KS = (1, 3, 4, 5, 8, 9, 16, 17, 32)
# (F, T, K, G, layout) paired, not crossed: every value of every axis at least once, the extremes together; the tile edges of the kernel
# meet their neighbours (64 columns and 64 rows a workgroup, four waves striding over the rows, the K tiles 4 / 8 / 16 / 32 and the
# first K behind each); G in {1, 2, K}.  Layouts: "each" group[k] = k; "one" all 0; "runs" numpy.array_split; "interleaved"
# group[k] = k % G; "gaps" group[k] = 2 (k // 2) (every odd group empty); "second" all components in group 1 (group 0 empty).
SHAPES = ((1025, 1, 32, 32, "each"), (1, 1000, 1, 1, "one"), (1025, 64, 3, 2, "runs"), (7, 64, 4, 2, "interleaved"), (7, 65, 5, 5, "each"),
          (1025, 65, 8, 2, "runs"), (7, 1000, 9, 2, "interleaved"), (7, 63, 16, 16, "each"), (7, 63, 17, 17, "gaps"), (7, 65, 32, 2, "runs"),
          (7, 1, 8, 1, "one"), (1, 64, 16, 2, "second"))


def layout(name, K, G):
    if name == "each":
        return np.arange(K, dtype=np.int32)
    if name == "one":
        return np.zeros(K, np.int32)
    if name == "runs":
        return split_runs(K, G)
    if name == "interleaved":
        return (np.arange(K) % G).astype(np.int32)
    if name == "gaps":
        return (2 * (np.arange(K) // 2)).astype(np.int32)
    if name == "second":
        return np.ones(K, np.int32)
    raise KeyError(name)


def split_runs(K, G):
    """group[k] of ``groups=G``: the K ordered components in G contiguous runs sized as numpy.array_split."""
    group = np.empty(K, np.int32)
    for g, run in enumerate(np.array_split(np.arange(K), G)):
        group[run] = g
    return group


def gpu_cases():
    cases = [{"F": f, "T": t, "K": k, "G": g, "layout": name, "power": power, "seed": 700 + i}
             for i, (f, t, k, g, name) in enumerate(SHAPES) for power in (1, 2)]
    assert {c["F"] for c in cases} == set(FS) and {c["T"] for c in cases} == set(TS) and {c["K"] for c in cases} == set(KS)
    assert all(c["G"] in (1, 2, c["K"]) for c in cases)
    return cases


def case_id(case):
    return "F{F}-T{T}-K{K}-G{G}-{layout}-p{power}".format(**case)


def make_case(case):
    """(re, im, W, H, group) — re, im standard normal, W and H uniform in [0.5, 1.5) (every P_g of a non-empty group is far above 0),
    all float32; group int32."""
    rng = np.random.default_rng(case["seed"])
    F, T, K = case["F"], case["T"], case["K"]
    re = rng.standard_normal((F, T)).astype(np.float32)
    im = rng.standard_normal((F, T)).astype(np.float32)
    W = (0.5 + rng.random((F, K))).astype(np.float32)
    H = (0.5 + rng.random((K, T))).astype(np.float32)
    return re, im, W, H, layout(case["layout"], K, case["G"])


_RESULTS = {}


def result(case, dtype=np.float64, **defect):
    """(out_re, out_im) of a case in ``dtype``; computed once and shared (callers must not write to it)."""
    key = (case_id(case), np.dtype(dtype).name, tuple(sorted((k, str(v)) for k, v in defect.items())))
    if key not in _RESULTS:
        re, im, W, H, group = make_case(case)
        if defect.pop("swap_groups", False):
            group = (case["G"] - 1 - group).astype(np.int32)
        _RESULTS[key] = separate(re, im, W, H, group, case["G"], case["power"], dtype, **defect)
    return _RESULTS[key]


# ------------------------------------------------------------------------------------------------ the whole chain in float64
SR, N_FFT, HOP = 22050, 2048, 512
CLIP_SECONDS = 4.0
SDR_FLOOR = 25.0  # dB, what the device must reach (float64 below: 38 and 32 dB; 7 dB are left for fp32)


def two_tone_clip():
    """(x, a, b) float64 [88200]: a = 0.5 sin(2 pi 220 t) on for the first half of every 1.0 s, b = 0.3 sin(2 pi 1760 t) on for the first
    40 % of every 0.6 s starting 0.2 s early, both gates smoothed with a unit-sum 441-tap Hann; x = a + b."""
    t = np.arange(int(SR * CLIP_SECONDS)) / SR
    taps = np.hanning(441)
    taps /= taps.sum()
    gate_a = np.convolve(((t % 1.0) < 0.5).astype(np.float64), taps, mode="same")
    gate_b = np.convolve((((t + 0.2) % 0.6) < 0.24).astype(np.float64), taps, mode="same")
    a = 0.5 * gate_a * np.sin(2 * np.pi * 220 * t)
    b = 0.3 * gate_b * np.sin(2 * np.pi * 1760 * t)
    return a + b, a, b


def hann():
    return 0.5 - 0.5 * np.cos(2 * np.pi * np.arange(N_FFT) / N_FFT)


def stft(x):
    """Complex STFT [1025, 1 + len // 512] in float64: centred, reflect-padded, periodic Hann."""
    x = np.asarray(x, np.float64)
    padded = np.pad(x, N_FFT // 2, mode="reflect")
    n_frames = 1 + len(x) // HOP
    frames = np.stack([padded[i * HOP: i * HOP + N_FFT] for i in range(n_frames)])
    return np.fft.rfft(frames * hann()[None, :], axis=1).T


def istft(D, n):
    """Window-sum-square normalised overlap-add of the inverse transforms, centre padding removed, length n."""
    win = hann()
    frames = np.fft.irfft(D.T, n=N_FFT, axis=1) * win[None, :]
    total = np.zeros(N_FFT + HOP * (D.shape[1] - 1))
    wss = np.zeros_like(total)
    for i in range(D.shape[1]):
        total[i * HOP: i * HOP + N_FFT] += frames[i]
        wss[i * HOP: i * HOP + N_FFT] += win * win
    total = np.where(wss > 1.17549435e-38, total / np.where(wss > 1.17549435e-38, wss, 1.0), total)
    return total[N_FFT // 2: N_FFT // 2 + n]


def sdr(estimate, target):
    estimate, target = np.asarray(estimate, np.float64), np.asarray(target, np.float64)
    return float(10 * np.log10((target ** 2).sum() / ((estimate - target) ** 2).sum()))


_MODELS = {}


def chain_model(x, n_components, seed, n_iter=200):
    """(D complex [F, T], W, H) of the float64 chain up to the factorisation: the seeded start of ``ar.nmf``, ``n_iter`` iterations,
    unit-sum templates ordered by centroid.  Computed once per (n_components, seed)."""
    key = (n_components, seed, n_iter, len(x))
    if key not in _MODELS:
        D = stft(x)
        V = np.abs(D)
        W, H = nr.iterate(V, *nr.seeded_start(V, n_components, seed), n_iter)
        _MODELS[key] = (D, *nr.normalise_and_order(W, H))
    return _MODELS[key]


def chain(x, n_components, groups, power, seed, n_iter=200):
    """stems [G, len(x)] of the whole chain in float64."""
    D, W, H = chain_model(x, n_components, seed, n_iter)
    group = np.arange(n_components) if groups is None else split_runs(n_components, groups)
    G = int(group.max()) + 1
    m = masks(W, H, group, G, power)
    return np.stack([istft(m[g] * D, len(x)) for g in range(G)])


if __name__ == "__main__":
    worst = (0.0, None)
    for case in gpu_cases():
        e = pair_error(result(case, np.float32), result(case))
        print(f"{case_id(case):>36}: emulation {e:.3g} (ceiling {ceiling(case['K'], case['G'], case['power']):.3g})")
        if e > worst[0]:
            worst = (e, case_id(case))
    print("worst:", worst, "-> MASK_TOL", 4 * worst[0])
    x, a, b = two_tone_clip()
    print(f"round trip istft(stft(x)) - x: {np.abs(istft(stft(x), len(x)) - x).max():.3g}")
    for K, groups in ((2, None), (4, 2)):
        for seed in (0, 1, 2):
            for power in (1, 2):
                stems = chain(x, K, groups, power, seed)
                print(f"K {K} groups {groups} seed {seed} power {power}: SDR {sdr(stems[0], a):.2f} / {sdr(stems[1], b):.2f} dB, "
                      f"sum - round trip {np.abs(stems.sum(0) - istft(stft(x), len(x))).max():.3g}")
