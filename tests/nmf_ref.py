"""Reference for the spectrogram factorisation (csrc/nmf.hip, maua_nmf_kl_f32 / maua_nmf_kl_div_f32): the definition of
include/maua_hip.h restated in float64 numpy, an all-float32 emulation of it (every operand and intermediate rounded to fp32, every sum
accumulated sequentially in index order, no fused multiply-add), the comparison helper the GPU test uses, the shared case list, the
planted case and the host side of ``ar.nmf`` (start, normalisation, ordering).

    PYTHONPATH=. python tests/nmf_ref.py

prints, without a GPU, the emulation's worst relative error against float64 over the GPU case list and the planted case's figures,
from which the constants below are derived (4 x the figure, rounded up to two digits; never taken from the kernel).

The worst-case bound of one step (the ceiling).  u = 2^-24 is the unit round-off of fp32; every quantity below is positive, every sum has
non-negative terms, so a relative error of the terms bounds the relative error of the sum whatever the summation order, and a sum of n
terms adds at most (n - 1) u for its own roundings (to first order in u).
  H step from an exact fp32 state.  P = sum_k W H: K products and K - 1 additions (K roundings when fused), relative error <= K u.  The
  clamp max(P, eps) is exact.  R = V / P: K u + u.  A term W R: + u.  The numerator sum over f: + (F - 1) u, so (K + F + 1) u.  The
  denominator sum_f W: (F - 1) u.  H * numerator: + u; the quotient: + u, and the denominator's error adds:
      (K + F + 1) + (F - 1) + 2 = (2 F + K + 2) u,   asserted as   H_CEILING = (2 F + K + 16) u
  (the 14 u of slack cover the second-order terms: (2 F + K)^2 u^2 < u for every shape of the list).
  W step from an exact fp32 state, by the same count with T for F:  (2 T + K + 16) u.
  W step after an H step (one full iteration), against float64 carried through both steps: the W step's own (2 T + K + 16) u plus the
  error e_H the new H arrives with,   W_CEILING = (2 T + 2 F + 2 K + 32) u.   (That counts e_H once.  A strict first-order worst case
  would count it three times — P, the product R H and the denominator each carry it — but the errors of a column of H are those of
  sums of positive terms rounded independently; the tighter figure is the one asserted, and the emulation sits two orders of
  magnitude below it.)
The divergence.  A term V log(V / P) - V + P has derivative 1 - V / P in P; P carries K u, so a term moves by at most K u |P - V|
<= K u (V + P); its evaluation and the sum in double add nothing visible; the conversion of V and P is exact.  Asserted per column:
(K + 2) u sum_f (V + P), absolute."""
import math

import numpy as np

U = 2.0 ** -24
EPS = 1e-12

# Measured by `python tests/nmf_ref.py`: the fp32 emulation against float64 over gpu_cases(), worst relative error of any element.
# Tolerance = 4 x the figure, rounded up to two digits.
H_STEP_TOL = 7.2e-6      # 4 x 1.79e-6   H after an H step, alone or in an iteration (worst case F=1025 T=257 K=16; ceiling there 1.24e-4)
W_ONLY_TOL = 7.7e-6      # 4 x 1.93e-6   W after a W-only step                       (worst case F=257 T=1000 K=17; ceiling 1.21e-4)
W_AFTER_H_TOL = 1.1e-5   # 4 x 2.60e-6   W after the H step of an iteration          (worst case F=257 T=1000 K=17; ceiling 1.54e-4)
# The planted case, 200 iterations: final divergence of the emulation against float64's, relative excess (D32 - D64) / D64.
PLANTED_EXCESS = 7.8e-9  # measured: D64 = 0.281846661, the emulation ends 7.79e-9 (relative) above it
PLANTED_MARGIN = max(4 * PLANTED_EXCESS, 1e-6)  # the floor decides
PLANTED_COSINE = 0.999   # every true template against its best recovered one (float64 and the emulation give >= 0.999996)


# ------------------------------------------------------------------------------------------------ the definition
def _seq_sum(terms, axis, dtype):
    """Sum along ``axis`` accumulated in index order in ``dtype`` (numpy's cumsum is sequential; its sum is pairwise)."""
    if dtype == np.float64:
        return terms.sum(axis=axis)
    return np.take(np.cumsum(terms, axis=axis, dtype=dtype), -1, axis=axis)


def product(W, H, eps, dtype=np.float64, skip_component=None):
    """P = max(W . H, eps) [F, T]: k ascending from 0, every product and partial sum rounded to ``dtype``."""
    W, H = np.asarray(W, dtype), np.asarray(H, dtype)
    p = np.zeros((W.shape[0], H.shape[1]), dtype)
    for k in range(W.shape[1]):
        if k != skip_component:
            p = p + W[:, k:k + 1] * H[k:k + 1, :]
    return np.maximum(p, dtype(eps))


def h_step(V, W, H, eps=EPS, dtype=np.float64, drop_last_row=False, skip_component=None):
    """H * (sum_f W R) / max(sum_f W, eps).  The two switches build deliberately wrong variants (tests/test_nmf_host.py)."""
    V, W, H = np.asarray(V, dtype), np.asarray(W, dtype), np.asarray(H, dtype)
    with np.errstate(all="ignore"):
        R = V / product(W, H, eps, dtype, skip_component)
        rows = slice(0, W.shape[0] - 1) if drop_last_row else slice(None)
        num = _seq_sum(W[rows, :, None] * R[rows, None, :], 0, dtype)          # [K, T]
        den = np.maximum(_seq_sum(W, 0, dtype), dtype(eps))                    # [K]
        return ((H * num) / den[:, None]).astype(dtype)


def w_step(V, W, H, eps=EPS, dtype=np.float64, skip_component=None):
    """W * (sum_t R H) / max(sum_t H, eps)."""
    V, W, H = np.asarray(V, dtype), np.asarray(W, dtype), np.asarray(H, dtype)
    with np.errstate(all="ignore"):
        R = V / product(W, H, eps, dtype, skip_component)
        num = _seq_sum(R[:, None, :] * H[None, :, :], 2, dtype)                # [F, K]
        den = np.maximum(_seq_sum(H, 1, dtype), dtype(eps))                    # [K]
        return ((W * num) / den[None, :]).astype(dtype)


def iterate(V, W, H, n_iter=1, update_w=True, update_h=True, eps=EPS, dtype=np.float64, stale_h=False, **defect):
    """n_iter iterations (H step, then W step with the new H) -> (W, H) in ``dtype``.  ``stale_h``: the W step uses the H from before the
    H step (a deliberate defect)."""
    W, H = np.asarray(W, dtype), np.asarray(H, dtype)
    for _ in range(n_iter):
        old = H
        if update_h:
            H = h_step(V, W, H, eps, dtype, **defect)
        if update_w:
            W = w_step(V, W, old if stale_h else H, eps, dtype, skip_component=defect.get("skip_component"))
    return W, H


def divergence_cols(V, W, H, eps=EPS, p_dtype=np.float64):
    """d_cols [T] in float64: sum_f (V log(V / P) - V + P), 0 log 0 = 0, P = max(W . H, eps) computed in ``p_dtype``."""
    V = np.asarray(V, np.float64)
    P = product(W, H, eps, p_dtype).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        log_term = np.where(V > 0, V * np.log(np.where(V > 0, V, 1.0) / P), 0.0)
    return (log_term - V + P).sum(axis=0)


def divergence(V, W, H, eps=EPS, p_dtype=np.float64):
    return float(divergence_cols(V, W, H, eps, p_dtype).sum())


def divergence_tolerance(V, W, H, eps=EPS):
    """Per column, absolute: (K + 2) u sum_f (V + P)."""
    P = product(W, H, eps)
    return (np.asarray(W).shape[1] + 2) * U * (np.asarray(V, np.float64) + P).sum(axis=0)


def h_ceiling(F, T, K):
    return (2 * F + K + 16) * U


def w_only_ceiling(F, T, K):
    return (2 * T + K + 16) * U


def w_ceiling(F, T, K):
    return (2 * T + 2 * F + 2 * K + 32) * U


# ------------------------------------------------------------------------------------------------ comparison
def rel_error(got, ref):
    """Worst relative error of any element (inf where the reference is 0 and the value is not, or a value is not finite)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        e = np.where(ref == 0, np.where(got == 0, 0.0, np.inf), np.abs(got - ref) / np.abs(ref))
    e = np.where(np.isfinite(got), e, np.inf)
    return float(e.max()) if e.size else 0.0


def compare(got, ref, tol, what):
    """List of complaints (empty = ``got`` agrees with the float64 ``ref``): every element within ``tol`` relative, none exempt; where
    the reference is exactly 0 the value must be exactly 0."""
    got = np.asarray(got)
    if got.shape != np.shape(ref):
        return [f"{what}: shape {got.shape} != {np.shape(ref)}"]
    e = rel_error(got, ref)
    return [] if e <= tol else [f"{what}: worst relative error {e:.3g} > {tol:.3g}"]


# ------------------------------------------------------------------------------------------------ the GPU case list
FS = (1, 2, 63, 64, 65, 257, 1025)
TS = (1, 2, 63, 64, 65, 255, 256, 257, 1000)
KS = (1, 2, 3, 4, 5, 8, 15, 16, 17, 31, 32)
# paired, not crossed: every value of every axis at least once, the extremes together; the tile edges of the kernels meet their
# neighbours (64 columns per workgroup of the H step, 256 lanes striding over t and 2 | 1 rows per workgroup in the W step, four
# quarters of the f range, the K tiles 4 / 8 / 16 / 32 and the first K behind each)
SHAPES = ((1025, 1, 32), (1, 1000, 1), (2, 2, 2), (63, 63, 3), (64, 64, 4), (65, 65, 5), (257, 255, 8), (64, 256, 15), (65, 257, 16),
          (257, 1000, 17), (63, 64, 31), (1025, 257, 16))
CHAINED = ((65, 257, 16), (257, 255, 8), (63, 64, 31))  # the three cases of the chained check


def gpu_cases():
    cases = [{"F": f, "T": t, "K": k, "seed": 500 + i} for i, (f, t, k) in enumerate(SHAPES)]
    assert {c["F"] for c in cases} == set(FS) and {c["T"] for c in cases} == set(TS) and {c["K"] for c in cases} == set(KS)
    return cases


def case_id(case):
    return "F{F}-T{T}-K{K}".format(**case)


def make_case(case):
    """(V, W, H) in float32: strictly positive gamma-distributed V, W and H uniform in [0.5, 1.5) — W.H is far above eps, the clamp is
    never the deciding branch."""
    rng = np.random.default_rng(case["seed"])
    F, T, K = case["F"], case["T"], case["K"]
    V = np.maximum(rng.gamma(2.0, 1.0, (F, T)), 1e-3).astype(np.float32)
    W = (0.5 + rng.random((F, K))).astype(np.float32)
    H = (0.5 + rng.random((K, T))).astype(np.float32)
    return V, W, H


_STEPS = {}


def steps(case, dtype=np.float64, **defect):
    """The three single steps of a case from the same start, in ``dtype``: dict(h_only = H, w_only = W, full = (W, H)).  The float64
    result is computed once and shared (callers must not write to it)."""
    key = (case_id(case), np.dtype(dtype).name, tuple(sorted(defect.items())))
    if key not in _STEPS:
        V, W, H = make_case(case)
        stale = defect.pop("stale_h", False) if defect else False
        _STEPS[key] = {"h_only": h_step(V, W, H, EPS, dtype, **defect),
                       "w_only": w_step(V, W, H, EPS, dtype, skip_component=defect.get("skip_component")),
                       "full": iterate(V, W, H, 1, True, True, EPS, dtype, stale_h=stale, **defect)}
    return _STEPS[key]


def compare_steps(got, ref, h_tol=H_STEP_TOL, w_only_tol=W_ONLY_TOL, w_tol=W_AFTER_H_TOL):
    """The comparison of the GPU test: the three steps of ``got`` against the float64 ``ref`` (both as steps() returns them)."""
    return (compare(got["h_only"], ref["h_only"], h_tol, "H of the H-only step") + compare(got["w_only"], ref["w_only"], w_only_tol, "W of the W-only step")
            + compare(got["full"][1], ref["full"][1], h_tol, "H of the full iteration") + compare(got["full"][0], ref["full"][0], w_tol, "W of the full iteration"))


# ------------------------------------------------------------------------------------------------ the planted case
PLANTED_F, PLANTED_T, PLANTED_K, PLANTED_ITERS, PLANTED_SEED = 96, 400, 3, 200, 0
PLANTED_PERIODS, PLANTED_DECAY = (37, 53, 71), 4.0


def planted():
    """(V float32 [96, 400], W* [96, 3], H* [3, 400]): template k is a Hann bump plus 0.05 on the k-th third of the bins and 0 on the
    others (disjoint supports: the factorisation is unique up to scale and order), the activations are bursts exp(-phase / 4) at three
    periods, V = W* . H* + 1e-4."""
    third = PLANTED_F // 3
    Wt = np.zeros((PLANTED_F, PLANTED_K))
    for k in range(PLANTED_K):
        Wt[k * third:(k + 1) * third, k] = 0.55 - 0.5 * np.cos(2 * np.pi * (np.arange(third) + 0.5) / third)
    t = np.arange(PLANTED_T, dtype=np.float64)
    Ht = np.stack([np.exp(-((t + 5 * k) % p) / PLANTED_DECAY) for k, p in enumerate(PLANTED_PERIODS)])
    return (Wt @ Ht + 1e-4).astype(np.float32), Wt, Ht


def seeded_start(V, n_components, seed):
    """The start of ``ar.nmf``: numpy.random.default_rng(seed), W [F, K] then H [K, T] uniform in [0, 1), both scaled by
    sqrt(mean(V) / K), rounded to float32."""
    V = np.asarray(V)
    rng = np.random.default_rng(seed)
    scale = math.sqrt(float(V.mean(dtype=np.float64)) / n_components)
    W = (rng.random((V.shape[0], n_components)) * scale).astype(np.float32)
    H = (rng.random((n_components, V.shape[1])) * scale).astype(np.float32)
    return W, H


def divergence_trace(V, W, H, n_iter, dtype, eps=EPS):
    """Divergence (float64 arithmetic on the state as it stands) before the first and after every iteration, and the final state."""
    W, H = np.asarray(W, dtype), np.asarray(H, dtype)
    trace = [divergence(V, W, H, eps)]
    for _ in range(n_iter):
        W, H = iterate(V, W, H, 1, True, True, eps, dtype)
        trace.append(divergence(V, W, H, eps))
    return np.array(trace), W, H


_PLANTED = {}


def planted_reference():
    """dict(trace [201], W, H) of the float64 loop on the planted case from the seeded start; computed once."""
    if not _PLANTED:
        V, _, _ = planted()
        trace, W, H = divergence_trace(V, *seeded_start(V, PLANTED_K, PLANTED_SEED), PLANTED_ITERS, np.float64)
        _PLANTED.update(trace=trace, W=W, H=H)
    return _PLANTED


def template_cosines(W, W_true):
    """For every true template, the best cosine similarity with any column of ``W``."""
    a = np.asarray(W, np.float64)
    b = np.asarray(W_true, np.float64)
    a = a / np.maximum(np.linalg.norm(a, axis=0, keepdims=True), 1e-300)
    b = b / np.linalg.norm(b, axis=0, keepdims=True)
    return (b.T @ a).max(axis=1)


# ------------------------------------------------------------------------------------------------ host side of ar.nmf
def centroids(W):
    W = np.asarray(W, np.float64)
    return (np.arange(W.shape[0])[:, None] * W).sum(axis=0) / np.maximum(W.sum(axis=0), 1e-300)


def normalise_and_order(W, H):
    """Templates to unit sum (activations scaled the other way), then ascending spectral centroid, ties by index."""
    W, H = np.asarray(W, np.float64), np.asarray(H, np.float64)
    s = W.sum(axis=0)
    s = np.where(s > 0, s, 1.0)
    W, H = W / s[None, :], H * s[:, None]
    order = np.argsort(centroids(W), kind="stable")
    return W[:, order], H[order]


if __name__ == "__main__":
    worst = {"h_only": (0.0, None), "w_only": (0.0, None), "full_h": (0.0, None), "full_w": (0.0, None)}
    for case in gpu_cases():
        ref, emu = steps(case), steps(case, np.float32)
        F, T, K = case["F"], case["T"], case["K"]
        e = {"h_only": rel_error(emu["h_only"], ref["h_only"]), "w_only": rel_error(emu["w_only"], ref["w_only"]),
             "full_h": rel_error(emu["full"][1], ref["full"][1]), "full_w": rel_error(emu["full"][0], ref["full"][0])}
        print(f"{case_id(case):>18}: H-only {e['h_only']:.3g} (ceiling {h_ceiling(F, T, K):.3g})  W-only {e['w_only']:.3g} ({w_only_ceiling(F, T, K):.3g})"
              f"  full: H {e['full_h']:.3g}  W {e['full_w']:.3g} ({w_ceiling(F, T, K):.3g})")
        for key, val in e.items():
            if val > worst[key][0]:
                worst[key] = (val, case_id(case))
    print("worst:", worst)
    V, Wt, Ht = planted()
    ref = planted_reference()
    t32, W32, H32 = divergence_trace(V, *seeded_start(V, PLANTED_K, PLANTED_SEED), PLANTED_ITERS, np.float32)
    d64, d32 = ref["trace"], t32
    print(f"planted: D64 {d64[0]:.6g} -> {d64[-1]:.9g}, largest rise {np.diff(d64).max():.3g}, smallest decrease {(-np.diff(d64)).min():.3g}")
    print(f"         D32 -> {d32[-1]:.9g}, largest rise {np.diff(d32).max():.3g}; relative excess {(d32[-1] - d64[-1]) / d64[-1]:.3g}")
    print(f"         cosines float64 {template_cosines(ref['W'], Wt)}, fp32 {template_cosines(W32, Wt)}")
