#!/usr/bin/env python3
"""Timing of the spectrogram factorisation on the MI355X (the figures of profiles/nmf.md):

    python tools/bench_nmf.py [--frames 10336] [--iters 200] [--rounds 3] [--out nmf_bench.json]

For the shapes of a 240 s clip (T = 10336 frames) with F = 128 (mel) and F = 1025 (STFT) bins at K = 8 and K = 16, on seeded
gamma-distributed V, in one warm process:
  * maua_nmf_kl_f32 with update_w = 0 (the H-step kernel alone), with update_h = 0 (the W-step kernel alone) and with both, and
  * the same updates written as torch ops on the same device (two matrix products, a clamp and a division per step, W.H and V / (W.H)
    materialised),
each timed by device events around one window of ``--iters`` iterations after a warm-up window, the variants alternating over
``--rounds`` rounds (minimum and median reported, per iteration).  Also the bytes of V read per iteration (2 F T 4) against the time of
the full iteration, and the largest relative difference between the two formulations after 10 iterations from the same start.
Nothing here asserts a speed.  Needs a GPU: there is no fallback."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from maua_stylegan2_amd import _lib  # noqa: E402

EPS = 1e-12
SHAPES = ((128, 8), (128, 16), (1025, 8), (1025, 16))


def torch_iteration(V, W, H):
    R = V / (W @ H).clamp_min(EPS)
    H = H * (W.t() @ R) / W.sum(dim=0).clamp_min(EPS)[:, None]
    R = V / (W @ H).clamp_min(EPS)
    W = W * (R @ H.t()) / H.sum(dim=1).clamp_min(EPS)[None, :]
    return W, H


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=10336)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_nmf: no GPU visible")
    torch.set_grad_enabled(False)
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    start, stop = _lib.HipEvent(), _lib.HipEvent()
    results = []
    for F, K in SHAPES:
        T = a.frames
        rng = np.random.default_rng(F * 100 + K)
        V = torch.from_numpy(np.maximum(rng.gamma(2.0, 1.0, (F, T)), 1e-3).astype(np.float32)).to(dev)
        W0 = torch.from_numpy((0.5 + rng.random((F, K))).astype(np.float32)).to(dev)
        H0 = torch.from_numpy((0.5 + rng.random((K, T))).astype(np.float32)).to(dev)
        W, H = W0.clone(), H0.clone()

        def hip(n_iter, update_w, update_h):
            _lib.check(lib.maua_nmf_kl_f32(V.data_ptr(), W.data_ptr(), H.data_ptr(), F, T, K, n_iter, update_w, update_h, EPS,
                                           _lib.stream_ptr(dev)), "maua_nmf_kl_f32")

        def torch_loop(n_iter):
            w, h = W, H
            for _ in range(n_iter):
                w, h = torch_iteration(V, w, h)
            return w, h

        # the two formulations compute the same thing
        hip(10, 1, 1)
        Wt, Ht = W0, H0
        for _ in range(10):
            Wt, Ht = torch_iteration(V, Wt, Ht)
        agree = max(float(((W - Wt).abs() / Wt).max()), float(((H - Ht).abs() / Ht).max()))

        variants = {"hip_h_step": lambda: hip(a.iters, 0, 1), "hip_w_step": lambda: hip(a.iters, 1, 0), "hip_iteration": lambda: hip(a.iters, 1, 1),
                    "torch_iteration": lambda: torch_loop(a.iters)}
        times = {name: [] for name in variants}
        for rnd in range(a.rounds + 1):  # the first round warms every variant and is not counted
            for name, fn in variants.items():
                W.copy_(W0), H.copy_(H0)
                torch.cuda.synchronize()
                start.record()
                fn()
                stop.record()
                torch.cuda.synchronize()
                if rnd:
                    times[name].append(start.elapsed_ms(stop) / a.iters)
        v_bytes = 2 * F * T * 4
        row = {"F": F, "T": T, "K": K, "iters_per_window": a.iters, "v_bytes_per_iteration": v_bytes, "max_rel_difference_after_10": agree}
        for name, ts in times.items():
            row[f"{name}_ms_min"], row[f"{name}_ms_median"] = min(ts), statistics.median(ts)
        row["v_gbytes_per_s_at_hip_iteration"] = v_bytes / (row["hip_iteration_ms_min"] * 1e-3) / 1e9
        row["fma_per_iteration"] = 4 * F * T * K
        results.append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"device": _lib.device_info()["name"], "shapes": results}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
