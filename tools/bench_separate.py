#!/usr/bin/env python3
"""Timing of the source separation on the MI355X (the figures of profiles/separate.md):

    python tools/bench_separate.py [--frames 10336] [--reps 20] [--rounds 3] [--out separate_bench.json]

For the shapes of a 240 s clip (F = 1025 bins, T = 10336 frames) at K = 8 and 16 components in G = 2 and 8 stems (contiguous runs,
``numpy.array_split``), power 2, on seeded data, in one warm process:
  * maua_nmf_separate_f32 for all G stems in one launch: (2 + 2 G) F T 4 bytes read and written, and the rate that gives,
  * a device-to-device copy of the same number of bytes (``Tensor.copy_``), measured in the same run: the rate the launch is set against,
  * the same masks written as torch ops on the same device (per-group matrix products, a square, a sum, a division and two products;
    every intermediate materialised), for information,
each timed by device events around ``--reps`` back-to-back calls after a warm-up round, the variants alternating over ``--rounds``
rounds (minimum and median reported, per call), and
  * the whole ``ar.separate`` of a 240 s clip of seeded noise (STFT, 200 iterations of KL-NMF, masks, G inverse STFTs, the copy to the
    host), wall clock around a synchronised call, once per shape after one warm call.
Also the largest relative difference between the kernel and the torch formulation.  Nothing here asserts a speed.  Needs a GPU: there
is no fallback."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from maua_stylegan2_amd import _lib  # noqa: E402

F = 1025
SHAPES = ((8, 2), (8, 8), (16, 2), (16, 8))
POWER = 2


def torch_masks(re, im, W, H, runs, power):
    q = torch.stack([W[:, run] @ H[run] for run in runs])
    if power == 2:
        q = q * q
    D = q.sum(dim=0)
    m = torch.where(D > 0, q / D, torch.full_like(q, 1.0 / len(runs)))
    return m * re, m * im


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=10336)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_separate: no GPU visible")
    torch.set_grad_enabled(False)
    import maua_stylegan2_amd.audioreactive as ar

    lib = _lib.load()
    dev = torch.device("cuda", 0)
    start, stop = _lib.HipEvent(), _lib.HipEvent()
    T = a.frames
    clip = np.random.default_rng(1).standard_normal((T - 1) * 512).astype(np.float32) * 0.1
    results = []
    for K, G in SHAPES:
        rng = np.random.default_rng(K * 100 + G)
        re = torch.from_numpy(rng.standard_normal((F, T)).astype(np.float32)).to(dev)
        im = torch.from_numpy(rng.standard_normal((F, T)).astype(np.float32)).to(dev)
        W = torch.from_numpy((0.5 + rng.random((F, K))).astype(np.float32)).to(dev)
        H = torch.from_numpy((0.5 + rng.random((K, T))).astype(np.float32)).to(dev)
        runs = [torch.from_numpy(run).to(dev) for run in np.array_split(np.arange(K), G)]
        group = np.concatenate([np.full(len(run), g, np.int32) for g, run in enumerate(np.array_split(np.arange(K), G))])
        table = (ctypes.c_int32 * K)(*group.tolist())
        out_re = torch.empty((G, F, T), dtype=torch.float32, device=dev)
        out_im = torch.empty_like(out_re)
        n_bytes = (2 + 2 * G) * F * T * 4
        src = torch.empty(n_bytes // 2, dtype=torch.uint8, device=dev).fill_(1)  # a copy reads and writes: half the bytes each way
        dst = torch.empty_like(src)

        def hip():
            _lib.check(lib.maua_nmf_separate_f32(re.data_ptr(), im.data_ptr(), W.data_ptr(), H.data_ptr(), table, F, T, K, G, POWER, 0, G,
                                                 out_re.data_ptr(), out_im.data_ptr(), _lib.stream_ptr(dev)), "maua_nmf_separate_f32")

        hip()
        t_re, t_im = torch_masks(re, im, W, H, runs, POWER)
        scale = float(re.abs().max())
        agree = max(float((out_re - t_re).abs().max()), float((out_im - t_im).abs().max())) / scale
        del t_re, t_im

        variants = {"hip_masks": hip, "device_copy": lambda: dst.copy_(src), "torch_masks": lambda: torch_masks(re, im, W, H, runs, POWER)}
        times = {name: [] for name in variants}
        for rnd in range(a.rounds + 1):  # the first round warms every variant and is not counted
            for name, fn in variants.items():
                torch.cuda.synchronize()
                start.record()
                for _ in range(a.reps):
                    fn()
                stop.record()
                torch.cuda.synchronize()
                if rnd:
                    times[name].append(start.elapsed_ms(stop) / a.reps)
        row = {"F": F, "T": T, "K": K, "G": G, "power": POWER, "reps_per_window": a.reps, "bytes_per_call": n_bytes,
               "max_difference_from_torch_over_max_input": agree}
        for name, ts in times.items():
            row[f"{name}_ms_min"], row[f"{name}_ms_median"] = min(ts), statistics.median(ts)
        row["hip_masks_gbytes_per_s"] = n_bytes / (row["hip_masks_ms_min"] * 1e-3) / 1e9
        row["device_copy_gbytes_per_s"] = n_bytes / (row["device_copy_ms_min"] * 1e-3) / 1e9
        del out_re, out_im, src, dst
        whole = []
        for _ in range(2):  # the first call warms the constants and the allocator
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            ar.separate(clip, 22050, n_components=K, groups=G, power=POWER, n_iter=200)
            torch.cuda.synchronize()
            whole.append(time.perf_counter() - t0)
        row["separate_240s_clip_s"] = whole[-1]
        results.append(row)
        print(json.dumps(row), flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump({"device": _lib.device_info()["name"], "shapes": results}, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
