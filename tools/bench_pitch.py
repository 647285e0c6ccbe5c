#!/usr/bin/env python3
"""Timing of the pitch tracker on the MI355X (the figures of profiles/pitch.md):

    python tools/bench_pitch.py [--seconds 240] [--reps 3] [--out pitch_bench.json]

  * maua_yin_f32 alone, by device events, at ar.raw_pitch's defaults (frame 2048, hop 512, lags 10 .. 340 at 22050 Hz) on a seeded synthetic
    clip: a window of 50 back-to-back launches after 5 warm-up launches, and the per-launch minimum / median of 50 single launches;
  * ar.pitch and ar.chroma (defaults, n_frames = 30 fps) on the same clip in the same warm process, alternating, host clock around a
    device synchronise.
Needs a GPU: there is no fallback."""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

import maua_stylegan2_amd.audioreactive as ar  # noqa: E402
from maua_stylegan2_amd import _lib  # noqa: E402

SR, FRAME, HOP, TAU_MIN, TAU_MAX, THRESHOLD = 22050, 2048, 512, 10, 340, 0.1


def clip(seconds, seed=0):
    """A melody of half-second notes (harmonics 1-4, a bass note an octave and a fifth below) with a noise floor."""
    rng = np.random.default_rng(seed)
    n = int(seconds * SR)
    t = np.arange(n, dtype=np.float64) / SR
    notes = 110.0 * 2.0 ** (rng.integers(0, 30, size=int(seconds * 2) + 1) / 12.0)
    f = notes[np.minimum((t * 2).astype(np.int64), len(notes) - 1)]
    phase = 2 * np.pi * np.cumsum(f) / SR
    y = sum(np.sin(h * phase) / h for h in (1, 2, 3, 4)) * 0.2 + 0.1 * np.sin(phase / 3.0) + 0.01 * rng.standard_normal(n)
    return y.astype(np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=240.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_pitch: no GPU visible")
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    audio = clip(a.seconds)
    y = torch.from_numpy(audio).to(dev)
    n = y.numel()
    n_frames = 1 + n // HOP
    lag, apd = torch.empty(n_frames, device=dev), torch.empty(n_frames, device=dev)
    tau = torch.empty(n_frames, dtype=torch.int32, device=dev)

    def launch():
        _lib.check(lib.maua_yin_f32(y.data_ptr(), n, FRAME, HOP, TAU_MIN, TAU_MAX, THRESHOLD, lag.data_ptr(), apd.data_ptr(), tau.data_ptr(),
                                    None, n_frames, _lib.stream_ptr(dev)), "maua_yin_f32")

    for _ in range(5):
        launch()
    torch.cuda.synchronize()
    start, stop = _lib.HipEvent(), _lib.HipEvent()
    start.record()
    for _ in range(50):
        launch()
    stop.record()
    torch.cuda.synchronize()
    window_ms = start.elapsed_ms(stop) / 50
    singles = []
    for _ in range(50):
        start.record()
        launch()
        stop.record()
        torch.cuda.synchronize()
        singles.append(start.elapsed_ms(stop))
    pairs = n_frames * FRAME * TAU_MAX  # (x[j] - x[j + tau])^2 terms: one subtract and one fma each
    result = {"clip_seconds": a.seconds, "sr": SR, "n_frames": n_frames, "frame": FRAME, "hop": HOP, "tau": [TAU_MIN, TAU_MAX],
              "difference_terms": pairs, "yin_ms_window_of_50": window_ms, "yin_ms_single_min": min(singles),
              "yin_ms_single_median": statistics.median(singles), "yin_terms_per_second": pairs / (window_ms * 1e-3),
              "voiced_fraction": float((apd < 0.5).float().mean())}

    video_frames = int(a.seconds * 30)
    timings = {"pitch": [], "chroma": [], "pitch_margin_none": []}
    calls = {"pitch": lambda: ar.pitch(audio, SR, video_frames, device="cuda"),
             "chroma": lambda: ar.chroma(audio, SR, video_frames, device="cuda"),
             "pitch_margin_none": lambda: ar.pitch(audio, SR, video_frames, margin=None, device="cuda")}
    for rep in range(a.reps + 1):  # the first round warms every shape and is not counted
        for name, fn in calls.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if rep:
                timings[name].append(time.perf_counter() - t0)
    for name, ts in timings.items():
        result[f"{name}_s"] = ts
        result[f"{name}_s_median"] = statistics.median(ts)
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
