#!/usr/bin/env python3
"""Timing of the dense-transition HMM entries and of the chord features on the MI355X (the figures of profiles/hmm.md):

    python tools/bench_hmm.py [--seconds 240] [--reps 5] [--torch-frames 2000] [--out hmm_bench.json]

  * maua_hmm_viterbi_f64 alone and maua_hmm_posterior_f64 alone at S = 25 and S = 97 states, T = 1 + seconds * 22050 / 512 frames
    (10 336 for 240 s), by device events around single launches after warm-up launches (minimum / median / maximum), on random
    observations and the chord model's transition matrix;
  * the same two recursions written as torch ops on the device (a per-frame loop in float64; a handful of launches per frame) on the
    first --torch-frames frames, and as numpy on the host (vectorised over the states, a per-frame loop) on all frames;
  * ar.chords against ar.chroma end to end on a synthetic chord progression of that length, alternating in one warm process, host
    clock around a device synchronise.
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
from maua_stylegan2_amd.audioreactive import harmony  # noqa: E402

SR, HOP = 22050, 512


def progression(seconds, seed=0):
    """C Am F G in a loop, two seconds a chord: three notes of six decaying partials each, a noise click every half second."""
    n_chord = 2 * SR
    t = np.arange(n_chord) / SR
    env = np.minimum(t / 0.02, 1.0) * np.exp(-0.7 * t)
    c3 = 440.0 * 2.0 ** (-21 / 12)
    chords = []
    for pcs in ((0, 4, 7), (9, 0, 4), (5, 9, 0), (7, 11, 2)):
        y = np.zeros(n_chord)
        for pc in pcs:
            for h in range(1, 7):
                y += 0.6 ** h * np.sin(2 * np.pi * c3 * 2.0 ** (pc / 12) * h * t)
        chords.append(y * env)
    n = int(seconds * SR)
    y = np.tile(np.concatenate(chords), n // (4 * n_chord) + 1)[:n]
    rng = np.random.default_rng(seed)
    for at in range(0, n - SR // 100, SR // 2):
        y[at: at + SR // 100] += 2.0 * rng.standard_normal(SR // 100)
    return (0.9 * y / np.abs(y).max()).astype(np.float32)


def event_times(launch, warm=3, reps=10):
    for _ in range(warm):
        launch()
    torch.cuda.synchronize()
    start, stop = _lib.HipEvent(), _lib.HipEvent()
    out = []
    for _ in range(reps):
        start.record()
        launch()
        stop.record()
        torch.cuda.synchronize()
        out.append(start.elapsed_ms(stop))
    return {"min": min(out), "median": statistics.median(out), "max": max(out)}


def torch_viterbi(logobs, log_trans, log_init):
    lo = logobs.double()
    delta = log_init + lo[0]
    back = torch.zeros(lo.shape, dtype=torch.uint8, device=lo.device)
    for t in range(1, lo.shape[0]):
        best, back[t] = (delta[:, None] + log_trans).max(dim=0)
        delta = best + lo[t]
    return delta, back


def torch_posterior(obs, trans, init):
    ob = obs.double()
    T = ob.shape[0]
    gamma, scale = torch.empty_like(ob), torch.empty(T, dtype=torch.float64, device=ob.device)
    a = init * ob[0]
    for t in range(T):
        if t:
            a = (gamma[t - 1] @ trans) * ob[t]
        scale[t] = a.sum()
        gamma[t] = a / scale[t]
    beta = torch.ones_like(a)
    for t in range(T - 2, -1, -1):
        beta = (trans @ (ob[t + 1] * beta)) / scale[t + 1]
        gamma[t] *= beta
    return gamma, scale


def numpy_viterbi(logobs, log_trans, log_init):
    lo = logobs.astype(np.float64)
    delta = log_init + lo[0]
    back = np.zeros(lo.shape, np.uint8)
    for t in range(1, lo.shape[0]):
        cand = delta[:, None] + log_trans
        back[t] = cand.argmax(0)
        delta = cand.max(0) + lo[t]
    return delta, back


def numpy_posterior(obs, trans, init):
    ob = obs.astype(np.float64)
    T = ob.shape[0]
    gamma, scale = np.empty_like(ob), np.empty(T)
    a = init * ob[0]
    for t in range(T):
        if t:
            a = (gamma[t - 1] @ trans) * ob[t]
        scale[t] = a.sum()
        gamma[t] = a / scale[t]
    beta = np.ones_like(a)
    for t in range(T - 2, -1, -1):
        beta = (trans @ (ob[t + 1] * beta)) / scale[t + 1]
        gamma[t] *= beta
    return gamma, scale


def host_ms(fn, reps=2):
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(1e3 * (time.perf_counter() - t0))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=240.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--torch-frames", type=int, default=2000)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_hmm: no GPU visible")
    lib = _lib.load()
    dev = torch.device("cuda", 0)
    stream = _lib.stream_ptr(dev)
    T = 1 + int(a.seconds * SR) // HOP
    result = {"clip_seconds": a.seconds, "sr": SR, "hop": HOP, "n_frames": T, "torch_frames": min(a.torch_frames, T)}
    rng = np.random.default_rng(0)
    for S in (25, 97):
        log_trans_h, log_init_h = harmony.chord_transitions(S, SR / HOP, 1.0)
        logobs_h = (20.0 * rng.random((T, S))).astype(np.float32)
        logobs = torch.from_numpy(logobs_h).to(dev)
        obs = harmony.likelihoods(logobs)
        log_trans, log_init = torch.from_numpy(log_trans_h).to(dev), torch.from_numpy(log_init_h).to(dev)
        trans, init = log_trans.exp(), log_init.exp()
        delta = torch.empty(S, dtype=torch.float64, device=dev)
        back = torch.empty((T, S), dtype=torch.uint8, device=dev)
        states = torch.empty(T, dtype=torch.int32, device=dev)
        gamma = torch.empty((T, S), dtype=torch.float64, device=dev)
        scale = torch.empty(T, dtype=torch.float64, device=dev)

        def viterbi(frames=T):
            _lib.check(lib.maua_hmm_viterbi_f64(logobs.data_ptr(), log_trans.data_ptr(), log_init.data_ptr(), frames, S, delta.data_ptr(),
                                                back.data_ptr(), states.data_ptr(), stream), "maua_hmm_viterbi_f64")

        def posterior(frames=T):
            _lib.check(lib.maua_hmm_posterior_f64(obs.data_ptr(), trans.data_ptr(), init.data_ptr(), frames, S, gamma.data_ptr(), scale.data_ptr(),
                                                  stream), "maua_hmm_posterior_f64")

        r = {"viterbi_ms": event_times(viterbi), "posterior_ms": event_times(posterior)}
        r["viterbi_us_per_frame"] = 1e3 * r["viterbi_ms"]["median"] / T
        r["posterior_us_per_frame"] = 1e3 * r["posterior_ms"]["median"] / T
        n = result["torch_frames"]
        r["viterbi_ms_torch_frames"] = event_times(lambda: viterbi(n))
        r["posterior_ms_torch_frames"] = event_times(lambda: posterior(n))
        kernel_delta, kernel_gamma = delta.clone(), gamma[:n].clone()
        host_ms(lambda: torch_viterbi(logobs[:64], log_trans, log_init), 1)  # (warm the shapes)
        host_ms(lambda: torch_posterior(obs[:64], trans, init), 1)
        r["torch_viterbi_ms"] = host_ms(lambda: torch_viterbi(logobs[:n], log_trans, log_init))
        r["torch_posterior_ms"] = host_ms(lambda: torch_posterior(obs[:n], trans, init))
        t_delta, _ = torch_viterbi(logobs[:n], log_trans, log_init)
        t_gamma, _ = torch_posterior(obs[:n], trans, init)
        r["torch_delta_equals_kernel"] = bool(torch.equal(t_delta, kernel_delta))
        r["torch_gamma_max_difference"] = float((t_gamma - kernel_gamma).abs().max())
        obs_h = obs.cpu().numpy()
        r["numpy_viterbi_ms"] = host_ms(lambda: numpy_viterbi(logobs_h, log_trans_h, log_init_h))
        r["numpy_posterior_ms"] = host_ms(lambda: numpy_posterior(obs_h, np.exp(log_trans_h), np.exp(log_init_h)))
        result[f"S{S}"] = r

    audio = progression(a.seconds)
    video_frames = int(a.seconds * 30)
    calls = {"chroma": lambda: ar.chroma(audio, SR, video_frames, device="cuda"),
             "chroma_margin_0": lambda: ar.chroma(audio, SR, video_frames, margin=0, device="cuda"),
             "chords_triads": lambda: ar.chords(audio, SR, video_frames, device="cuda"),
             "chords_sevenths": lambda: ar.chords(audio, SR, video_frames, device="cuda", vocabulary="sevenths"),
             "key": lambda: ar.key(audio, SR)}
    timings = {name: [] for name in calls}
    for rep in range(a.reps + 1):  # the first round warms every shape and is not counted
        for name, fn in calls.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            if rep:
                timings[name].append(1e3 * (time.perf_counter() - t0))
    for name, ts in timings.items():
        result[f"{name}_ms"] = ts
        result[f"{name}_ms_median"] = statistics.median(ts)
    track = ar.raw_chords(audio, SR)
    result["chord_changes_decoded"] = int((track.labels[1:] != track.labels[:-1]).sum())
    line = json.dumps(result)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
