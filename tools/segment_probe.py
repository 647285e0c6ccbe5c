"""Per-stage wall time of laplacian_segmentation on a synthetic 5-minute track (22050 Hz, 128 bpm, sections of 32 beats).

    python tools/segment_probe.py [--seconds 300] [--out segment_probe.json]

Each stage is timed with a device synchronise on both sides, after one warm-up pass of the whole pipeline; the result is one JSON
line (seconds per stage, the constant-Q transform separate from the new kernels)."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from maua_stylegan2_amd.audioreactive import segment  # noqa: E402
from maua_stylegan2_amd.audioreactive import signal as sig  # noqa: E402


def track(seconds, sr=22050, bpm=128, seed=0):
    rng = np.random.default_rng(seed)
    n = int(seconds * sr)
    t = np.arange(n) / sr
    y = 2e-3 * rng.standard_normal(n)
    beat = 60.0 / bpm
    chords = [(220.0, 277.18, 329.63), (146.83, 185.0, 220.0), (196.0, 246.94, 293.66), (164.81, 207.65, 246.94)]
    sec = 32 * beat
    for s in range(int(np.ceil(seconds / sec))):
        a, b = int(s * sec * sr), min(n, int((s + 1) * sec * sr))
        for f in chords[(s * 7 // 3) % 4]:
            y[a:b] += 0.15 * np.sin(2 * np.pi * f * t[a:b])
    kick = np.sin(2 * np.pi * 60 * np.arange(1764) / sr) * np.exp(-np.arange(1764) / 441.0)
    for q in range(int(seconds / beat)):
        a = int(q * beat * sr)
        y[a: a + kick.size] += 0.8 * kick[: max(0, min(kick.size, n - a))]
    return y.astype(np.float32)


def run(y, sr, k, times):
    dev = torch.device("cuda", torch.cuda.current_device())

    def stage(name, fn):
        torch.cuda.synchronize(dev)
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize(dev)
        times[name] = times.get(name, 0.0) + time.perf_counter() - t0
        return out

    audio = stage("upload", lambda: torch.from_numpy(y).to(dev))
    env, power = stage("onset_envelope (stft + mel + median)", lambda: segment.onset_envelope(audio, sr))
    win = int(8.0 * sr) // 512
    tg = stage("tempogram [new]", lambda: segment.tempogram(env, win))
    tempo = segment.tempo_from_tempogram(tg.cpu().numpy(), sr)
    period = int(round(60.0 * sr / 512 / tempo))
    x = env.double() / env.double().std()
    ls, cs, bl = stage("beat DP [new]", lambda: segment.beat_dp(x, period))
    _, beats = stage("beat track total (tempogram + DP + host walk)", lambda: segment.beat_track(env, sr))
    c, mfcc = stage("features (tuning + CQT + MFCC) [existing]", lambda: segment.features(audio, sr, power))
    bounds = segment.sync_bounds(beats, c.shape[1])
    csync = stage("beat sync median [new]", lambda: segment.beat_sync(c, bounds, True))
    msync = stage("beat sync mean [new]", lambda: segment.beat_sync(mfcc, bounds, False))
    links = stage("knn links [new]", lambda: segment.knn_links(csync, segment.knn_count(csync.shape[1])))
    bw = stage("bandwidth (torch)", lambda: segment.link_bandwidth(links))
    _, rf = stage("affinity + time-lag median [new]", lambda: segment.rec_affinity(links, bw))
    emb = stage("Laplacian + eigh + median filter (torch / existing)", lambda: segment.spectral_embedding(rf, msync, k).cpu().numpy())
    seg = stage("k-means (host)", lambda: segment.kmeans(emb, k))
    stage("boundaries (host)", lambda: segment.segment_boundaries(seg, beats, c.shape[1], sr))
    return csync.shape[1]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=300.0)
    ap.add_argument("--k", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("segment_probe: no GPU")
    sr = 22050
    y = track(a.seconds, sr)
    run(y, sr, a.k, {})  # warm-up
    times = {}
    n_cols = run(y, sr, a.k, times)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    segment.laplacian_segmentation(y, sr, k=a.k)
    total = time.perf_counter() - t0
    new = sum(v for name, v in times.items() if "[new]" in name)
    res = {"seconds_of_audio": a.seconds, "sync_columns": n_cols, "stages_s": {k: round(v, 5) for k, v in times.items()},
           "new_kernels_s": round(new, 5), "features_with_cqt_s": round(times["features (tuning + CQT + MFCC) [existing]"], 5),
           "laplacian_segmentation_total_s": round(total, 4)}
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(a.out) or ".", exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
