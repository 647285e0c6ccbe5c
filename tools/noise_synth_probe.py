"""Cost of synthesised noise slots (ar.NoiseSynth, maua_noise_synth_f32) on the 1024^2 bench generator.  Prints one JSON line.

    python tools/noise_synth_probe.py [--batch 8] [--period 110] [--reps 200] [--replays 60] [--rounds 3]

Configuration of profiles/noise_synth.md: the two 512^2 and the two 1024^2 noise layers each get a recipe of two loop terms with an envelope
each (one 4-byte write and two 4-byte reads per element: batch 8 moves 0.25 GB).

  launch_us / launch_gbps   the launch alone, device events around ``reps`` launches on one stream, the frame moving by ``batch`` per launch
                            so that consecutive launches read other rows of the loops (2.3 GB of banks: nothing stays in the 256 MB cache);
  replay_ms_static / _synth one lane's replay (frame-source seek + graph launch) of ``batch`` frames with every slot on the checkpoint's
                            buffers / with the four slots synthesised, ``replays`` replays per timing, ``rounds`` timings of each, alternating.
"""
import argparse
import json
import os
import sys


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--period", type=int, default=110)
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--replays", type=int, default=60)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--size", type=int, default=1024)
    args = ap.parse_args()
    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

    import torch

    import maua_stylegan2_amd.audioreactive as ar
    from maua_stylegan2_amd import _lib, seeding
    from maua_stylegan2_amd.models.stylegan2 import Generator

    torch.set_grad_enabled(False)
    dev = torch.device("cuda:0")
    g = Generator(args.size, 512, 8, channel_multiplier=2, constant_input=True)
    g.load_state_dict(seeding.seeded_state_dict(args.size, seed=0))
    g = g.to(dev).eval()
    n = args.replays * args.batch
    gen = torch.Generator(device=dev)
    gen.manual_seed(1000)
    lat = torch.randn(n, g.n_latent, 512, device=dev, generator=gen)
    sizes = seeding.noise_sizes(args.size)
    slots = [i for i, s in enumerate(sizes) if s >= args.size // 2]
    recipes = {}
    for i in slots:
        s = sizes[i]
        terms = [ar.noise_term(torch.randn(args.period, 1, s, s, device=dev, generator=gen), envelope=torch.rand(n, device=dev, generator=gen),
                               phase=7 * k) for k in range(2)]
        recipes[i] = ar.NoiseSynth(s, s, terms, gain=0.4)
    out = {"device": _lib.device_info()["name"], "batch": args.batch, "period": args.period, "slots": {i: sizes[i] for i in slots},
           "bank_gb": round(sum(t.numel() for r in recipes.values() for t in r.tensors()) * 4 / 1e9, 2)}

    # ---- the launch alone
    lib, st = _lib.load(), _lib.stream_ptr(dev)
    maps = {i: torch.empty(args.batch, 1, sizes[i], sizes[i], device=dev) for i in slots}
    host = (_lib.NoiseSynthSlot * len(slots))(*[recipes[i].table_entry(maps[i].data_ptr(), i) for i in slots])
    table = torch.frombuffer(bytearray(bytes(host)), dtype=torch.uint8).to(dev)
    moved = sum(m.numel() for m in maps.values()) * 4 * 3
    for r in range(10):
        _lib.check(lib.maua_noise_synth_f32(table.data_ptr(), len(slots), args.batch, args.batch * r, None, st), "maua_noise_synth_f32")
    times = []
    for _ in range(args.rounds):
        torch.cuda.synchronize(dev)
        start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        start.record()
        for r in range(args.reps):
            # (src == NULL: the envelopes are read from their start; frame0 moves the loops)
            _lib.check(lib.maua_noise_synth_f32(table.data_ptr(), len(slots), args.batch, args.batch * r, None, st), "maua_noise_synth_f32")
        stop.record()
        stop.synchronize()
        times.append(start.elapsed_time(stop) * 1e3 / args.reps)
    out["launch_us"] = [round(t, 2) for t in times]
    out["launch_mb"] = round(moved / 1e6, 1)
    out["launch_gbps"] = [round(moved / (t * 1e-6) / 1e9, 1) for t in times]

    # ---- one lane's replay with and without the synthesised slots
    stream = torch.cuda.Stream(dev)
    with torch.cuda.stream(stream):
        lanes = {"static": g.capture_graph(args.batch, lane=0, frames_u8=True),
                 "synth": g.capture_graph(args.batch, lane=1, frames_u8=True, synth_slots=tuple(slots))}
        noise = [None] * g.num_layers
        lanes["static"].bind(lat, noise)
        lanes["synth"].bind(lat, [recipes.get(i) for i in range(g.num_layers)])
        result = {k: [] for k in lanes}
        for name, lane in lanes.items():  # warm-up
            for r in range(5):
                lane.replay(r * args.batch)
        for _ in range(args.rounds):
            for name, lane in lanes.items():
                stream.synchronize()
                start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                start.record(stream)
                for r in range(args.replays):
                    lane.replay(r * args.batch)
                stop.record(stream)
                stop.synchronize()
                result[name].append(round(start.elapsed_time(stop) / args.replays, 4))
    out["replay_ms_static"], out["replay_ms_synth"] = result["static"], result["synth"]
    print(json.dumps(out))


if __name__ == "__main__":
    main()
