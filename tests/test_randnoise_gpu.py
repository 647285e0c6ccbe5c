"""GPU: the counter-based noise generator (csrc/noise.hip, maua_randn_frames_f32) against the float64 restatement of its definition
(tests/philox_ref.py), and seeded ``randomize_noise`` renders through ``render.synthesize``.

Tolerance of the float comparison (the convention of tests/test_signal_entries_gpu.py): 4 x the float32-vs-float64 error of the numpy
restatement evaluated in float32 over the SAME cases — seed 0x123456789ABCDEF0, the 23 frames {f0 + b : f0 in (0, 7, 2^31 - 9), b < 8}, every
slot at its largest map (slot i of the 1920-wide generator, whose prefix the 1024^2 and 256^2 maps of that slot are) — measured on the CPU:

    slot  hw        max |f32 - f64|        slot  hw        max |f32 - f64|
    0     32        9.84e-07               11    131072    1.89e-06
    1     128       9.67e-07               12    131072    1.66e-06
    2     128       8.95e-07               13    524288    1.75e-06
    3     512       1.00e-06               14    524288    1.73e-06
    4     512       1.34e-06               15    2097152   1.85e-06
    5     2048      1.28e-06               16    2097152   2.05e-06
    6     2048      1.29e-06               17    1         2.15e-07
    7     8192      1.59e-06               18    3         9.36e-07
    8     8192      1.63e-06               19    5         5.21e-07
    9     32768     1.56e-06               20    35        7.00e-07
    10    32768     1.51e-06               overall         2.049e-06   ->  TOL = 8.2e-06

(it comes from the float32 angle 2 pi u and from ln u; the kernel takes the angle in half turns, so its own error is expected below that of
the float32 restatement)."""
import ctypes

import numpy as np
import pytest
import torch

import philox_ref as pr
from redzone import Guard

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

SEED = 0x123456789ABCDEF0
TOL = 4 * 2.049e-6
RES = [4] + [r for k in range(3, 11) for r in (2 ** k, 2 ** k)]            # 17 noise layers of a 1024^2 generator
SHAPES = {
    "1024": [(i, r * r) for i, r in enumerate(RES)],
    "256": [(i, r * r) for i, r in enumerate(RES[:13])],
    "1920-wide": [(i, 2 * r * r) for i, r in enumerate(RES)],               # 4 x 8 ... 1024 x 2048
    "odd": [(17, 1), (18, 3), (19, 5), (20, 35)],
}
SRC_DWORDS = 134  # sizeof(maua_frame_source_t) / 4
NOISE_DW, STRIDE_DW = 6, 6 + 64  # dword offsets of noise[] and noise_stride[] inside the struct


def _table_words(entries, maps):
    words = []
    for (slot, hw), t in zip(entries, maps):
        p = t.data_ptr()
        words += [p & 0xFFFFFFFF, p >> 32, hw, slot & 0xFFFFFFFF]
    return np.array(words, dtype=np.uint32).view(np.int32)


def _launch(dev, entries, batch, seed, frame0, form, guard=None):
    """One maua_randn_frames_f32 launch into red-zoned windows.  form "arg": frames from the frame0 argument; "src": from a frame source
    whose frame0 was set with maua_frame_source_seek (argument 0).  Returns (guard, maps, src words before, src view or None)."""
    from maua_stylegan2_amd import _lib

    lib = _lib.load()
    g = guard or Guard(dev)
    maps = [g.out((batch, hw), f"dst{slot}") for slot, hw in entries]
    table = g.inp(_table_words(entries, maps), "table", torch.int32)
    st = _lib.stream_ptr(dev)
    src, before = None, None
    if form == "src":
        src = g.out((SRC_DWORDS,), "src", torch.int32)
        src.copy_(torch.arange(SRC_DWORDS, dtype=torch.int32) + 0x5A000000)  # recognisable words everywhere
        _lib.check(lib.maua_frame_source_seek(src.data_ptr(), frame0, st), "seek")
        before = src.clone()
        rc = lib.maua_randn_frames_f32(table.data_ptr(), len(entries), batch, seed, 0, src.data_ptr(), st)
    else:
        rc = lib.maua_randn_frames_f32(table.data_ptr(), len(entries), batch, seed, frame0, None, st)
    assert rc == 0, rc
    g.check(written=[f"dst{slot}" for slot, _ in entries])
    return g, maps, before, src


def _check_source_words(entries, maps, before, src, frame0):
    """Only the pointer / stride words of the generated slots changed, to dst - frame0 * hw and hw."""
    after, was = src.cpu().numpy().copy(), before.cpu().numpy()
    assert after[0] == frame0
    for (slot, hw), t in zip(entries, maps):
        ptr = int(after[NOISE_DW + 2 * slot: NOISE_DW + 2 * slot + 2].view(np.uint64)[0])
        stride = int(after[STRIDE_DW + 2 * slot: STRIDE_DW + 2 * slot + 2].view(np.int64)[0])
        assert stride == hw and ptr == (t.data_ptr() - frame0 * hw * 4) % 2 ** 64, (slot, hex(ptr), stride)
        after[NOISE_DW + 2 * slot: NOISE_DW + 2 * slot + 2] = was[NOISE_DW + 2 * slot: NOISE_DW + 2 * slot + 2]
        after[STRIDE_DW + 2 * slot: STRIDE_DW + 2 * slot + 2] = was[STRIDE_DW + 2 * slot: STRIDE_DW + 2 * slot + 2]
    assert np.array_equal(after, was), "words of the frame source outside the generated slots changed"


def test_kernel_matches_the_float64_reference_on_every_slot_shape(gpu):
    """Every slot shape of the 1024^2, the 256^2 and the 1920-wide generators + hw in {1, 3, 5, 35}, batch in {1, 3, 8}, frame0 in
    {0, 7, 2^31 - 9}, both forms; red zones around every map, the table and the frame source."""
    frames0 = (0, 7, 2 ** 31 - 9)
    cases = []
    for name, entries in SHAPES.items():
        for batch in (1, 3, 8):
            for f0 in frames0:
                for form in ("arg", "src"):
                    _, maps, before, src = _launch(gpu, entries, batch, SEED, f0, form)
                    if form == "src":
                        _check_source_words(entries, maps, before, src, f0)
                    cases.append((name, entries, batch, f0, form, maps))
    hw_max = {}
    for entries in SHAPES.values():
        for slot, hw in entries:
            hw_max[slot] = max(hw_max.get(slot, 0), hw)
    worst = {}
    for frame in sorted({f0 + b for f0 in frames0 for b in range(8)}):
        for slot, hw_ref in hw_max.items():
            ref = torch.from_numpy(pr.noise_map(SEED, frame, slot, hw_ref)).to(gpu)
            for name, entries, batch, f0, form, maps in cases:
                b = frame - f0
                if not 0 <= b < batch:
                    continue
                for (s, hw), t in zip(entries, maps):
                    if s == slot:
                        err = float((t[b].double() - ref[:hw]).abs().max())
                        worst[name] = max(worst.get(name, 0.0), err)
                        assert err <= TOL, (name, slot, hw, batch, f0, form, frame, err)
    print("max |kernel - float64 reference| per shape family:", {k: f"{v:.3e}" for k, v in worst.items()}, f"TOL {TOL:.3e}")


def test_device_output_meets_the_moment_conditions(gpu):
    """The conditions of tests/test_randnoise_host.py on the device's own values (frames 0-1 x slots 0-1, hw = 2^20)."""
    _, maps, _, _ = _launch(gpu, [(0, 1 << 20), (1, 1 << 20)], 2, SEED, 0, "arg")
    got = np.stack([maps[s][f].cpu().numpy().astype(np.float64) for f in (0, 1) for s in (0, 1)])
    stats, z_max = pr.moment_statistics(got)
    print({k: round(float(v), 3) for k, v in stats.items()}, z_max)
    for name, value in stats.items():
        assert value <= 4.0, (name, value)
    assert z_max <= pr.Z_MAX


def test_maps_do_not_depend_on_the_batch_decomposition(gpu):
    """Frames 0..23 as 24 x batch 1, 8 x batch 3 and 3 x batch 8 are identical bit for bit (both forms), two runs are identical, and
    another seed, frame or slot changes every map."""
    entries = [(0, 16), (1, 64), (2, 35), (3, 5), (4, 4096), (5, 65536), (6, 4096)]

    def render(batch, seed=SEED, first=0, form="arg", entries=entries):
        parts = [_launch(gpu, entries, batch, seed, first + f0, form)[1] for f0 in range(0, 24, batch)]
        return [torch.cat([p[k] for p in parts]).view(torch.int32) for k in range(len(entries))]

    base = render(8)
    for other in (render(1), render(3), render(8), render(3, form="src"), render(1, form="src"), render(8, form="src")):
        for a, b in zip(base, other):
            assert torch.equal(a, b)
    for changed in (render(8, seed=SEED + 1), render(8, seed=SEED ^ (1 << 63)), render(8, first=1),
                    render(8, entries=[(slot + 7, hw) for slot, hw in entries])):
        for k, (a, b) in enumerate(zip(base, changed)):
            same = (a == b).view(24, -1).float().mean(dim=1)
            assert bool((same < 0.01).all()) and not any(torch.equal(a[f], b[f]) for f in range(24)), (k, same.max())
    assert torch.equal(base[4], render(8)[4]) and not torch.equal(base[4], base[6])  # same hw, other slot


def test_frame_source_rewrite_touches_only_the_generated_slots(gpu):
    """Slots 2, 9 and 31 generated at frame 1000 (a slot number outside the struct's table only names the counter word: its map is
    filled, no word of the struct is written for it); empty entries (dst NULL, hw 0) are skipped."""
    from maua_stylegan2_amd import _lib

    lib = _lib.load()
    g = Guard(gpu)
    entries = [(2, 35), (9, 1024), (31, 7), (40, 64)]
    maps = [g.out((3, hw), f"dst{slot}") for slot, hw in entries]
    words = _table_words(entries + [(5, 16), (6, 0)], maps + [torch.empty(0, device=gpu), maps[0]]).copy()
    words[4 * 4: 4 * 4 + 2] = 0  # entry 4: dst NULL
    table = g.inp(words, "table", torch.int32)
    src = g.out((SRC_DWORDS,), "src", torch.int32)
    src.copy_(torch.arange(SRC_DWORDS, dtype=torch.int32) + 0x5A000000)
    st = _lib.stream_ptr(gpu)
    _lib.check(lib.maua_frame_source_seek(src.data_ptr(), 1000, st), "seek")
    before = src.clone()
    assert lib.maua_randn_frames_f32(table.data_ptr(), 6, 3, SEED, 0, src.data_ptr(), st) == 0
    g.check(written=[f"dst{slot}" for slot, _ in entries])
    _check_source_words(entries[:3], maps[:3], before, src, 1000)
    for (slot, hw), t in zip(entries, maps):
        ref = torch.from_numpy(pr.noise_maps(SEED, 1000, 3, slot, hw)).to(gpu)
        assert float((t.double() - ref).abs().max()) <= TOL
    # the absolute frame of the src form is frame0 argument + src->frame0 (a shard's sequences start at the job's frame `frame0`)
    g2, maps2, _, _ = _launch(gpu, entries[:2], 3, SEED, 1000, "arg")
    g3 = Guard(gpu)
    maps3 = [g3.out((3, hw), f"dst{slot}") for slot, hw in entries[:2]]
    table3 = g3.inp(_table_words(entries[:2], maps3), "table", torch.int32)
    _lib.check(lib.maua_frame_source_seek(src.data_ptr(), 400, st), "seek")
    assert lib.maua_randn_frames_f32(table3.data_ptr(), 2, 3, SEED, 600, src.data_ptr(), st) == 0
    g3.check(written=["dst2", "dst9"])
    for a, b in zip(maps2, maps3):
        assert torch.equal(a, b)


# ------------------------------------------------------------------------------------------------ renders
SIZE, N, BATCH = 64, 26, 8  # three full batches + a tail of two


@pytest.fixture(scope="module")
def small(gpu):
    from maua_stylegan2_amd import seeding
    from maua_stylegan2_amd.models.stylegan2 import Generator

    g = Generator(SIZE, 512, 8, channel_multiplier=2, constant_input=True)
    g.load_state_dict(seeding.seeded_state_dict(SIZE, seed=5, rgb_gain=seeding.unsaturated_rgb_gain(SIZE)), strict=True)
    g = g.to(gpu).eval()
    lat = seeding.seeded_latents(N, g.n_latent, seed=6)
    return g, lat


def _frames(g, lat, noise, **kw):
    from maua_stylegan2_amd import render

    lo, hi = kw.get("frame_range") or (0, len(lat))
    out = np.zeros((hi - lo, SIZE, SIZE, 3), np.uint8)
    for first, u8 in render.synthesize(g, lat, noise, BATCH, **kw):
        out[first - lo: first - lo + u8.shape[0]] = u8.cpu().numpy()
    return out


def _close(a, b):
    diff = np.abs(a.astype(np.int16) - b.astype(np.int16))
    return diff.max() <= 1 and (diff > 0).mean() < 1e-2


def test_generator_random_noise_is_the_reference(gpu, small):
    g, _ = small
    maps = g.random_noise(2 ** 31 - 9, 3, SEED)
    assert len(maps) == g.num_layers and [tuple(m.shape) for m in maps] == [(3, 1, r, r) for r in RES[: g.num_layers]]
    for slot, m in enumerate(maps):
        ref = torch.from_numpy(pr.noise_maps(SEED, 2 ** 31 - 9, 3, slot, m.shape[-1] ** 2)).to(gpu)
        assert float((m.reshape(3, -1).double() - ref).abs().max()) <= TOL
    some = g.random_noise(5, 2, 77, slots=[4, 1])
    assert [tuple(m.shape) for m in some] == [(2, 1, 16, 16), (2, 1, 8, 8)]
    assert torch.equal(some[0], g.random_noise(0, 8, 77)[4][5:7])
    for bad in ([], [0, 0], [g.num_layers], [-1]):
        with pytest.raises(RuntimeError):
            g.random_noise(0, 1, 1, slots=bad)


@pytest.mark.parametrize("lanes", [1, 3])
def test_randomised_render_reads_the_generated_maps_on_the_graph_path(gpu, small, lanes, monkeypatch):
    """synthesize(randomize_noise=True) with noise_seed = S is bit-identical to synthesize(randomize_noise=False) fed the explicit sequences
    random_noise(0, n_frames, S): the captured route reads the generated maps and nothing else — and it IS the captured route."""
    from maua_stylegan2_amd.models import stylegan2

    g, lat = small
    replays = []
    original = stylegan2.GraphLane.replay
    monkeypatch.setattr(stylegan2.GraphLane, "replay", lambda self, frame0, stream=None: (replays.append((self.lane, frame0, self.random_slots)),
                                                                                          original(self, frame0, stream))[1])
    g.noise_seed = SEED
    try:
        randomised = _frames(g, lat, [None] * g.num_layers, randomize_noise=True, lanes=lanes)
    finally:
        g.noise_seed = None
    assert [(k, f) for k, f, _ in replays] == [(i % lanes, 8 * i) for i in range(3)]
    assert all(slots == tuple(range(g.num_layers)) for _, _, slots in replays)
    explicit = _frames(g, lat, g.random_noise(0, N, SEED), randomize_noise=False, lanes=lanes)
    assert np.array_equal(randomised, explicit)
    static = _frames(g, lat, [None] * g.num_layers, randomize_noise=False, lanes=lanes)
    assert not any(np.array_equal(randomised[i], static[i]) for i in range(N))  # the noise is really there
    assert len({randomised[i].tobytes() for i in range(N)}) == N


def test_shards_mixed_input_offsets_and_seeding(gpu, small):
    g, lat = small
    none = [None] * g.num_layers
    g.noise_seed = SEED
    try:
        whole = _frames(g, lat, none, randomize_noise=True)
        # frame_range shards: the bound of tests/test_world8_gpu.py for played ranks (a shard's tail batch runs at another batch size)
        a = _frames(g, lat, none, randomize_noise=True, frame_range=(0, 12))
        b = _frames(g, lat, none, randomize_noise=True, frame_range=(12, 24))
        assert np.array_equal(a[:8], whole[:8]) and _close(a, whole[:12]) and _close(b, whole[12:24])
        # a rank that was handed frames 12.. only (scattered sequences): noise_frame_offset names their place in the job
        g.noise_frame_offset = 12
        try:
            shifted = _frames(g, lat[12:24], none, randomize_noise=True)
        finally:
            g.noise_frame_offset = 0
        assert np.array_equal(shifted[:8], b[:8]) and _close(shifted, whole[12:24])
        # the eager path (no graph) generates the same maps
        eager = _frames(g, lat, none, randomize_noise=True, use_graph=False)
        assert np.array_equal(eager, whole)
        # mixed input: per-frame sequences for the low resolutions, generated maps above
        from maua_stylegan2_amd import seeding

        given = [torch.from_numpy(seeding.seeded_array(7, f"n{i}", (N, 1, r, r))) if r <= 16 else None for i, r in enumerate(RES[: g.num_layers])]
        holes = [i for i, nz in enumerate(given) if nz is None]
        mixed = _frames(g, lat, given, randomize_noise=True)
        filled = list(given)
        for i, nz in zip(holes, g.random_noise(0, N, SEED, slots=holes)):
            filled[i] = nz
        assert np.array_equal(mixed, _frames(g, lat, filled, randomize_noise=False))
        assert not np.array_equal(mixed, whole)
    finally:
        g.noise_seed = None
    # no seed set: one draw from torch's CPU generator per render
    first, second = _frames(g, lat, none, randomize_noise=True), _frames(g, lat, none, randomize_noise=True)
    assert not any(np.array_equal(first[i], second[i]) for i in range(N))
    torch.manual_seed(1234)
    first = _frames(g, lat, none, randomize_noise=True)
    torch.manual_seed(1234)
    assert np.array_equal(first, _frames(g, lat, none, randomize_noise=True))
    assert ctypes.sizeof(ctypes.c_void_p) == 8
