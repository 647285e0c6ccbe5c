"""GPU: synthesised noise slots (csrc/noise_synth.hip, maua_noise_synth_f32; ar.NoiseSynth) against a float64 numpy evaluation of the
definition in include/maua_hip.h, and through the generator, ``render.synthesize`` and ``generate()``.

    dst[b, e] = gain * sum_k env_k[f] * mask_k[e] * v_k,   v_k = bank_k[(F + phase_k) mod P_k, e]  or the counter-based map (tests/philox_ref.py)

Tolerance, derived from the arithmetic (not measured): the kernel rounds env * mask once per term, accumulates with one fused multiply-add
per term and rounds the product with the gain — n_terms + n_terms + 1 roundings, each at most 2^-24 of a quantity bounded by
S = sum_k |env mask v| — so  |err| <= (n_terms + 3) 2^-24 |gain| S  per element (the bound the issue states; first-order slack included).
A "randn" term is itself only an fp32 evaluation of the Philox / Box-Muller map: it adds RANDN_TOL |gain env mask|, RANDN_TOL = 4 x the
float32-vs-float64 error of tests/philox_ref.py on the very maps the case uses, the convention of tests/test_randnoise_gpu.py.
"""
import sys

import numpy as np
import pytest
import torch

import philox_ref as pr
from redzone import CANARY_BITS, Guard

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

EPS = 2.0 ** -24
N_FRAMES = 19
PERIODS = (1, 5, 7, N_FRAMES)
SEED = 0x1234567800000ABC  # above 2^32: both key words matter
SRC_DWORDS = 134  # sizeof(maua_frame_source_t) / 4
NOISE_DW, STRIDE_DW = 6, 6 + 64  # dword offsets of noise[] and noise_stride[] inside the struct


def _rng(*key):
    return np.random.default_rng([77, *key])


class Operands:
    """The banks, envelopes and masks of one map size on the device (uploaded once) with their float64 twins."""

    def __init__(self, dev, hw):
        self.hw = hw
        self.bank_np = {p: _rng(hw, p).standard_normal((p, hw)).astype(np.float32) for p in PERIODS}
        self.env_np = [(_rng(hw, 100 + k).random(N_FRAMES) * 1.5 - 0.25).astype(np.float32) for k in range(4)]
        self.mask_np = [_rng(hw, 200 + k).random(hw).astype(np.float32) for k in range(4)]
        up = lambda a: torch.from_numpy(a).to(dev)  # noqa: E731
        self.bank = {p: up(a) for p, a in self.bank_np.items()}
        self.env = [up(a) for a in self.env_np]
        self.mask = [up(a) for a in self.mask_np]
        # a mask 4 bytes off a 16-byte boundary: the whole sample then takes the element-by-element path even where hw % 4 == 0
        self._shifted = torch.zeros(hw + 4, dtype=torch.float32, device=dev)
        self._shifted[1: 1 + hw].copy_(self.mask[0])
        self.mask_off = self._shifted[1: 1 + hw]
        assert self.mask_off.data_ptr() % 16 == 4


def _entry(dst, hw, slot, gain, seed, terms):
    """terms: [(bank tensor or None = randn, envelope tensor or None, mask tensor or None, period, phase)]"""
    from maua_stylegan2_amd import _lib

    e = _lib.NoiseSynthSlot()
    e.dst, e.hw, e.slot, e.n_terms, e.gain, e.seed = (dst.data_ptr() if dst is not None else None), hw, slot, len(terms), gain, seed
    for k, (bank, env, mask, period, phase) in enumerate(terms):
        t = e.term[k]
        t.bank, t.envelope, t.mask = (None if x is None else x.data_ptr() for x in (bank, env, mask))
        t.period, t.phase = period, phase
    return e


def _table(g, entries):
    from maua_stylegan2_amd import _lib

    arr = (_lib.NoiseSynthSlot * len(entries))(*entries)
    return g.inp(np.frombuffer(bytes(arr), dtype=np.uint8).copy(), "table", torch.uint8)


def _reference(hw, batch, local0, frame0, slot, gain, seed, terms_np, randn_tol=0.0):
    """float64 maps [batch, hw] and the per-element tolerance.  terms_np: [(bank [P, hw] or None, env [n] or None, mask [hw] or None, P, phase)]"""
    out, mag, extra = np.zeros((batch, hw)), np.zeros((batch, hw)), np.zeros((batch, hw))
    for b in range(batch):
        f = local0 + b
        F = frame0 + f
        for bank, env, mask, period, phase in terms_np:
            v = pr.noise_map(seed, F, slot, hw) if bank is None else bank[(F + phase) % period].astype(np.float64)
            e = 1.0 if env is None else float(env[f])
            m = np.ones(hw) if mask is None else mask.astype(np.float64)
            out[b] += e * m * v
            mag[b] += np.abs(e * m * v)
            if bank is None:
                extra[b] += randn_tol * np.abs(gain * e * m)
    return gain * out, (len(terms_np) + 3) * EPS * abs(gain) * mag + extra


def _randn_tol(seed, frames, slot, hw):
    return 4 * max(float(np.abs(pr.noise_map(seed, f, slot, hw, np.float32).astype(np.float64) - pr.noise_map(seed, f, slot, hw)).max())
                   for f in frames)


def _assert_close(got, want, tol, what):
    err = np.abs(got.double().cpu().numpy() - want)
    over = err > tol
    assert not over.any(), (what, float(err.max()), float((err / np.maximum(tol, 1e-300)).max()))
    return float((err / np.maximum(tol, 1e-300)).max())


def _launch(dev, entries_of, batch, frame0, local0=None):
    """One launch.  entries_of(guard) -> ([entry], [names of the outputs written]); with ``local0`` through a frame source seeked there.
    Returns (guard, src words before, src view)."""
    from maua_stylegan2_amd import _lib

    lib = _lib.load()
    g = Guard(dev)
    entries, written = entries_of(g)
    table = _table(g, entries)
    st = _lib.stream_ptr(dev)
    src, before = None, None
    if local0 is not None:
        src = g.out((SRC_DWORDS,), "src", torch.int32)
        src.copy_(torch.arange(SRC_DWORDS, dtype=torch.int32) + 0x5A000000)  # recognisable words everywhere
        _lib.check(lib.maua_frame_source_seek(src.data_ptr(), local0, st), "seek")
        before = src.clone()
    rc = lib.maua_noise_synth_f32(table.data_ptr(), len(entries), batch, frame0, None if src is None else src.data_ptr(), st)
    assert rc == 0, rc
    g.check(written=written)
    return g, before, src


# ------------------------------------------------------------------------------------------------ 1. the entry at the edge shapes
@pytest.mark.parametrize("h,w", [(1, 3), (5, 7), (4, 8), (16, 16)])
def test_entry_matches_the_float64_reference_at_the_edge_shapes(gpu, h, w):
    """batch {1, 3, 8} x n_terms {1 (every period), 4 (periods 1, 5, 7, 19)} x phases {0, P - 1} x frame0 {0, n_frames - batch: the loops wrap
    inside the batch} x envelope / mask present / absent, gain != 1; (5, 7): hw = 35, every odd sample unaligned; plus a mask 4 bytes off a
    16-byte boundary and one case with a "randn" term and a seed above 2^32.  Red zones around every output and the table."""
    hw = h * w
    ops = Operands(gpu, hw)
    gain = -1.75
    worst, cases = 0.0, 0

    def run(batch, frame0, spec, seed=0, slot=0, mask_off=False, what=None):
        """spec: [(period or None = randn, phase, with_env, with_mask)]"""
        nonlocal worst, cases
        dev_terms, np_terms = [], []
        for k, (period, phase, with_env, with_mask) in enumerate(spec):
            mask_t, mask_n = (ops.mask_off, ops.mask_np[0]) if mask_off and with_mask else (ops.mask[k], ops.mask_np[k])
            dev_terms.append((None if period is None else ops.bank[period], ops.env[k] if with_env else None, mask_t if with_mask else None,
                              period or 1, phase))
            np_terms.append((None if period is None else ops.bank_np[period], ops.env_np[k] if with_env else None,
                             mask_n if with_mask else None, period or 1, phase))
        box = {}

        def entries_of(g):
            box["dst"] = g.out((batch, hw), "dst")
            return [_entry(box["dst"], hw, slot, gain, seed, dev_terms)], ["dst"]

        # src == NULL: the local frame is b, so the envelopes are read from their start and frame0 only moves loops and counter
        _launch(gpu, entries_of, batch, frame0)
        tol_r = _randn_tol(seed, range(frame0, frame0 + batch), slot, hw) if any(p is None for p, *_ in spec) else 0.0
        want, tol = _reference(hw, batch, 0, frame0, slot, gain, seed, np_terms, tol_r)
        worst = max(worst, _assert_close(box["dst"], want, tol, what or (h, w, batch, frame0, spec)))
        cases += 1

    for batch in (1, 3, 8):
        for frame0 in (0, N_FRAMES - batch):
            for with_env in (False, True):
                for with_mask in (False, True):
                    for period in PERIODS:  # one term, every period, both phases
                        for phase in (0, period - 1):
                            run(batch, frame0, [(period, phase, with_env, with_mask)])
                    for last in (False, True):  # four terms: phases all 0 / all P - 1
                        run(batch, frame0, [(p, (p - 1) if last else 0, with_env, with_mask) for p in PERIODS])
            # a mask off the 16-byte grid, and mixed presence across the terms
            run(batch, frame0, [(5, 4, True, True), (7, 0, False, False)], mask_off=True)
            run(batch, frame0, [(7, 6, True, False), (1, 0, False, True), (N_FRAMES, 18, True, True)])
    # the counter-based term, seed above 2^32, next to a loop; alone; behind an envelope and a mask
    run(8, N_FRAMES - 8, [(5, 3, True, False), (None, 0, True, True)], seed=SEED, slot=11)
    run(3, 2 ** 31 - 9, [(None, 0, False, False)], seed=SEED, slot=2)
    print(f"[{h} x {w}] {cases} launches, worst |err| / tolerance {worst:.3f}")


# ------------------------------------------------------------------------------------------------ 2. one launch, several slots
def test_one_launch_fills_several_slots_and_skips_the_empty_entry(gpu):
    """hw 35, 32, (empty), 3, 256 in one table, batch 3, frames 15 .. 17 (the 5- and 7-frame loops wrap): every destination matches its
    reference, nothing is written outside [batch, hw], every element inside is, and the empty entry's destination keeps its canary."""
    batch, frame0, gain = 3, 15, 0.5
    sizes = [35, 32, None, 3, 256]
    ops = {hw: Operands(gpu, hw) for hw in sizes if hw}
    spec = {35: [(5, 3, True, True), (7, 6, False, False)], 32: [(7, 0, True, False)], 3: [(1, 0, False, True), (5, 4, True, False), (None, 0, True, False)],
            256: [(N_FRAMES, 18, True, True), (5, 0, False, False), (7, 2, True, False), (1, 0, False, True)]}
    dsts = {}

    def terms(hw, numpy):
        o = ops[hw]
        pick = (lambda d, n: n) if numpy else (lambda d, n: d)
        return [(None if p is None else pick(o.bank[p], o.bank_np[p]), pick(o.env[k], o.env_np[k]) if we else None,
                 pick(o.mask[k], o.mask_np[k]) if wm else None, p or 1, ph) for k, (p, ph, we, wm) in enumerate(spec[hw])]

    def entries_of(g):
        entries = []
        for slot, hw in enumerate(sizes):
            if hw is None:
                dsts["empty"] = g.out((batch, 64), "empty")
                entries.append(_entry(dsts["empty"], 64, slot, 1.0, 0, []))  # n_terms = 0 with a valid destination
            else:
                dsts[hw] = g.out((batch, hw), f"dst{hw}")
                entries.append(_entry(dsts[hw], hw, slot, gain, SEED, terms(hw, False)))
        return entries, [f"dst{hw}" for hw in sizes if hw]

    g, _, _ = _launch(gpu, entries_of, batch, frame0)
    assert g.untouched("empty") and bool((dsts["empty"].view(torch.int32) == CANARY_BITS).all())
    for slot, hw in enumerate(sizes):
        if hw:
            tol_r = _randn_tol(SEED, range(frame0, frame0 + batch), slot, hw)
            want, tol = _reference(hw, batch, 0, frame0, slot, gain, SEED, terms(hw, True), tol_r)
            _assert_close(dsts[hw], want, tol, hw)


# ------------------------------------------------------------------------------------------------ 3. the frame-source form
@pytest.mark.parametrize("frame0", [0, 4])
def test_frame_source_form_reads_the_frame_and_rewires_the_slots(gpu, frame0):
    """A frame source seeked to frame 6: the launch makes the maps of local frames 6 .. 6 + batch - 1 (envelope index; loops and counter
    at ``frame0`` + that) and leaves noise[slot] + (6 + b) * stride pointing at dst + b * hw; no other word of the struct changes."""
    batch, local0, gain = 3, 6, 1.25
    layout = [(2, 35), (9, 256)]  # (slot, hw)
    ops = {hw: Operands(gpu, hw) for _, hw in layout}
    spec = {35: [(7, 6, True, True), (None, 0, True, False)], 256: [(5, 1, True, False), (N_FRAMES, 0, False, True)]}
    dsts = {}

    def terms(hw, numpy):
        o = ops[hw]
        pick = (lambda d, n: n) if numpy else (lambda d, n: d)
        return [(None if p is None else pick(o.bank[p], o.bank_np[p]), pick(o.env[k], o.env_np[k]) if we else None,
                 pick(o.mask[k], o.mask_np[k]) if wm else None, p or 1, ph) for k, (p, ph, we, wm) in enumerate(spec[hw])]

    def entries_of(g):
        entries = []
        for slot, hw in layout:
            dsts[hw] = g.out((batch, hw), f"dst{hw}")
            entries.append(_entry(dsts[hw], hw, slot, gain, SEED, terms(hw, False)))
        return entries, [f"dst{hw}" for _, hw in layout]

    _, before, src = _launch(gpu, entries_of, batch, frame0, local0=local0)
    for slot, hw in layout:
        tol_r = _randn_tol(SEED, range(frame0 + local0, frame0 + local0 + batch), slot, hw)
        want, tol = _reference(hw, batch, local0, frame0, slot, gain, SEED, terms(hw, True), tol_r)
        _assert_close(dsts[hw], want, tol, (slot, hw))
    after, was = src.cpu().numpy().copy(), before.cpu().numpy()
    assert after[0] == local0
    for slot, hw in layout:
        ptr = int(after[NOISE_DW + 2 * slot: NOISE_DW + 2 * slot + 2].view(np.uint64)[0])
        stride = int(after[STRIDE_DW + 2 * slot: STRIDE_DW + 2 * slot + 2].view(np.int64)[0])
        assert stride == hw
        for b in range(batch):  # what a layer computes: noise[slot] + (src->frame0 + b) * stride
            assert (ptr + (local0 + b) * stride * 4) % 2 ** 64 == dsts[hw].data_ptr() + b * hw * 4
        after[NOISE_DW + 2 * slot: NOISE_DW + 2 * slot + 2] = was[NOISE_DW + 2 * slot: NOISE_DW + 2 * slot + 2]
        after[STRIDE_DW + 2 * slot: STRIDE_DW + 2 * slot + 2] = was[STRIDE_DW + 2 * slot: STRIDE_DW + 2 * slot + 2]
    assert np.array_equal(after, was), "words of the frame source outside the synthesised slots changed"


# ------------------------------------------------------------------------------------------------ 4 / 5. generator and render
SIZE, N, BATCH = 64, 19, 4  # render: four graph batches + an eager tail of three
RES = [4] + [r for k in range(3, 7) for r in (2 ** k, 2 ** k)]  # the nine noise layers of a 64^2 generator


@pytest.fixture(scope="module")
def small(gpu):
    from maua_stylegan2_amd import seeding
    from maua_stylegan2_amd.models.stylegan2 import Generator

    g = Generator(SIZE, 512, 8, channel_multiplier=2, constant_input=True)
    g.load_state_dict(seeding.seeded_state_dict(SIZE, seed=5, rgb_gain=seeding.unsaturated_rgb_gain(SIZE)), strict=True)
    g = g.to(gpu).eval()
    assert g.num_layers == len(RES)
    return g, seeding.seeded_latents(N, g.n_latent, seed=6).to(gpu)


def _recipe(gpu, slot, tag, randn=False, gain=0.7):
    """A recipe for noise slot ``slot`` of the small generator: a 5-frame and a 7-frame loop behind two envelopes and a mask (+ a seeded
    "randn" term), of unit order like the checkpoint's buffers."""
    import maua_stylegan2_amd.audioreactive as ar

    r = RES[slot]
    rng = _rng(slot, tag)
    t = lambda *shape: torch.from_numpy(rng.standard_normal(shape).astype(np.float32)).to(gpu)  # noqa: E731
    u = lambda *shape: torch.from_numpy(rng.random(shape).astype(np.float32)).to(gpu)  # noqa: E731
    terms = [ar.noise_term(t(5, 1, r, r), envelope=u(N), phase=3), ar.noise_term(t(7, r, r), envelope=u(N), mask=u(r, r), phase=6)]
    if randn:
        terms.append(ar.noise_term("randn", envelope=u(N)))
    return ar.NoiseSynth(r, r, terms, gain=gain, seed=SEED)


def test_recipe_frames_match_the_reference_and_do_not_depend_on_the_batch(gpu):
    """ar.NoiseSynth.frames / materialize / window / std on the device: the float64 formula, bit-identical whatever the batch."""
    r = _recipe(gpu, 4, 0, randn=True)  # 16 x 16
    hw = 256
    whole = r.materialize(slot=4)
    assert tuple(whole.shape) == (N, 1, 16, 16) and r.shape == (N, 1, 16, 16)
    np_terms = [(None if b is None else b.cpu().numpy(), e.cpu().numpy(), None if m is None else m.cpu().numpy(), p, ph) for b, e, m, p, ph in r._terms]
    want, tol = _reference(hw, N, 0, 0, 4, r.gain, r.seed, np_terms, _randn_tol(SEED, range(N), 4, hw))
    _assert_close(whole.reshape(N, hw), want, tol, "materialize")
    for batch in (1, 3, 8):
        parts = torch.cat([r.frames(f, min(batch, N - f), 4) for f in range(0, N, batch)])
        assert torch.equal(parts.view(torch.int32), whole.view(torch.int32))
    assert torch.equal(r.window(11, 19).materialize(slot=4), whole[11:19])
    assert torch.equal(r.window(11, 19).window(2, 6).frames(1, 2, 4), whole[14:16])
    picks = sorted({(2 * j + 1) * N // 32 for j in range(16)})
    assert abs(float(r.std()) - float(torch.cat([r.frames(f, 1) for f in picks]).std())) == 0.0
    assert abs(float(r.std()) - float(whole.std())) < 0.25 * float(whole.std())  # a bounded sample, not the exact amplitude
    with pytest.raises(ValueError):
        r.frames(17, 3)


def test_captured_forward_synthesises_the_bound_recipes(gpu, small, monkeypatch):
    """Recipes on slots 2 and 8, a per-frame tensor on slot 5: capture_graph(batch 3, synth_slots) + bind + replay(n) is BIT-equal to the
    eager forward fed with recipe.frames(n, 3); other recipes are bound to the same cached lane without a new capture; a recipe in a slot the
    lane was not captured for, a tensor or None in a synth slot, a wrong map size or envelope length are errors."""
    from maua_stylegan2_amd import render, seeding

    g, lat = small
    given = torch.from_numpy(seeding.seeded_array(7, "n5", (N, 1, 32, 32))).to(gpu)
    first = {2: _recipe(gpu, 2, 0), 8: _recipe(gpu, 8, 0, randn=True)}
    second = {2: _recipe(gpu, 2, 1, randn=True), 8: _recipe(gpu, 8, 1)}

    def noise_list(recipes):
        noise = [None] * g.num_layers
        noise[5] = given
        for i, r in recipes.items():
            noise[i] = r
        return noise

    def eager(recipes, n, b):
        noise = noise_list(recipes)
        noise[5] = given[n: n + b]
        for i, r in recipes.items():
            noise[i] = r.frames(n, b, i)
        image, _ = g(styles=lat[n: n + b], noise=noise, input_is_latent=True, randomize_noise=False)
        return image

    stream = torch.cuda.Stream(gpu)
    with torch.cuda.stream(stream):
        lane = g.capture_graph(3, lane=1, synth_slots=(2, 8))
        assert lane.synth_slots == (2, 8) and lane.synth_frame_offset == 0
        lane.bind(lat, noise_list(first))
        for n in (0, 5, 16):  # 5 .. 7 and 16 .. 18: both loops wrap inside the batch
            lane.replay(n)
            stream.synchronize()
            got = lane.image.clone()
            want = eager(first, n, 3)
            assert torch.equal(got.view(torch.int32), want.view(torch.int32)), n
        lane.replay(5)
        stream.synchronize()
        with_first = lane.image.clone()
        lane.bind(lat, noise_list(second))  # the same captured graph, another render's recipes
        lane.replay(5)
        stream.synchronize()
        assert torch.equal(lane.image.view(torch.int32), eager(second, 5, 3).view(torch.int32))
        assert not torch.equal(lane.image, with_first)
        static, _ = g(styles=lat[5:8], noise=[None] * 5 + [given[5:8]] + [None] * 3, input_is_latent=True, randomize_noise=False)
        assert not torch.equal(with_first, static)  # the recipes are really in the image
        # what bind refuses
        for bad in ({**first, 3: _recipe(gpu, 3, 0)}, {2: first[2]}, {2: first[2], 8: _recipe(gpu, 6, 0)}):
            with pytest.raises(RuntimeError):
                lane.bind(lat, noise_list(bad))
        tensor_in_synth_slot = noise_list(first)
        tensor_in_synth_slot[2] = torch.zeros(N, 1, 8, 8, device=gpu)
        with pytest.raises(RuntimeError, match="NoiseSynth"):
            lane.bind(lat, tensor_in_synth_slot)
        with pytest.raises(RuntimeError, match="frames"):
            lane.bind(lat[:10], noise_list(first))  # envelopes of 19 frames, a render of 10
        with pytest.raises(RuntimeError, match="offset"):
            lane.bind(lat[:8], noise_list({i: r.window(11, 19) for i, r in first.items()}))
        with pytest.raises(RuntimeError):
            g.capture_graph(3, lane=1, random_slots=(2,), synth_slots=(2, 8))
        lane.release()
    stream.synchronize()
    # render.graph_lanes: cached per synth slot set; the second render's recipes reuse the captured lane
    captures = []
    original = g.capture_graph
    monkeypatch.setattr(g, "capture_graph", lambda *a, **k: (captures.append(k.get("synth_slots")), original(*a, **k))[1])
    (s1, lane1), = render.graph_lanes(g, 3, 1, synth=((2, 8), 0))
    (s2, lane2), = render.graph_lanes(g, 3, 1, synth=((2, 8), 0))
    (_, plain), = render.graph_lanes(g, 3, 1)
    assert lane1 is lane2 and plain is not lane1 and captures == [(2, 8), None] and plain.synth_slots == ()
    frames = {}
    for tag, recipes in (("first", first), ("second", second)):
        with torch.cuda.stream(s1):
            lane1.bind(lat, noise_list(recipes))
            lane1.replay(16)
            s1.synchronize()
            frames[tag] = lane1.u8.clone()
            assert torch.equal(frames[tag], render.frames_to_uint8(eager(recipes, 16, 3))), tag
            lane1.release()
    assert not torch.equal(frames["first"], frames["second"]) and len(captures) == 2


def _frames(g, lat, noise, **kw):
    from maua_stylegan2_amd import render

    out = np.zeros((len(lat), SIZE, SIZE, 3), np.uint8)
    for first, u8 in render.synthesize(g, lat, noise, BATCH, **kw):
        out[first: first + u8.shape[0]] = u8.cpu().numpy()
    return out


def test_synthesize_graph_eager_and_windows_agree(gpu, small, monkeypatch):
    """19 frames at batch 4: four graph batches + an eager tail of three are identical to the all-eager render, and the windows [0, 8) and
    [8, 19) rendered separately (the second: its own lanes, frame offset 8) equal the full render frame for frame."""
    from maua_stylegan2_amd.models import stylegan2

    g, lat = small
    replays = []
    original = stylegan2.GraphLane.replay
    monkeypatch.setattr(stylegan2.GraphLane, "replay", lambda self, frame0, stream=None: (replays.append((frame0, self.synth_slots, self.synth_frame_offset)),
                                                                                          original(self, frame0, stream))[1])
    noise = [None] * g.num_layers
    noise[3], noise[8] = _recipe(gpu, 3, 2, randn=True), _recipe(gpu, 8, 2)
    whole = _frames(g, lat, noise)
    assert replays == [(n, (3, 8), 0) for n in (0, 4, 8, 12)]
    assert np.array_equal(whole, _frames(g, lat, noise, use_graph=False)) and len(replays) == 4
    assert len({whole[i].tobytes() for i in range(N)}) == N
    assert not np.array_equal(whole, _frames(g, lat, [None] * g.num_layers))
    del replays[:]
    cut = lambda lo, hi: [nz if nz is None else nz.window(lo, hi) for nz in noise]  # noqa: E731
    a, b = _frames(g, lat[:8], cut(0, 8)), _frames(g, lat[8:], cut(8, N))
    assert replays == [(0, (3, 8), 0), (4, (3, 8), 0), (0, (3, 8), 8), (4, (3, 8), 8)]
    assert np.array_equal(np.concatenate([a, b]), whole)
    with pytest.raises(RuntimeError, match="frame offset"):
        _frames(g, lat[:8], [None, noise[3].window(0, 8)] + [None] * 6 + [noise[8].window(8, 16)])


# ------------------------------------------------------------------------------------------------ 6. generate() with the example plugin
def test_generate_with_the_hires_plugin_synthesises_every_scale_on_the_lanes(gpu, tmp_path, monkeypatch):
    """``generate()`` with examples/hires_noise.py on stand-in audio features, on the seeded 512^2 generator (the smallest size ``render``
    delivers): no noise scale is None, the two 512^2 scales are recipes, the full batches come from graph lanes that synthesise them — and
    the same job under a process group of one rank (broadcast recipes, ``window``, gathered frames) delivers the same frames."""
    from conftest import GOLDEN

    import maua_stylegan2_amd.audioreactive as ar
    from maua_stylegan2_amd import generate_audiovisual as gav
    from maua_stylegan2_amd import render, seeding
    from maua_stylegan2_amd.audioreactive.examples import hires_noise
    from maua_stylegan2_amd.models import stylegan2
    from played_world import PlayedWorld

    if GOLDEN not in sys.path:
        sys.path.insert(0, GOLDEN)
    import plugin_stubs as stubs

    monkeypatch.chdir(tmp_path)
    size, n, fps, batch = 512, 10, 5, 4
    torch.save({"g_ema": seeding.seeded_state_dict(size, seed=0)}, "seeded512.pt")
    np.save("selection.npy", seeding.seeded_array(42, "selection", (12, 16, 512)))
    feats = stubs.Features(n, fps)
    monkeypatch.setattr(ar, "onsets", feats.onsets)
    monkeypatch.setattr(ar, "chroma", feats.chroma)
    monkeypatch.setattr(ar, "load_audio", feats.load_audio)
    monkeypatch.setenv("MAUA_GENERATOR_CACHE", "0")
    delivered, seen, replays = [], [], []

    class KeepingSink(render.FrameSink):
        def __init__(self, output_file, width, height, *a, **k):
            self.count, self.w, self.h = 0, width, height

        def write(self, frame):
            delivered.append(np.array(frame, copy=True))
            self.count += 1

        def close(self):
            pass

    monkeypatch.setattr(render, "FrameSink", KeepingSink)
    original = stylegan2.GraphLane.replay
    monkeypatch.setattr(stylegan2.GraphLane, "replay", lambda self, frame0, stream=None: (replays.append((frame0, self.synth_slots)),
                                                                                          original(self, frame0, stream))[1])

    def get_noise(height, width, scale, num_scales, args):
        nz = hires_noise.get_noise(height, width, scale, num_scales, args)
        seen.append(nz)
        return nz

    def job():
        del delivered[:], seen[:], replays[:]
        monkeypatch.setattr(torch, "randn", stubs.SeededRandn(47))
        torch.manual_seed(3)
        gav.generate(ckpt="seeded512.pt", audio_file="clip.wav", initialize=hires_noise.initialize, get_latents=hires_noise.get_latents,
                     get_noise=get_noise, latent_file="selection.npy", G_res=size, out_size=size, fps=fps, batch=batch,
                     output_file=str(tmp_path / "o.mp4"))
        torch.cuda.synchronize()
        return np.stack(delivered), list(seen), list(replays)

    frames, noise, played = job()
    assert frames.shape == (n, size, size, 3) and frames.std() > 5
    assert len(noise) == 15 and all(nz is not None for nz in noise)
    kinds = [isinstance(nz, ar.NoiseSynth) for nz in noise]
    assert kinds == [False] * 13 + [True] * 2 and all(nz.shape == (n, 1, size, size) and nz.offset == 0 for nz in noise[13:])
    assert played == [(0, (13, 14)), (4, (13, 14))]  # two full batches on the lanes; the tail of two is eager
    assert abs(float(noise[14].std()) - 1 / 2.5) < 0.1  # the plugin's normalisation, from the sampled amplitude
    world = PlayedWorld(1)
    with world.playing(0):
        grouped, noise_g, played_g = job()
    assert world.stats["broadcast"] > 0 and world.stats["gather"] > 0
    assert played_g == played and [isinstance(nz, ar.NoiseSynth) for nz in noise_g] == kinds
    assert np.array_equal(grouped, frames)
