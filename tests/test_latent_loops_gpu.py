"""GPU: looping latent sequences on the device (audioreactive/latent.py spline_loops / slerp_loops on a CUDA selection, loop_sections;
csrc/latent_loops.hip maua_keyframe_blend_f32) — parity with the host paths the goldens pin to the reference, sectioned == per-section
bit for bit, the kernel's edge shapes through the C ABI between red zones, and the sections example plugin through generate().

Error bound of a blended frame (spline parity and the ABI cases): the device evaluates sum_i W[f, i] key_i as a chain of m fp32 fused
multiply-adds on fp32 weights, so |error| <= (2^-24 per rounded weight + 2^-24 per chain step, m steps) * sum_i |W[f, i]| max|key|
<= (m + 1) 2^-24 sum_i |W[f, i]| max|key|; the tests allow 4 (m + 2) 2^-24 sum_i |W[f, i]| max|key| per frame, with W in float64 from
scipy (or the test's own table), never from the code under test.  About 1e-5 for the golden selection."""
import numpy as np
import pytest
import torch
from scipy import interpolate

import segment_ref as ref
from redzone import Guard

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
SR = 22050
EPS = 2.0 ** -24


def _unit_fit_weights(m, period):
    """W [period, m] float64: column i is the spline through the i-th unit vector (scipy, in the test)."""
    x, knots = np.linspace(0, 1, period), np.linspace(0, 1, m)
    return np.stack([interpolate.splev(x, interpolate.splrep(knots, unit)) for unit in np.eye(m)], axis=1)


def _check_spline(sel, n_frames, n_loops, loop, gpu):
    from maua_stylegan2_amd.audioreactive import latent

    want = latent.spline_loops(sel, n_frames, n_loops, loop)  # host float64 path (golden: 1e-9 of the reference)
    got = latent.spline_loops(torch.from_numpy(sel).to(gpu), n_frames, n_loops, loop)
    assert got.is_cuda and got.dtype == torch.float32 and got.shape == want.shape and want.dtype == torch.float64
    m = len(sel) + (1 if loop else 0)
    period = int(n_frames // max(1, n_loops))
    w = _unit_fit_weights(m, period)
    rows = np.arange(n_frames) % period
    bound = 4 * (m + 2) * EPS * np.abs(w).sum(1)[rows] * float(np.abs(sel).max())
    err = (got.double().cpu() - want).abs().reshape(n_frames, -1).max(1).values.numpy()
    print(f"spline m={m} P={period} n={n_frames}: max err {err.max():.3g}, smallest bound {bound.min():.3g}")
    assert bool(torch.isfinite(got).all()) and (err <= bound).all(), (err.max(), bound.min())
    return got


def test_spline_loops_on_the_golden_selection(gpu, golden):
    g = golden("audioreactive_torch.npz")
    _check_spline(g["spline.sel"], 37, 2, True, gpu)


def test_spline_loops_open_with_four_keys(gpu):
    sel = np.random.default_rng(4).standard_normal((4, 3, 10)).astype(np.float32)
    _check_spline(sel, 23, 1, False, gpu)


def test_spline_loops_full_size_selection(gpu):
    sel = np.random.default_rng(12).standard_normal((12, 18, 512)).astype(np.float32)
    _check_spline(sel, 1000, 3, True, gpu)


def test_slerp_loops_on_the_golden_configurations(gpu, golden):
    from maua_stylegan2_amd.audioreactive import latent, signal as sig

    g = golden("latent_utils.npz")
    sig.set_SMF(1)
    sel = torch.from_numpy(g["slerp_loops.sel"]).to(gpu)
    for tag in "abc":
        n_frames, n_loops, smoothing, loop = (int(v) for v in g[f"slerp_loops.{tag}.cfg"])
        y = latent.slerp_loops(sel, n_frames, n_loops, smoothing, bool(loop))
        assert y.is_cuda and list(y.shape) == g[f"slerp_loops.{tag}.shape"].tolist() and y.dtype == torch.float32
        err = np.abs(y.cpu().numpy()[:, ::6, :] - g[f"slerp_loops.{tag}.y"]).max()
        print(f"slerp {tag}: max err {err:.3g}")
        np.testing.assert_allclose(y.cpu().numpy()[:, ::6, :], g[f"slerp_loops.{tag}.y"], atol=1e-5, err_msg=tag)
        assert torch.equal(y, y[:, :1].expand_as(y))  # layer 0 repeated over the layers


def test_slerp_loops_between_identical_keys(gpu):
    from maua_stylegan2_amd.audioreactive import latent, signal as sig

    sig.set_SMF(1)
    key = torch.from_numpy(np.random.default_rng(2).standard_normal((1, 3, 64)).astype(np.float32) * 2.0)
    y = latent.slerp_loops(key.repeat(2, 1, 1).to(gpu), 24, 1, 1, True)
    assert y.shape == (24, 3, 64) and bool(torch.isfinite(y).all())
    assert float((y.cpu() - key[:, :1]).abs().max()) <= 1e-5  # (a slerp loop moves layer 0 and repeats it over the layers)


def _sectioned_equals_per_section(gpu, sel, frames, key_starts, n_keys, n_loops, pad, kind, loop):
    from maua_stylegan2_amd.audioreactive import latent

    sel = sel.to(gpu)
    one = latent.spline_loops if kind == "spline" else (lambda s, n, k, loop: latent.slerp_loops(s, n, k, 1, loop))
    parts = [one(latent.wrapping_slice(sel, start, n_keys), n, k, loop=loop) for n, start, k in zip(frames, key_starts, n_loops) if n]
    parts.append(parts[-1][-1:].expand(pad, *sel.shape[1:]))
    want = torch.cat(parts)
    got = latent.loop_sections(sel.cpu(), frames, key_starts, n_keys, n_loops, n_frames=sum(frames) + pad, kind=kind, loop=loop)
    assert got.is_cuda and got.dtype == torch.float32 and got.shape == want.shape
    assert bool(torch.isfinite(got).all()) and torch.equal(got, want)
    assert torch.equal(latent.loop_sections(sel, frames, key_starts, n_keys, n_loops, kind=kind, loop=loop), want[: sum(frames)])


def test_loop_sections_equals_the_per_section_calls(gpu):
    sel = torch.from_numpy(np.random.default_rng(6).standard_normal((6, 3, 40)).astype(np.float32))
    _sectioned_equals_per_section(gpu, sel, [1, 2, 0, 5, 40], [5, 3, 0, 4, 2], 4, [1, 1, 1, 2.5, 1.5], 3, "spline", True)


def test_loop_sections_slerp_equals_the_per_section_calls(gpu):
    """A slerp section needs one frame per leg, so the 1- and 2-frame sections exist only for a single key without the closure (one leg);
    the same section lengths scaled to whole legs run with four keys and the closure as well."""
    from maua_stylegan2_amd.audioreactive import signal as sig

    sig.set_SMF(1)
    sel = torch.from_numpy(np.random.default_rng(7).standard_normal((6, 3, 40)).astype(np.float32))
    _sectioned_equals_per_section(gpu, sel, [1, 2, 0, 5, 40], [5, 3, 0, 4, 2], 1, [1, 1, 1, 2.5, 1.5], 3, "slerp", False)
    _sectioned_equals_per_section(gpu, sel, [5, 10, 0, 25, 40], [5, 3, 0, 4, 2], 4, [1, 1, 1, 2.5, 1.5], 3, "slerp", True)


# ------------------------------------------------------------------------------------------------ the kernel through the C ABI
N_BANK, N_SECTIONS, N_ROWS = 9, 3, 11
MAX_KEYS = 32  # MAUA_LOOP_MAX_KEYS


def _tables(feats, n_frames, keys, seed):
    rng = np.random.default_rng(seed)
    bank = (rng.standard_normal((N_BANK, feats)) * 3.0).astype(np.float32)
    key_idx = rng.integers(0, N_BANK, (N_SECTIONS, keys)).astype(np.int32)
    weights = rng.standard_normal((N_ROWS, keys)).astype(np.float32)
    weights[rng.random((N_ROWS, keys)) < 0.2] = 0.0  # unused columns are exact zeros
    row = rng.integers(0, N_ROWS, n_frames).astype(np.int32)
    sec = rng.integers(0, N_SECTIONS, n_frames).astype(np.int32)
    return bank, key_idx, weights, row, sec


def _launch(lib, bank, key_idx, weights, row, sec, out, feats, n_frames, keys):
    return lib.maua_keyframe_blend_f32(bank.data_ptr(), N_BANK, feats, key_idx.data_ptr(), weights.data_ptr(), row.data_ptr(), sec.data_ptr(),
                                       out.data_ptr(), n_frames, N_SECTIONS, N_ROWS, keys, torch.cuda.current_stream().cuda_stream)


def _guarded(gpu, tables, feats, n_frames, keys, offset=0):
    """Every buffer between red zones; ``offset`` floats in front of bank and out inside their windows (1: 16-byte misaligned)."""
    from maua_stylegan2_amd import _lib

    bank, key_idx, weights, row, sec = tables
    g = Guard(gpu)
    bank_d = g.inp(np.concatenate([np.zeros(offset, np.float32), bank.reshape(-1)]), "bank")[offset:]
    out_w = g.out((offset + n_frames * feats,), "out")
    out_w[:offset] = 0.0
    out_d = out_w[offset:]
    args = (bank_d, g.inp(key_idx, "key_idx", torch.int32), g.inp(weights, "weights"), g.inp(row, "row", torch.int32),
            g.inp(sec, "sec", torch.int32), out_d)
    assert bank_d.data_ptr() % 16 == 4 * offset % 16 and out_d.data_ptr() % 16 == 4 * offset % 16
    rc = _launch(_lib.load(), *args, feats, n_frames, keys)
    return g, rc, out_d.view(n_frames, feats), args


def _reference(gpu, tables):
    """float64 restatement and the per-frame bound, on the device."""
    bank, key_idx, weights, row, sec = (torch.from_numpy(t).to(gpu) for t in tables)
    w, idx = weights.double()[row.long()], key_idx.long()[sec.long()]  # [n_frames, keys]
    want = torch.zeros((len(row), bank.shape[1]), dtype=torch.float64, device=gpu)
    for i in range(w.shape[1]):
        want += w[:, i, None] * bank.double()[idx[:, i]]
    bound = 4 * (w.shape[1] + 2) * EPS * w.abs().sum(1) * float(bank.abs().max())
    return want, bound


@pytest.mark.parametrize("feats", [1, 3, 60, 513, 9216])
def test_kernel_edge_shapes_between_red_zones(gpu, feats):
    for n_frames in (1, 7, 300):
        for keys in (1, 4, 5, 13, MAX_KEYS):
            tables = _tables(feats, n_frames, keys, seed=feats + 31 * n_frames + keys)
            g, rc, out, _ = _guarded(gpu, tables, feats, n_frames, keys)
            assert rc == 0, (feats, n_frames, keys, rc)
            g.check(written=("out",))
            want, bound = _reference(gpu, tables)
            err = (out.double() - want).abs().max(1).values
            assert bool((err <= bound).all()), (feats, n_frames, keys, float(err.max()), float(bound.min()))


@pytest.mark.parametrize("feats", [60, 9216])
def test_unaligned_buffers_give_the_aligned_bits(gpu, feats):
    """feats % 4 == 0 with bank and out one float off 16-byte alignment: the element path, bit-identical to the 16-byte path."""
    n_frames, keys = 7, 5
    tables = _tables(feats, n_frames, keys, seed=feats)
    g0, rc0, aligned, _ = _guarded(gpu, tables, feats, n_frames, keys)
    g1, rc1, shifted, _ = _guarded(gpu, tables, feats, n_frames, keys, offset=1)
    assert rc0 == 0 and rc1 == 0
    g0.check(written=("out",))
    g1.check(written=("out",))
    want, bound = _reference(gpu, tables)
    assert bool(((shifted.double() - want).abs().max(1).values <= bound).all())
    assert torch.equal(aligned, shifted)


def test_a_frame_does_not_depend_on_the_tables_around_it(gpu):
    """The same weight row and keys inside a wider table (more zero columns, other sections and rows, another frame count) give the same
    bits: what loop_sections == per-section calls rests on."""
    feats, keys = 513, 5
    bank, key_idx, weights, row, sec = _tables(feats, 7, keys, seed=99)
    _, rc, narrow, _ = _guarded(gpu, (bank, key_idx, weights, row, sec), feats, 7, keys)
    wide_idx = np.concatenate([key_idx, np.full((N_SECTIONS, 8), N_BANK - 1, np.int32)], axis=1)
    wide_w = np.concatenate([weights, np.zeros((N_ROWS, 8), np.float32)], axis=1)
    order = np.arange(7)[::-1].copy()  # the frames in another order, between frames of other rows
    row2, sec2 = np.zeros(300, np.int32), np.zeros(300, np.int32)
    row2[40 * np.arange(7)], sec2[40 * np.arange(7)] = row[order], sec[order]
    _, rc2, wide, _ = _guarded(gpu, (bank, wide_idx, wide_w, row2, sec2), feats, 300, keys + 8)
    assert rc == 0 and rc2 == 0
    assert torch.equal(wide[40 * np.arange(7)], narrow[torch.from_numpy(order).to(gpu)])


def test_refused_calls_leave_the_output_untouched(gpu):
    from maua_stylegan2_amd import _lib

    tables = _tables(60, 7, 5, seed=1)
    g, rc, _, args = _guarded(gpu, tables, 60, 7, 5)
    assert rc == 0
    lib = _lib.load()
    g2 = Guard(gpu)
    out = g2.out((7 * 60,), "out")
    assert _launch(lib, *args[:5], out, 60, 7, MAX_KEYS + 1) == -22
    assert _launch(lib, *args[:5], out, 0, 7, 5) == -22
    assert _launch(lib, *args[:5], out, 60, 0, 5) == 0  # no frames: a successful no-op
    assert g2.untouched("out")
    g2.check()
    g.check(written=("out",))


def test_sections_plugin_generates(gpu, tmp_path, monkeypatch):
    """audioreactive/examples/sections.py through generate() on the sectioned click-track fixture, as the kelp-style plugin test runs."""
    import scipy.io.wavfile

    from maua_stylegan2_amd import generate_audiovisual as gav
    from maua_stylegan2_amd import render, seeding
    from maua_stylegan2_amd.audioreactive.examples import sections

    monkeypatch.chdir(tmp_path)
    monkeypatch.setattr(render.shutil, "which", lambda name: None)
    monkeypatch.setattr(sections, "SECTION_TYPES", 2)  # the fixture has two kinds of section
    y = ref.sectioned_track("ABAB", 8, 120, seed=3)
    scipy.io.wavfile.write("track.wav", SR, (y * 32767 / max(1.0, float(np.abs(y).max()))).astype(np.int16))
    np.save("lat.npy", seeding.seeded_latents(8, 16, seed=3).numpy())
    seen = {}

    def get_latents(selection, args):
        seen["latents"] = sections.get_latents(selection, args)
        seen["n_frames"] = args.n_frames
        return seen["latents"]

    out = gav.generate(ckpt=None, audio_file="track.wav", initialize=sections.initialize, get_latents=get_latents,
                       get_noise=lambda height, width, scale, num_scales, args: None, latent_file="lat.npy", G_res=512, out_size=512,
                       fps=6, batch=4, output_file=str(tmp_path / "o.mp4"))
    n = seen["n_frames"]
    assert seen["latents"].is_cuda and seen["latents"].shape == (n, 16, 512) and bool(torch.isfinite(seen["latents"]).all())
    raw = np.fromfile(out + ".rgb24", dtype=np.uint8)
    assert raw.size == n * 512 * 512 * 3
    assert raw.reshape(n, 512, 512, 3).std() > 5
