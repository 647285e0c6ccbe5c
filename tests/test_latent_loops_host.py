"""CPU: the host side of the device latent loops (audioreactive/latent.py: spline_weights, loop_frame_tables, loop_sections' refusals;
include/maua_hip.h: maua_keyframe_blend_f32) — the spline weight matrix against the per-column scipy loop, the frame tables against a
plain restatement of the host paths' tiling, every refusal, the unchanged host path, and the entry declared, bound and exported.  No
device call."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch
from scipy import interpolate

from conftest import REPO

N_ARGS = 13


def _scipy_loop(keys, period):
    """spline_loops' per-column fit, verbatim: keys [m, F] float64 -> [period, F]."""
    x, knots = np.linspace(0, 1, period), np.linspace(0, 1, keys.shape[0])
    return np.stack([interpolate.splev(x, interpolate.splrep(knots, keys[:, j])) for j in range(keys.shape[1])], axis=1)


@pytest.mark.parametrize("m,period", [(4, 8), (5, 37), (13, 1000)])
def test_spline_weights_reproduce_the_per_column_fit(m, period):
    from maua_stylegan2_amd.audioreactive import latent

    keys = np.random.default_rng(m * period).standard_normal((m, 24)) * 3.0
    w = latent.spline_weights(m, period)
    assert w.shape == (period, m) and w.dtype == np.float64
    diff = np.abs(w @ keys - _scipy_loop(keys, period)).max()
    rows = np.abs(w.sum(1) - 1.0).max()
    print(f"spline_weights({m}, {period}): max |W keys - scipy| = {diff:.3g}, max |row sum - 1| = {rows:.3g}")
    assert diff <= 1e-12 and rows <= 1e-12
    assert latent.spline_weights(m, period) is w and not w.flags.writeable  # cached per (m, P), shared


def test_spline_weights_refuse_what_scipy_or_the_host_path_cannot_do():
    from maua_stylegan2_amd.audioreactive import latent

    with pytest.raises(ValueError, match="at least 4 keys"):
        latent.spline_weights(3, 10)
    with pytest.raises(ValueError, match="period"):
        latent.spline_weights(5, 0)


def _tiled_rows(n, period):
    """The host paths' tiling: the period int(n / P) times, then its head as the tail."""
    rows = list(range(period)) * int(n / period)
    return (rows + rows[: n - len(rows)])[:n]


@pytest.mark.parametrize("n,n_loops", [(37, 2), (7, 3), (1, 1)])
def test_frame_tables_of_one_section(n, n_loops):
    from maua_stylegan2_amd.audioreactive import latent

    period = latent._loop_period("spline", n, n_loops, 5)
    assert period == int(n // max(1, n_loops))
    row, sec = latent.loop_frame_tables([n], [period])
    assert row.dtype == sec.dtype == torch.int32
    assert row.tolist() == _tiled_rows(n, period) and sec.tolist() == [0] * n


def test_frame_tables_of_sections_with_an_empty_one_and_padded_frames():
    from maua_stylegan2_amd.audioreactive import latent

    frames, n_loops, pad = [1, 2, 0, 5], [1, 1, 1, 2.5], 3
    periods = [latent._loop_period("spline", f, n, 5) if f else 0 for f, n in zip(frames, n_loops)]
    assert periods == [1, 2, 0, 2]
    want_row, want_sec, base = [], [], 0
    for s, (f, p) in enumerate(zip(frames, periods)):
        if f:
            want_row += [base + r for r in _tiled_rows(f, p)]
            want_sec += [s] * f
            base += p
    want_row += [want_row[-1]] * pad
    want_sec += [want_sec[-1]] * pad
    row, sec = latent.loop_frame_tables(frames, periods, sum(frames) + pad)
    assert row.tolist() == want_row and sec.tolist() == want_sec
    # shared weight blocks: explicit first rows
    row, _ = latent.loop_frame_tables([4, 4], [2, 2], row_bases=[0, 0])
    assert row.tolist() == [0, 1, 0, 1, 0, 1, 0, 1]
    # a slerp period is whole legs
    assert latent._loop_period("slerp", 53, 2, 5) == 25 and latent._loop_period("slerp", 4, 1, 5) == 0


def test_loop_sections_refuses_on_the_host():
    """Every refusal is raised before the device is touched (this box has none)."""
    from maua_stylegan2_amd.audioreactive import latent

    sel = np.zeros((6, 2, 4), np.float32)

    def call(frames=(8, 8), key_starts=(0, 4), n_keys=4, n_loops=1, **kw):
        return latent.loop_sections(sel, list(frames), list(key_starts), n_keys, n_loops, **kw)

    with pytest.raises(ValueError, match="more than n_frames"):
        call(n_frames=15)
    with pytest.raises(ValueError, match="key_start 6"):
        call(key_starts=(0, 6))
    with pytest.raises(ValueError, match="key_start -1"):
        call(key_starts=(-1, 0))
    with pytest.raises(ValueError, match="n_keys"):
        call(n_keys=0)
    with pytest.raises(ValueError, match="n_keys"):
        call(n_keys=7)
    with pytest.raises(ValueError, match="section 1: 8 frames give a loop period of 0"):
        call(n_loops=[1, 9])
    with pytest.raises(ValueError, match="section 0"):
        call(frames=(4, 8), kind="slerp")           # 4 frames over 5 legs
    with pytest.raises(ValueError, match="at least 4 keys"):
        call(n_keys=2)                              # 3 keys with the closure
    with pytest.raises(ValueError, match="at least 4 keys"):
        call(n_keys=3, loop=False)
    with pytest.raises(ValueError, match="exceed"):
        latent.loop_sections(np.zeros((40, 2, 4), np.float32), [100], [0], latent.LOOP_MAX_KEYS, 1)  # 33 with the closure
    with pytest.raises(ValueError, match="kind"):
        call(kind="linear")
    with pytest.raises(ValueError, match="no last frame"):
        call(frames=(0, 0), n_frames=2)
    with pytest.raises(ValueError, match="n_loops"):
        call(n_loops=[1, 1, 1])
    with pytest.raises(ValueError, match="negative"):
        call(frames=(-1, 8))


def test_host_input_keeps_the_host_path(golden):
    from maua_stylegan2_amd.audioreactive import latent

    g = golden("audioreactive_torch.npz")
    for sel in (g["spline.sel"], torch.from_numpy(g["spline.sel"])):
        y = latent.spline_loops(sel, 37, 2)
        assert y.dtype == torch.float64 and not y.is_cuda
        np.testing.assert_allclose(y.numpy(), g["spline.y"], atol=1e-9)


def test_header_binding_and_library_agree_on_the_entry(built_lib):
    import maua_stylegan2_amd.audioreactive as ar
    from maua_stylegan2_amd import _lib
    from maua_stylegan2_amd.audioreactive import latent

    text = open(os.path.join(REPO, "include", "maua_hip.h")).read()
    limit = re.search(r"#define\s+MAUA_LOOP_MAX_KEYS\s+(\d+)\b", text)
    assert limit and int(limit.group(1)) == latent.LOOP_MAX_KEYS == 32
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    decl = re.search(r"\bint\s+maua_keyframe_blend_f32\s*\(([^)]*)\)", code)
    assert decl, "maua_keyframe_blend_f32 is not declared in include/maua_hip.h"
    assert len(decl.group(1).split(",")) == N_ARGS
    assert "maua_keyframe_blend_f32" in _lib.exported_symbols() and len(_lib._SIGNATURES["maua_keyframe_blend_f32"][1]) == N_ARGS
    assert hasattr(ctypes.CDLL(built_lib), "maua_keyframe_blend_f32"), "maua_keyframe_blend_f32 is not exported by the library"
    assert ar.loop_sections is latent.loop_sections and ar.spline_weights is latent.spline_weights  # star-exported like the bends


def test_entry_rejects_bad_arguments_without_gpu(built_lib):
    """Argument validation runs before any HIP call."""
    from maua_stylegan2_amd import _lib

    lib = _lib.load()
    fake = 0x1000  # never dereferenced: every call below is refused or a no-op

    def blend(bank=fake, n_bank=4, feats=8, key_idx=fake, weights=fake, row=fake, sec=fake, out=fake, n_frames=3, n_sections=1, n_rows=3,
              kmax=5):
        return lib.maua_keyframe_blend_f32(bank, n_bank, feats, key_idx, weights, row, sec, out, n_frames, n_sections, n_rows, kmax, None)

    for name in ("bank", "key_idx", "weights", "row", "sec", "out"):
        assert blend(**{name: None}) == -22, name
    for name in ("n_bank", "feats", "n_sections", "n_rows", "kmax"):
        assert blend(**{name: 0}) == -22 and blend(**{name: -1}) == -22, name
    assert blend(kmax=33) == -22 and blend(n_frames=-1) == -22
    assert blend(n_frames=0) == 0 and blend(n_frames=0, out=None) == 0  # nothing to write
