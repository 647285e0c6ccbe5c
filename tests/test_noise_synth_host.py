"""CPU: the synthesised-noise entry (include/maua_hip.h, maua_noise_synth_f32) as a header declaration, a binding and a set of argument
refusals, and the host side of ``ar.NoiseSynth``: validation (no device involved) and the arithmetic of ``window``."""
import ctypes
import os
import re

import pytest
import torch

from conftest import REPO


def _header():
    return open(os.path.join(REPO, "include", "maua_hip.h")).read()


def test_entry_is_declared_exported_and_bound(built_lib):
    from maua_stylegan2_amd import _lib

    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    assert re.search(r"\bint\s+maua_noise_synth_f32\s*\(", code)
    assert "#define MAUA_NOISE_SYNTH_MAX_TERMS 4" in code and _lib.NOISE_SYNTH_MAX_TERMS == 4
    assert hasattr(ctypes.CDLL(built_lib), "maua_noise_synth_f32")
    assert "maua_noise_synth_f32" in _lib.exported_symbols() and len(_lib._SIGNATURES["maua_noise_synth_f32"][1]) == 6
    assert _lib.ABI_VERSION == 8 and _lib.load().maua_abi_version() == 8


def test_struct_layouts_equal_the_header(built_lib):
    """maua_noise_term_t: three pointers + two int32 = 32 bytes; maua_noise_synth_slot_t: pointer, three int32, float, uint64, four terms =
    160 bytes, every member at the offset a C compiler gives it."""
    from maua_stylegan2_amd import _lib

    term, slot = _lib.NoiseTerm, _lib.NoiseSynthSlot
    assert ctypes.sizeof(term) == 3 * 8 + 2 * 4 == 32
    assert [getattr(term, n).offset for n in ("bank", "envelope", "mask", "period", "phase")] == [0, 8, 16, 24, 28]
    assert ctypes.sizeof(slot) == 8 + 3 * 4 + 4 + 8 + 4 * 32 == 160
    assert [getattr(slot, n).offset for n in ("dst", "hw", "slot", "n_terms", "gain", "seed", "term")] == [0, 8, 12, 16, 20, 24, 32]
    # the member lists of the header, in order
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    body = lambda name: re.search(r"typedef struct \{([^}]*)\}\s*" + name + ";", code).group(1)  # noqa: E731
    members = lambda name: re.findall(r"(\w+)(?:\[\w+\])?;", body(name))  # noqa: E731
    assert members("maua_noise_term_t") == [n for n, _ in term._fields_]
    assert members("maua_noise_synth_slot_t") == [n for n, _ in slot._fields_]


def test_entry_refuses_bad_arguments_without_gpu(built_lib):
    from maua_stylegan2_amd import _lib

    lib = _lib.load()
    fake = 0x1000  # never dereferenced: every call below is rejected during validation
    call = lambda table=fake, n=1, batch=1, frame0=0, src=None: lib.maua_noise_synth_f32(table, n, batch, frame0, src, None)  # noqa: E731
    assert call(table=None) == -22
    assert call(n=0) == -22 and call(n=33) == -22 and call(n=-1) == -22
    assert call(batch=0) == -22 and call(batch=-2) == -22
    assert call(frame0=-1) == -22 and call(frame0=-1, src=fake) == -22


# ------------------------------------------------------------------------------------------------ ar.NoiseSynth on the host
H, W = 5, 7


def _synth(*a, **k):
    import maua_stylegan2_amd.audioreactive as ar

    return ar.NoiseSynth(*a, device="cpu", **k)


def test_validation_needs_no_device_and_names_the_fault():
    import maua_stylegan2_amd.audioreactive as ar

    t = ar.noise_term
    bank, env, mask = torch.zeros(3, 1, H, W), torch.zeros(19), torch.zeros(H, W)
    ok = _synth(H, W, [t(bank, env, mask, 4), t(torch.zeros(2, H, W)), t(torch.zeros(H, W), phase=-1), t("randn", env)], gain=0.5, seed=2 ** 40)
    assert ok.shape == (19, 1, H, W) and ok.n_frames == 19 and ok.seed == 2 ** 40
    assert [(p, ph) for _, _, _, p, ph in ok._terms] == [(3, 1), (2, 0), (1, 0), (1, 0)]  # phases reduced mod P
    free = _synth(H, W, [t(bank)])
    assert free.n_frames is None and free.shape == (1, 1, H, W)
    for terms, match in [([], "1 to 4"), ([t(bank)] * 5, "1 to 4"),
                         ([t(torch.zeros(3, 1, H, W + 1))], "bank"), ([t(torch.zeros(3, 2, H, W))], "bank"), ([t(torch.zeros(H * W))], "bank"),
                         ([t(torch.zeros(0, 1, H, W))], "P >= 1"), ([t("white")], "randn"), ([t(None)], "bank"),
                         ([t(bank, mask=torch.zeros(W, H))], "mask"), ([t(bank, mask=torch.zeros(1, H, W))], "mask"),
                         ([t(bank, envelope=torch.zeros(19, 1))], "envelope"), ([t(bank, envelope=torch.zeros(0))], "envelope"),
                         ([t("randn"), t("randn")], "at most one"),
                         ([t(bank, torch.zeros(19)), t(bank, torch.zeros(18))], "18 frames"),
                         ([t(bank, phase=1.5)], "phase")]:
        with pytest.raises((ValueError, TypeError), match=match):
            _synth(H, W, terms)
    for gain in (float("nan"), float("inf"), -float("inf"), "1"):
        with pytest.raises(ValueError, match="gain"):
            _synth(H, W, [t(bank)], gain=gain)
    with pytest.raises(ValueError, match="seed"):
        _synth(H, W, [t("randn")], seed=-1)
    with pytest.raises(RuntimeError, match="HIP device"):
        ok.frames(0, 1)  # evaluation is the device's: no CPU fallback


def test_window_continues_loops_envelopes_and_counter():
    """Periods 1, 5, 7 with phases 0, 3, 6 + a randn term, window (11, 19): row by row what the full recipe has at frame lo + i, in the
    table entry the recipe would write (phase, period and envelope pointer) as well."""
    import maua_stylegan2_amd.audioreactive as ar

    t = ar.noise_term
    n = 23
    envs = [torch.arange(n, dtype=torch.float32) + 100 * k for k in range(4)]
    banks = [torch.zeros(p, H, W) for p in (1, 5, 7)]
    full = _synth(H, W, [t(banks[0], envs[0], phase=0), t(banks[1], envs[1], phase=3), t(banks[2], envs[2], phase=6), t("randn", envs[3])], seed=9)
    lo, hi = 11, 19
    win = full.window(lo, hi)
    assert win.n_frames == hi - lo and win.shape == (hi - lo, 1, H, W) and win.offset == lo and full.offset == 0 and full.n_frames == n
    assert all(a[0] is b[0] and a[1] is b[1] for a, b in zip(win._terms, full._terms))  # shares banks and envelopes: nothing copied

    def entry_rows(recipe, i):
        """(bank row per term, envelope value per term, counter frame) of local frame i, from the entry launched with frame0 = offset."""
        e = recipe.table_entry(dst=0x1000, slot=3)
        assert (e.hw, e.slot, e.n_terms, e.seed) == (H * W, 3, 4, 9)
        rows, values = [], []
        for k in range(4):
            term = e.term[k]
            rows.append(None if not term.bank else (recipe.offset + i + term.phase) % term.period)
            assert 0 <= term.phase < term.period
            values.append(ctypes.cast(term.envelope + 4 * i, ctypes.POINTER(ctypes.c_float))[0])
        return rows, values, recipe.offset + i

    for i in range(hi - lo):
        want_rows = [(lo + i + ph) % p for p, ph in ((1, 0), (5, 3), (7, 6))] + [None]
        assert win.rows(i) == (want_rows, lo + i) == full.rows(lo + i)
        assert entry_rows(win, i) == entry_rows(full, lo + i) == (want_rows, [float(lo + i + 100 * k) for k in range(4)], lo + i)
    # window of a window composes
    inner = win.window(2, 6)
    assert inner.offset == lo + 2 and inner.n_frames == 4
    for i in range(4):
        assert inner.rows(i) == full.rows(lo + 2 + i) and entry_rows(inner, i) == entry_rows(full, lo + 2 + i)
    same = full.window(lo + 2, lo + 6)
    assert [entry_rows(same, i) for i in range(4)] == [entry_rows(inner, i) for i in range(4)]
    for bad in ((-1, 3), (5, 4), (0, hi - lo + 1)):
        with pytest.raises(ValueError):
            win.window(*bad)
    # a recipe without envelopes has no length: any window, only the offset moves
    loose = _synth(H, W, [t(banks[1], phase=3)]).window(1000, 1003)
    assert loose.n_frames is None and loose.rows(2) == ([(1002 + 3) % 5], 1002)
    # gain and structure travel
    assert full.with_gain(0.25).gain == 0.25 and full.gain == 1.0
    rebuilt = ar.NoiseSynth.from_structure(win.structure(), "cpu", win.tensors())
    assert [entry_rows(rebuilt, i) for i in range(hi - lo)] == [entry_rows(win, i) for i in range(hi - lo)]
