"""CPU: the inventory behind tests/test_input_forms_gpu.py — every ``_lib.call`` site of the audio modules has an operand spec
(tests/entry_specs.py) and a row of the function table (tests/input_form_cases.py) or a written exclusion — and the checking wrapper
itself, fed with CPU tensors and a stub in place of ``_lib.call``: nothing here touches a device."""
import ast
import ctypes
import glob
import os

import numpy as np
import pytest
import torch as th

import entry_specs as es
import input_form_cases as cases

HERE = os.path.dirname(os.path.abspath(__file__))
GLUE = os.path.join(os.path.dirname(HERE), "maua_stylegan2_amd", "audioreactive")

# the rows the table has to hold, by module
EXPECTED_ROWS = {
    "signal": ["stft_power", "stft_complex", "project", "hpss", "resample", "gaussian_filter", "cens", "nn_filter", "cqt_magnitude", "raw_pitch",
               "raw_pyin"],
    "decompose": ["nmf", "nmf_divergence", "separate"],
    "beat": ["raw_plp", "tempogram_peak", "pulse_synth"],
    "segment": ["tempogram", "beat_dp", "beat_sync", "knn_links", "rec_affinity"],
    "harmony": ["viterbi", "hmm_posterior"],
    "bars": ["bar_viterbi"],
    "filters": ["sosfilt", "sosfiltfilt", "envelope"],
    "latent": ["perlin_noise", "loop_sections"],
}
# operands the table has to vary where a function has more than its first one
EXPECTED_VARIED = {"project": {"fb", "p"}, "nmf": {"V", "W"}, "nmf_divergence": {"V", "W", "H"}, "tempogram_peak": {"env", "table", "prior"},
                   "sosfilt": {"x", "zi"}}


def call_sites():
    """[(module, enclosing function — "Class.method" for a method —, entry name)] of every ``_lib.call("maua_...", ...)``."""
    sites = []

    class Walk(ast.NodeVisitor):
        def __init__(self, module):
            self.module, self.stack = module, []

        def scoped(self, node):
            self.stack.append(node.name)
            self.generic_visit(node)
            self.stack.pop()

        visit_FunctionDef = visit_AsyncFunctionDef = visit_ClassDef = scoped

        def visit_Call(self, node):
            f = node.func
            if isinstance(f, ast.Attribute) and f.attr == "call" and isinstance(f.value, ast.Name) and f.value.id == "_lib":
                assert node.args and isinstance(node.args[0], ast.Constant) and isinstance(node.args[0].value, str), \
                    f"{self.module}.py:{node.lineno}: the entry of a _lib.call must be a string literal"
                assert self.stack, f"{self.module}.py:{node.lineno}: a _lib.call at module level"
                sites.append((self.module, ".".join(self.stack), node.args[0].value))
            self.generic_visit(node)

    for path in sorted(glob.glob(os.path.join(GLUE, "*.py"))):
        with open(path) as fh:
            Walk(os.path.splitext(os.path.basename(path))[0]).visit(ast.parse(fh.read(), path))
    return sites


def sample_args(name):
    """Arguments of the right kinds for ``name``'s slots: small distinct integers, 0.5 for the reals, [2, 3] for a host int32 table and
    None in every pointer slot (a spec reads the integers alone)."""
    from maua_stylegan2_amd import _lib

    out = []
    for i, slot in enumerate(_lib._SIGNATURES[name][1][:-1]):
        if slot is ctypes.c_void_p:
            out.append(None)
        elif slot in (ctypes.c_float, ctypes.c_double):
            out.append(0.5)
        elif slot in (ctypes.c_int, ctypes.c_int64):
            out.append(2 + i % 5)
        else:
            assert slot is _lib._I32P, (name, i, slot)
            out.append(np.array([2, 3], np.int32))
    return out


def test_inventory_every_call_site_has_a_spec_and_a_row(built_lib):
    from maua_stylegan2_amd import _lib

    sites = call_sites()
    entries = sorted({entry for _, _, entry in sites})
    assert len(sites) >= 40 and len(entries) >= 35, "the walk lost the call sites"
    assert all(entry.startswith("maua_") for entry in entries)
    missing = [entry for entry in entries if entry not in es.SPECS]
    assert not missing, f"entries launched from audioreactive/*.py without a spec in tests/entry_specs.py: {missing}"
    stale = sorted(set(es.SPECS) - set(entries))
    assert not stale, f"specs of entries no audio module launches: {stale}"
    for entry in entries:
        slots = _lib._SIGNATURES[entry][1]
        assert slots[-1] is ctypes.c_void_p  # the stream
        assert es.arity(entry) == len(slots) - 1, f"{entry}: the spec takes {es.arity(entry)} arguments, the binding {len(slots) - 1}"
        named = es.SPECS[entry](*sample_args(entry))
        indices = [i for i, _, _ in named]
        assert indices and len(set(indices)) == len(indices), f"{entry}: the spec names {indices}"
        for i, dtype, numel in named:
            assert slots[i] is ctypes.c_void_p, f"{entry}: argument {i} is no void* slot"
            assert all(isinstance(d, th.dtype) for d in (dtype if isinstance(dtype, tuple) else (dtype,))), (entry, i, dtype)
            assert int(numel) > 0, f"{entry}: argument {i} needs {numel} elements for the sample arguments"
        assert es.NULLABLE[entry] <= set(indices), f"{entry}: NULLABLE names an argument the spec does not"
    # the structs that travel as bytes
    assert es.FRAME_SOURCE_BYTES == ctypes.sizeof(_lib.FrameSource) and es.NOISE_SYNTH_SLOT_BYTES == ctypes.sizeof(_lib.NoiseSynthSlot)

    # the function table
    names = [row.name for row in cases.ROWS]
    assert len(set(names)) == len(names)
    assert len({row.function for row in cases.ROWS}) == len(names), "test ids are built from the function name alone"
    expected = [f"{module}.{function}" for module, functions in EXPECTED_ROWS.items() for function in functions]
    assert sorted(names) == sorted(expected), f"rows missing: {sorted(set(expected) - set(names))}, unexpected: {sorted(set(names) - set(expected))}"
    for row in cases.ROWS:
        assert row.varied and set(row.varied) <= set(row.operands), row.name
        assert row.refuse <= {(op, form) for op in row.varied for form in ("otherdev",)}, f"{row.name}: only another device may be refused"
        if row.function in EXPECTED_VARIED:
            assert set(row.varied) == EXPECTED_VARIED[row.function], row.name
    covered = {site for row in cases.ROWS for site in row.covers}
    enclosing = {f"{module}.{function}" for module, function, _ in sites}
    assert covered <= enclosing, f"rows cover functions that launch nothing: {sorted(covered - enclosing)}"
    assert all(reason.strip() for reason in list(cases.EXCLUDED_MODULES.values()) + list(cases.EXCLUDED_FUNCTIONS.values()))
    assert set(cases.EXCLUDED_FUNCTIONS) <= enclosing and not set(cases.EXCLUDED_FUNCTIONS) & covered
    assert not {name.split(".")[0] for name in covered} & set(cases.EXCLUDED_MODULES)
    orphans = sorted(site for site in enclosing if site not in covered and site not in cases.EXCLUDED_FUNCTIONS
                     and site.split(".")[0] not in cases.EXCLUDED_MODULES)
    assert not orphans, f"functions with a _lib.call that no row of tests/input_form_cases.py runs and no exclusion explains: {orphans}"


def test_mismatch_list_holds_every_tie():
    names = [c.name for c in cases.MISMATCHES]
    assert len(set(names)) == len(names)
    for function in ("project", "nmf_divergence", "nmf", "tempogram_peak", "viterbi", "hmm_posterior", "sosfilt", "bar_viterbi", "beat_sync"):
        tags = [n for n in names if n.startswith(function + "[")]
        assert any(n.endswith("+1]") for n in tags) and any(n.endswith("-1]") for n in tags), function
    for must in ("project[p-rows+1]", "project[p-rows-1]", "nmf_divergence[H-rows+1]", "nmf_divergence[H-rows-1]", "sosfilt[zi-sections+1]",
                 "sosfilt[x-rows-1]", "viterbi[matrix+1]", "hmm_posterior[vector-1]", "tempogram_peak[prior+1]", "nmf[W-cols-1]"):
        assert must in names, must


class Stub:
    """Stands in for ``_lib.call``: records what reaches it."""

    def __init__(self):
        self.calls = []

    def __call__(self, name, *args, device=None):
        self.calls.append((name, args, device))


def good_operands(name):
    """Arguments that fit ``name``'s spec exactly: CPU tensors of the minimum size in every pointer slot the spec names."""
    args = sample_args(name)
    named = es.SPECS[name](*args)
    for i, dtype, numel in named:
        args[i] = th.zeros(int(numel), dtype=dtype[0] if isinstance(dtype, tuple) else dtype)
    assert es.SPECS[name](*args) == named, "a spec reads the integer arguments alone"
    return args, named


WRONG = {th.float32: th.float64, th.float64: th.float32, th.int32: th.int64, th.uint8: th.int8, th.int16: th.int32}


@pytest.mark.parametrize("name", sorted(es.SPECS))
def test_wrapper_forwards_what_fits_and_nothing_else(built_lib, name):
    # every entry of the audio modules: the two lapses (maua_filterbank_f32, maua_nmf_kl_div_f32) and all entries of every module
    args, named = good_operands(name)
    stub = Stub()
    call = es.checked_call(stub)
    call(name, *args, device=0)
    assert call.launches == 1 and len(stub.calls) == 1 and stub.calls[0][0] == name and stub.calls[0][2] == 0
    assert all(a is b for a, b in zip(stub.calls[0][1], args)), "the operands must reach the call as they were given"
    for i, dtype, numel in named:
        first = dtype[0] if isinstance(dtype, tuple) else dtype
        short = list(args)
        short[i] = th.zeros(int(numel) - 1, dtype=first)
        with pytest.raises(AssertionError, match=rf"{name}: argument {i} has {int(numel) - 1} elements, expected at least {int(numel)}"):
            call(name, *short, device=0)
        mistyped = list(args)
        mistyped[i] = th.zeros(int(numel), dtype=WRONG[first])
        with pytest.raises(AssertionError, match=rf"{name}: argument {i} is {WRONG[first]}, expected"):
            call(name, *mistyped, device=0)
        absent = list(args)
        absent[i] = None
        if i in es.NULLABLE[name]:
            call(name, *absent, device=0)
        else:
            with pytest.raises(AssertionError, match=rf"{name}: argument {i} is None"):
                call(name, *absent, device=0)
    allowed = sum(1 for i, _, _ in named if i in es.NULLABLE[name])
    assert call.launches == len(stub.calls) == 1 + allowed and call.refused == 2 * len(named) + len(named) - allowed


def test_wrapper_refuses_what_it_does_not_know():
    stub = Stub()
    call = es.checked_call(stub)
    with pytest.raises(AssertionError, match="maua_no_such_entry: no operand spec"):
        call("maua_no_such_entry", th.zeros(3))
    with pytest.raises(AssertionError, match="maua_filterbank_f32: 3 arguments, the spec takes 8"):
        call("maua_filterbank_f32", th.zeros(3), th.zeros(3), th.zeros(3))
    # a tensor where the spec knows none (the int slot `m`), and something that is neither tensor, None nor address
    fb, p, out = th.zeros(6), th.zeros(6), th.zeros(4)
    with pytest.raises(AssertionError, match="maua_filterbank_f32: argument 3 is a tensor the spec does not name"):
        call("maua_filterbank_f32", fb, p, out, th.zeros(1), 3, 2, 0, 1e-10)
    with pytest.raises(AssertionError, match="maua_filterbank_f32: argument 1 is a ndarray, expected a tensor"):
        call("maua_filterbank_f32", fb, np.zeros(6, np.float32), out, 2, 3, 2, 0, 1e-10)
    call("maua_filterbank_f32", fb, 0x1000, out, 2, 3, 2, 0, 1e-10)  # an address passes unchecked, as in _lib.call
    assert len(stub.calls) == call.launches == 1 and call.refused == 4


def test_wrapper_restates_the_two_lapses():
    # fb [M, K] . p [K, N] -> out [M, N];  v [F, T], w [F, K], h [K, T] -> d_cols [T] float64 (include/maua_hip.h)
    assert es.SPECS["maua_filterbank_f32"](None, None, None, 5, 7, 3, 0, 1e-10) == [(0, th.float32, 35), (1, th.float32, 21), (2, th.float32, 15)]
    assert es.SPECS["maua_nmf_kl_div_f32"](None, None, None, 13, 70, 3, 1e-12, None) == [(0, th.float32, 910), (1, th.float32, 39),
                                                                                         (2, th.float32, 210), (7, th.float64, 70)]
    stub = Stub()
    call = es.checked_call(stub)
    v, w, cols = th.zeros(13, 70), th.zeros(13, 3), th.zeros(70, dtype=th.float64)
    with pytest.raises(AssertionError, match="maua_nmf_kl_div_f32: argument 2 has 140 elements, expected at least 210"):
        call("maua_nmf_kl_div_f32", v, w, th.zeros(2, 70), 13, 70, 3, 1e-12, cols)  # H one row short of W's columns
    with pytest.raises(AssertionError, match="maua_filterbank_f32: argument 1 is torch.float64"):
        call("maua_filterbank_f32", th.zeros(5, 7), th.zeros(7, 3, dtype=th.float64), th.zeros(5, 3), 5, 7, 3, 0, 1e-10)
    assert stub.calls == []
