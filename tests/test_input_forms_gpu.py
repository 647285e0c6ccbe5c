"""What the public ``ar.*`` device functions do with an operand that is not in its canonical form (tests/input_form_cases.py holds the
table): float64, a CPU tensor, a numpy array, a strided view, another GPU.  Exactly one of two answers is right, and the table says
which: the call is ACCEPTED and returns the dtype, shape and bits of the canonical call, or it is REFUSED with a ValueError / TypeError
that names the function before anything is launched.  An AttributeError, a refusal from inside ``_lib.call``, a MauaHipError or
different bits are failures.  There are no tolerances in this file.

Every test runs with ``checked_call`` (tests/entry_specs.py) in place of ``_lib.call``: a launch whose buffers are mistyped or
smaller than the entry's comment in include/maua_hip.h says is stopped with an AssertionError before it reaches the library, so glue
that loses its normalisation fails here without a kernel ever reading a bad buffer."""
import importlib
import re
import types

import numpy as np
import pytest
import torch as th

import entry_specs as es
import input_form_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture
def ar(gpu, monkeypatch):
    """The audio modules with the checking wrapper installed over ``_lib.call``; ``ar.call`` is the wrapper (its counters start at 0)."""
    from maua_stylegan2_amd import _lib
    call = es.checked_call(_lib.call)
    monkeypatch.setattr(_lib, "call", call)
    # by module path: the package re-exports functions under the names of some of its modules (ar.decompose is a function)
    modules = {name: importlib.import_module(f"maua_stylegan2_amd.audioreactive.{name}")
               for name in ("bars", "beat", "decompose", "filters", "harmony", "latent", "segment", "signal")}
    return types.SimpleNamespace(call=call, **modules)


def put(values, where, form, dev):
    """``values`` (numpy, canonical dtype) as the operand a form asks for; every form holds the same numbers."""
    on_device = lambda a: th.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    if form == "canon":
        return values.copy() if where == "np" else on_device(values)
    if form == "np64":
        out = values.astype(np.float64)
    elif form == "cpu32":
        out = th.from_numpy(values.astype(np.float32))
    elif form == "dev64":
        out = on_device(values.astype(np.float64))
    elif form == "otherdev":
        out = th.from_numpy(values.copy()).to("cuda:1")
    elif form == "strided":
        if values.ndim == 2:  # .t() of the stored transpose
            stored = np.ascontiguousarray(values.T)
            out = stored.T if where == "np" else on_device(stored).t()
        else:                 # every second element of an interleaved buffer (along the last axis)
            buf = np.full(values.shape[:-1] + (2 * values.shape[-1],), 77, dtype=values.dtype)
            buf[..., ::2] = values
            out = buf[..., ::2] if where == "np" else on_device(buf)[..., ::2]
        assert not (out.flags.c_contiguous if isinstance(out, np.ndarray) else out.is_contiguous())
    else:
        raise KeyError(form)
    same = out.detach().cpu().numpy() if isinstance(out, th.Tensor) else out
    assert same.shape == values.shape and np.array_equal(same.astype(np.float64), values.astype(np.float64)), "a form changed the values"
    return out


def leaves(result):
    """The arrays of a result, in order: tensors and arrays as numpy, a Python float as float64."""
    if isinstance(result, (tuple, list)):
        return [leaf for item in result for leaf in leaves(item)]
    if isinstance(result, th.Tensor):
        return [result.detach().cpu().numpy()]
    if isinstance(result, np.ndarray):
        return [result]
    if isinstance(result, float):
        return [np.full(1, result, dtype=np.float64)]
    raise TypeError(f"unexpected result {type(result).__name__}")


_CANON = {}  # row name -> the leaves of the canonical call, computed once (under the wrapper) and read-only from then on


def canonical(row, ar, dev):
    if row.name not in _CANON:
        got = leaves(row.call(ar, {name: put(op.values, op.where, "canon", dev) for name, op in row.operands.items()}))
        assert got and all(leaf.size for leaf in got), f"{row.name}: the canonical call returns nothing to compare"
        for leaf in got:
            leaf.flags.writeable = False
        _CANON[row.name] = got
    return _CANON[row.name]


def names(function, message):
    return re.search(rf"(?<![\w.]){re.escape(function)}(?!\w)", message) is not None


FORM_CASES = [pytest.param(row, operand, form, id=f"{row.function}[{operand}-{form}]")
              for row in cases.ROWS for operand in row.varied for form in cases.FORMS]


@pytest.mark.parametrize("row, operand, form", FORM_CASES)
def test_form_is_accepted_bit_for_bit_or_refused_by_name(ar, gpu, row, operand, form):
    if form == "otherdev" and th.cuda.device_count() < 2:
        pytest.skip("one GPU visible")
    want = canonical(row, ar, gpu)
    operands = {name: put(op.values, op.where, form if name == operand else "canon", gpu) for name, op in row.operands.items()}
    before = ar.call.launches
    if (operand, form) in row.refuse:
        with pytest.raises((ValueError, TypeError)) as refusal:
            row.call(ar, operands)
        assert names(row.function, str(refusal.value)), f"the refusal does not name {row.function}: {refusal.value}"
        assert ar.call.launches == before and ar.call.refused == 0
        return
    got = leaves(row.call(ar, operands))
    assert ar.call.launches > before and ar.call.refused == 0
    assert len(got) == len(want)
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.dtype == w.dtype and g.shape == w.shape, f"output {i}: {g.dtype} {g.shape}, the canonical call gives {w.dtype} {w.shape}"
        assert g.tobytes() == w.tobytes(), f"output {i} differs from the canonical call in {int((g != w).sum())} of {w.size} elements"


@pytest.mark.parametrize("case", [pytest.param(c, id=c.name) for c in cases.MISMATCHES])
def test_shape_mismatch_is_refused_before_any_launch(ar, gpu, case):
    with pytest.raises(ValueError) as refusal:
        case.call(ar, lambda values: th.from_numpy(np.ascontiguousarray(values)).to(gpu))
    assert names(case.function, str(refusal.value)), f"the refusal does not name {case.function}: {refusal.value}"
    assert ar.call.launches == 0 and ar.call.refused == 0
