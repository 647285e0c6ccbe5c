"""CPU: ``_lib.call`` converts and checks its arguments before anything touches the device (no launches)."""
import contextlib
import ctypes

import numpy as np
import pytest
import torch as th

ENTRY = "maua_filterbank_f32"  # (fb, p, out, m, k, n, to_db, amin, stream)


@pytest.fixture
def lib(built_lib):
    from maua_stylegan2_amd import _lib

    _lib.load()
    return _lib


class Recorder:
    """Stands in for the loaded library: records the arguments of every entry called on it and returns ``rc``."""

    def __init__(self, rc=0):
        self.rc, self.calls = rc, []

    def __getattr__(self, name):
        def entry(*args):
            self.calls.append((name, args))
            return self.rc

        return entry


@pytest.fixture
def recorder(lib, monkeypatch):
    """_lib.call with the library, the stream lookup and the device guard replaced: nothing below reaches HIP."""
    rec = Recorder()
    guarded = []

    @contextlib.contextmanager
    def guard(dev):
        guarded.append(dev)
        yield

    monkeypatch.setattr(lib, "load", lambda: rec)
    monkeypatch.setattr(lib, "stream_ptr", lambda device=None: 0x5EED)
    monkeypatch.setattr(lib.torch.cuda, "device", guard)
    rec.guarded = guarded
    return rec


def test_cpu_tensor_is_refused_with_entry_and_position(lib):
    with pytest.raises(RuntimeError, match=r"maua_filterbank_f32: argument 1 must be a CUDA \(HIP\) tensor"):
        lib.call(ENTRY, 0x1000, th.zeros(3, 2), 0x3000, 2, 3, 2, 0, 1e-10, device=0)


def test_non_contiguous_tensor_is_refused(lib):
    for dev in ("cpu", "meta"):
        with pytest.raises(ValueError, match=r"maua_filterbank_f32: argument 0 must be contiguous"):
            lib.call(ENTRY, th.empty(4, 4, device=dev).t(), 0x2000, 0x3000, 4, 4, 4, 0, 1e-10, device=0)


def test_wrong_argument_count_comes_first(lib):
    bad = th.empty(4, 4).t()  # would be refused too, but the count is checked before any argument
    with pytest.raises(TypeError, match="maua_filterbank_f32 takes 8 arguments"):
        lib.call(ENTRY, bad, bad, bad)
    with pytest.raises(TypeError, match="maua_filterbank_f32 takes 8 arguments"):
        lib.call(ENTRY, bad, bad, bad, 2, 3, 2, 0, 1e-10, 0)  # the stream is not the caller's to pass


def test_host_query_is_refused(lib):
    with pytest.raises(TypeError, match="maua_bar_ws_bytes takes no stream"):
        lib.call("maua_bar_ws_bytes", 8, 2, 4, 2, device=0)


def test_host_int32_tables(lib, recorder):
    # maua_bar_viterbi_f64(logobs, n_frames, interval*, width*, log_change, K, beats*, n_models, ws, score, path, stream)
    i32 = np.array([4, 6], np.int32)
    args = lambda interval: (0x1000, 8, interval, i32, 0x2000, 2, i32, 2, 0x3000, 0x4000, 0x5000)  # noqa: E731
    for bad in (np.array([4, 6], np.int64), np.zeros((2, 2), np.int32)[:, 0], [4, 6]):
        with pytest.raises(TypeError, match="maua_bar_viterbi_f64: argument 2 must be a contiguous int32 numpy array"):
            lib.call("maua_bar_viterbi_f64", *args(bad), device=0)
    # accepted up to the device check: with neither a tensor nor device= there is nowhere to launch
    with pytest.raises(ValueError, match="maua_bar_viterbi_f64: no tensor argument names the launch device"):
        lib.call("maua_bar_viterbi_f64", *args(i32))
    assert recorder.calls == []
    lib.call("maua_bar_viterbi_f64", *args(i32), device=0)
    (name, got), = recorder.calls
    assert name == "maua_bar_viterbi_f64" and len(got) == 12
    for pos in (2, 3, 6):
        assert isinstance(got[pos], ctypes.POINTER(ctypes.c_int32)) and ctypes.addressof(got[pos].contents) == i32.ctypes.data


def test_proxy_sees_converted_arguments_and_one_stream(lib, recorder):
    lib.call(ENTRY, 0x1000, None, 0x3000, 2, 3, 2, 1, 1e-10, device="cuda:0")
    assert recorder.calls == [(ENTRY, (0x1000, None, 0x3000, 2, 3, 2, 1, 1e-10, 0x5EED))]
    assert recorder.guarded == [th.device("cuda", 0)]
    with pytest.raises(TypeError, match="maua_filterbank_f32: argument 2 must be a tensor, None or an address"):
        lib.call(ENTRY, 0x1000, None, 3.5, 2, 3, 2, 1, 1e-10, device=0)
    assert len(recorder.calls) == 1


def test_rejection_carries_the_entry_name(lib, recorder):
    recorder.rc = -22
    with pytest.raises(lib.MauaHipError, match="maua_filterbank_f32 failed with code -22"):
        lib.call(ENTRY, 0x1000, 0x2000, 0x3000, 2, 3, 2, 0, 1e-10, device=0)
