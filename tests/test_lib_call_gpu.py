"""GPU: one launch through ``_lib.call``, and its refusals on real device tensors."""
import numpy as np
import pytest
import torch as th

pytestmark = pytest.mark.gpu

ENTRY = "maua_filterbank_f32"  # (fb [M, K], p [K, N], out [M, N], M, K, N, to_db, amin, stream)


def _operands(gpu):
    rng = np.random.default_rng(0)
    fb, p = rng.random((2, 3)).astype(np.float32), rng.random((3, 2)).astype(np.float32)
    return fb, p, th.from_numpy(fb).to(gpu), th.from_numpy(p).to(gpu)


def test_filterbank_through_call(gpu):
    from maua_stylegan2_amd import _lib

    fb, p, fbd, pd = _operands(gpu)
    out = th.empty((2, 2), dtype=th.float32, device=gpu)
    _lib.call(ENTRY, fbd, pd, out, 2, 3, 2, 0, 1e-10)
    want = (fb.astype(np.float64) @ p.astype(np.float64)).astype(np.float32)
    np.testing.assert_allclose(out.cpu().numpy(), want, rtol=2e-4, atol=1e-6 * want.max())  # project's bound in test_signal_gpu.py


def test_non_contiguous_tensor_launches_nothing(gpu):
    from maua_stylegan2_amd import _lib

    _, _, fbd, pd = _operands(gpu)
    out = th.full((2, 2), -7.0, dtype=th.float32, device=gpu)
    with pytest.raises(ValueError, match="maua_filterbank_f32: argument 1 must be contiguous"):
        _lib.call(ENTRY, fbd, pd.t(), out, 2, 3, 2, 0, 1e-10)
    th.cuda.synchronize(gpu)
    assert bool((out == -7.0).all())


def test_device_must_agree_with_the_tensors(gpu):
    from maua_stylegan2_amd import _lib

    if th.cuda.device_count() < 2:
        pytest.skip("needs two devices")
    _, _, fbd, pd = _operands(gpu)
    out = th.full((2, 2), -7.0, dtype=th.float32, device=gpu)
    with pytest.raises(ValueError, match="maua_filterbank_f32: argument 0 is on cuda:0, the launch goes to cuda:1"):
        _lib.call(ENTRY, fbd, pd, out, 2, 3, 2, 0, 1e-10, device=1)
    th.cuda.synchronize(gpu)
    assert bool((out == -7.0).all())
