"""GPU: maua_temporal_fold_u8 (csrc/temporal_fold.hip) byte for byte against the numpy restatement of its two formulas
(tests/temporal_fold_ref.py): every frame size / group count / sub-frame count / alignment it serves on both of its paths, the weights and
sums where a division could go wrong, every accumulator value of the linear-light search, and the launch inside a captured graph.  Guard
bytes of 0xA5 sit before and after every output and are checked after every launch; every input ends where its allocation ends."""
import ctypes

import numpy as np
import pytest
import torch

from temporal_fold_ref import accumulate_ref, fold_ref, srgb_tables_ref

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

GUARD, FILL = 256, 0xA5
FRAME_BYTES = [1, 3, 15, 16, 17, 48, 105, 3069, 12288, 196608]  # 105 = 5 x 7 x 3: a misaligned second frame; 3069 = 33 x 31 x 3
GROUPS = [1, 2, 3]
SUBFRAMES = [1, 2, 3, 5, 8, 16]
# (in, out) byte offsets from their allocations: the same offset keeps frame sizes that are multiples of 16 on the vector path, with a
# partial first and last column for 1, 3 and 15; different offsets send every size through the byte path
SAME = [(0, 0), (1, 1), (3, 3), (15, 15)]
MIXED = [(0, 1), (3, 0), (15, 3), (1, 15)]

_POOL = np.random.default_rng(20261019).integers(0, 256, 3 * 16 * 196608 + 4096, dtype=np.uint8)
_POOL.setflags(write=False)


def _bytes(count, start):
    start %= 4093
    return _POOL[start: start + count]


@pytest.fixture(scope="module")
def srgb(gpu):
    decode, threshold = srgb_tables_ref()
    return (decode, threshold), _device_tables(decode, threshold, gpu)


def _device_tables(decode, threshold, gpu):
    return tuple(torch.from_numpy(np.ascontiguousarray(t, dtype=np.uint16).view(np.int16).copy()).to(gpu) for t in (decode, threshold))


def _launch(gpu, frames, weights, in_off=0, out_off=0, tables=None):
    """frames uint8 [groups * N, frame_bytes] -> the kernel's uint8 [groups, frame_bytes], guards checked."""
    from maua_stylegan2_amd import _lib

    n = len(weights)
    groups, fb = frames.shape[0] // n, frames.shape[1]
    holder = torch.empty(in_off + frames.size, dtype=torch.uint8, device=gpu)
    src = holder[in_off:]  # ends exactly where its allocation ends
    src.copy_(torch.from_numpy(np.array(frames).reshape(-1)).to(gpu))  # (a copy: the pool the inputs are cut from is read-only)
    n_out = groups * fb
    buf = torch.full((GUARD + out_off + n_out + GUARD,), FILL, dtype=torch.uint8, device=gpu)
    out = buf[GUARD + out_off: GUARD + out_off + n_out]
    assert src.data_ptr() % 16 == in_off and out.data_ptr() % 16 == out_off
    dec, thr = tables if tables is not None else (None, None)
    rc = _lib.load().maua_temporal_fold_u8(src.data_ptr(), out.data_ptr(), groups, n, fb, (ctypes.c_uint8 * n)(*weights), _lib.ptr(dec),
                                           _lib.ptr(thr), _lib.stream_ptr(gpu))
    assert rc == 0, rc
    host = buf.cpu().numpy()
    assert (host[: GUARD + out_off] == FILL).all() and (host[GUARD + out_off + n_out:] == FILL).all(), "a guard byte was overwritten"
    return host[GUARD + out_off: GUARD + out_off + n_out].reshape(groups, fb)


@pytest.mark.parametrize("fb", FRAME_BYTES)
def test_random_frames_and_weights_on_every_shape_and_alignment(gpu, srgb, fb):
    """Random bytes, random weights (every third case with zeros among them), both light modes.  Sizes up to 3069 take every group count,
    sub-frame count and all eight alignment pairs; the two large sizes rotate group counts and alignment pairs over the sub-frame counts."""
    (decode, threshold), device_tables = srgb
    rng = np.random.default_rng(fb)
    case = 0
    for ni, n in enumerate(SUBFRAMES):
        for gi, groups in enumerate(GROUPS if fb <= 3069 else [GROUPS[ni % 3]]):
            offsets = SAME + MIXED if fb <= 3069 else [SAME[(ni + 1) % 4], MIXED[ni % 4]]
            for in_off, out_off in offsets:
                case += 1
                weights = rng.integers(0, 256, n)
                if case % 3 == 0:
                    weights[rng.integers(0, n)] = 0
                if not weights.any():
                    weights[0] = 1
                weights = [int(w) for w in weights]
                frames = _bytes(groups * n * fb, case * 131 + fb).reshape(groups * n, fb)
                linear = case % 2 == 0
                got = _launch(gpu, frames, weights, in_off, out_off, device_tables if linear else None)
                want = fold_ref(frames, weights, decode, threshold) if linear else fold_ref(frames, weights)
                assert np.array_equal(got, want), (fb, groups, n, in_off, out_off, weights, linear)


@pytest.mark.parametrize("weights", [[1, 2, 3], [0, 1, 0, 1], [0, 0, 5], [1, 1, 0, 0], [255, 1], [7, 0, 0, 0, 0, 0, 0, 9], [3] * 16, [1] + [0] * 15],
                         ids=lambda w: ",".join(map(str, w)))
def test_zero_weights_and_sums_that_are_no_power_of_two(gpu, srgb, weights):
    (decode, threshold), device_tables = srgb
    n = len(weights)
    for fb, (in_off, out_off) in [(48, (3, 3)), (105, (0, 0)), (3069, (1, 15))]:
        frames = _bytes(2 * n * fb, fb + n).reshape(2 * n, fb)
        assert np.array_equal(_launch(gpu, frames, weights, in_off, out_off), fold_ref(frames, weights))
        assert np.array_equal(_launch(gpu, frames, weights, in_off, out_off, device_tables), fold_ref(frames, weights, decode, threshold))


@pytest.mark.parametrize("weights", [[1, 1], [1, 1, 1, 1], [2, 2], [1, 2, 3], [255, 255], [5, 1, 0, 4]], ids=lambda w: ",".join(map(str, w)))
def test_even_sums_that_land_exactly_on_the_half_round_up(gpu, weights):
    """Every byte of these inputs has a weighted sum with remainder exactly W / 2 (asserted on the reference): the result is the quotient
    plus one."""
    n, total = len(weights), sum(weights)
    assert total % 2 == 0
    fb = 64
    # columns of random bytes, kept when their weighted sum has the remainder W / 2 (at least one column in W does)
    columns = np.random.default_rng(total).integers(0, 256, (n, 1 << 15), dtype=np.uint8)
    sums = (columns.astype(np.int64) * np.asarray(weights)[:, None]).sum(axis=0)
    frames = np.ascontiguousarray(columns[:, sums % total == total // 2][:, :fb])
    assert frames.shape == (n, fb)
    acc = (frames.astype(np.int64) * np.asarray(weights)[:, None]).sum(axis=0)
    assert np.all(acc % total == total // 2)
    want = fold_ref(frames, weights)
    assert np.array_equal(want[0], acc // total + 1)
    for offsets in [(0, 0), (1, 1), (0, 3)]:
        assert np.array_equal(_launch(gpu, frames, weights, *offsets), want)


def test_largest_accumulator_in_both_light_modes(gpu, srgb):
    (decode, threshold), device_tables = srgb
    weights = [255] * 16
    for fb, offsets in [(48, (0, 0)), (48, (15, 15)), (17, (0, 0))]:
        frames = np.full((2 * 16, fb), 255, np.uint8)
        mean, total = accumulate_ref(frames, weights, decode)
        assert total == 4080 and np.all(mean == 65535)  # 16 * 255 * 65535 + 2040: the largest numerator there is
        for tables, ref in [(None, fold_ref(frames, weights)), (device_tables, fold_ref(frames, weights, decode, threshold))]:
            got = _launch(gpu, frames, weights, *offsets, tables)
            assert np.array_equal(got, ref) and np.all(got == 255)
    saturated = np.full(256, 65535, np.uint16)  # the same numerator from every input byte, and a threshold table that ends in 65535
    top = threshold.copy()
    top[255] = 65535
    frames = _bytes(16 * 48, 5).reshape(16, 48)
    got = _launch(gpu, frames, weights, 0, 0, _device_tables(saturated, top, gpu))
    assert np.array_equal(got, fold_ref(frames, weights, saturated, top)) and np.all(got == 255)


def test_one_sub_frame_is_the_identity(gpu, srgb):
    _, device_tables = srgb
    ramp = np.concatenate([np.arange(256), _bytes(3069 - 256, 9)]).astype(np.uint8)
    for fb in (3069, 256, 48):
        frames = np.stack([ramp[:fb], ramp[:fb][::-1], np.roll(ramp[:fb], 7)])
        for w in (1, 7, 255):
            for offsets in [(0, 0), (3, 3), (1, 0)]:
                assert np.array_equal(_launch(gpu, frames, [w], *offsets), frames)
                assert np.array_equal(_launch(gpu, frames, [w], *offsets, device_tables), frames)


def _adversarial_thresholds():
    """Non-decreasing from 0 with runs of repeated values (the search must land on the LAST entry of a run), steps of one, a jump over
    half the range, and a last threshold of 65535."""
    thr = np.zeros(256, np.int64)
    thr[1:8] = 0                 # a run at the very start: L = 0 encodes to 7
    thr[8:64] = 1 + np.arange(56)  # steps of one
    thr[64:96] = 1000            # a long run
    thr[96:128] = 1001 + 3 * (np.arange(32) // 2)  # pairs
    thr[128:200] = 40000 + 257 * (np.arange(72) // 3)
    thr[200:254] = 65000 + np.arange(54)
    thr[254] = 65534
    thr[255] = 65535
    assert thr[0] == 0 and np.all(np.diff(thr) >= 0)
    return thr.astype(np.uint16)


@pytest.mark.parametrize("table", ["srgb", "adversarial"])
def test_linear_light_search_on_every_accumulator_value(gpu, srgb, table):
    """256 launches: launch k decodes byte v to 256 k + v, its one frame holds the bytes 0 .. 255 and N = 1, so L takes every 16-bit value
    exactly once (asserted on the reference) and each is searched in the threshold table."""
    from maua_stylegan2_amd import _lib

    threshold = srgb[0][1] if table == "srgb" else _adversarial_thresholds()
    decodes = (256 * np.arange(256)[:, None] + np.arange(256)[None, :]).astype(np.uint16)
    frame = np.arange(256, dtype=np.uint8)[None, :]
    seen = np.concatenate([accumulate_ref(frame, [1], decodes[k])[0].reshape(-1) for k in range(256)])
    assert np.array_equal(np.sort(seen), np.arange(65536, dtype=np.uint64))
    want = np.stack([fold_ref(frame, [1], decodes[k], threshold)[0] for k in range(256)])
    if table == "adversarial":
        assert want[0, 0] == 7 and want[255, 255] == 255 and want[255, 254] == 254
    dev_decodes = torch.from_numpy(decodes.view(np.int16).copy()).to(gpu)
    dev_threshold = torch.from_numpy(threshold.view(np.int16).copy()).to(gpu)
    src = torch.from_numpy(frame[0].copy()).to(gpu)
    buf = torch.full((256, 64 + 256 + 64), FILL, dtype=torch.uint8, device=gpu)
    lib, one = _lib.load(), (ctypes.c_uint8 * 1)(1)
    for k in range(256):
        rc = lib.maua_temporal_fold_u8(src.data_ptr(), buf[k, 64:320].data_ptr(), 1, 1, 256, one, dev_decodes[k].data_ptr(),
                                       dev_threshold.data_ptr(), _lib.stream_ptr(gpu))
        assert rc == 0, (k, rc)
    host = buf.cpu().numpy()
    assert (host[:, :64] == FILL).all() and (host[:, 320:] == FILL).all()
    assert np.array_equal(host[:, 64:320], want)


def test_captured_launch_replays_on_changed_input(gpu, srgb):
    """The entry between maua_graph_begin_capture and maua_graph_end_capture (no allocation, no synchronisation, the weights by value: the
    host array is overwritten after the capture), replayed twice on changed input: equal to the eager launch = the reference."""
    from maua_stylegan2_amd import _lib

    (decode, threshold), device_tables = srgb
    lib = _lib.load()
    groups, n, fb = 2, 4, 3069
    inputs = [_bytes(groups * n * fb, seed).reshape(groups * n, fb) for seed in (21, 22, 23)]
    stream = torch.cuda.Stream(gpu)
    for tables, mode in [((None, None), "encoded"), (device_tables, "linear")]:
        weights = [1, 2, 2, 1]
        host_weights = (ctypes.c_uint8 * n)(*weights)
        src = torch.from_numpy(inputs[0].copy()).to(gpu)
        buf = torch.full((GUARD + groups * fb + GUARD,), FILL, dtype=torch.uint8, device=gpu)
        out = buf[GUARD: GUARD + groups * fb]
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            with _lib.HipGraph() as graph:
                rc = lib.maua_temporal_fold_u8(src.data_ptr(), out.data_ptr(), groups, n, fb, host_weights, _lib.ptr(tables[0]), _lib.ptr(tables[1]),
                                               _lib.stream_ptr(gpu))
            assert rc == 0
            for i in range(n):
                host_weights[i] = 0  # the captured launch owns its copy
            for frames in inputs[1:]:
                src.copy_(torch.from_numpy(frames.copy()).to(gpu), non_blocking=False)
                out.fill_(FILL)
                graph.replay()
                stream.synchronize()
                eager = _launch(gpu, frames, weights, 0, 0, tables if mode == "linear" else None)
                want = fold_ref(frames, weights, decode, threshold) if mode == "linear" else fold_ref(frames, weights)
                host = buf.cpu().numpy()
                assert (host[:GUARD] == FILL).all() and (host[GUARD + groups * fb:] == FILL).all()
                assert np.array_equal(host[GUARD: GUARD + groups * fb].reshape(groups, fb), want) and np.array_equal(eager, want), mode


def test_fold_frames_reuses_its_scratch_buffer_and_refuses_ragged_batches(gpu):
    from maua_stylegan2_amd import render

    frames = _bytes(8 * 6 * 10 * 3, 77).reshape(8, 6, 10, 3)
    u8 = torch.from_numpy(frames.copy()).to(gpu)
    scratch = {}
    fold = render.TemporalFold(4, "tent", "linear")
    out = render.fold_frames(u8, fold, scratch)
    assert tuple(out.shape) == (2, 6, 10, 3) and out.dtype == torch.uint8 and len(scratch) == 1
    want = fold_ref(frames.reshape(8, -1), [1, 2, 2, 1], *srgb_tables_ref()).reshape(2, 6, 10, 3)
    assert np.array_equal(out.cpu().numpy(), want)
    again = render.fold_frames(u8, fold, scratch)
    assert again.data_ptr() == out.data_ptr() and len(scratch) == 1
    tail = render.fold_frames(u8[:4], render.TemporalFold(4), scratch)  # a tail batch: its own buffer, whole groups
    assert tuple(tail.shape) == (1, 6, 10, 3) and np.array_equal(tail.cpu().numpy(), fold_ref(frames[:4].reshape(4, -1), [1] * 4).reshape(1, 6, 10, 3))
    with pytest.raises(ValueError, match="whole groups"):
        render.fold_frames(u8[:6], fold, scratch)
    with pytest.raises(RuntimeError, match="uint8"):
        render.fold_frames(u8.float(), fold, scratch)
    empty = render.fold_frames(u8[:0], fold, scratch)
    assert tuple(empty.shape) == (0, 6, 10, 3)
