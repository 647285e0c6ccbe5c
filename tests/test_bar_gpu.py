"""GPU: the bar-pointer entry (csrc/bar.hip) called through the C ABI between red zones, over the case list of tests/bar_ref.py: the
cases checked against the dense decoder on the CPU; T = 1, 2, interval[0] - 1, interval[-1] and interval[-1] + 1 (the first wrap of
the ring); one tempo and one beat; an interval of 1; width == interval; 63, 64 and 65 lanes; a forbidden column of log_change;
nothing but ties; a NaN and a +inf observation; three bar lengths in one launch; the default model over 40 s; and the largest models
one CU holds (100 tempi; 320 lanes with 8 beats: K = 128 with B = 8 is refused, tests/test_bar_host.py says why).  score and path bit
for bit against the float64 restatement, two runs identical.  Every case ends with Guard.check: red zones intact round score, path
and the workspace, every element of score and path written."""
import ctypes

import numpy as np
import pytest
import torch

import bar_ref as r
from maua_stylegan2_amd import _lib
from redzone import Guard

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)

EINVAL = -22
OUT = ("score", "path")


def i32(values):
    values = [int(v) for v in values]
    return (ctypes.c_int32 * len(values))(*values)


def windows(g, T, K, beats, tag):
    ws_bytes = _lib.load().maua_bar_ws_bytes(T, K, max(beats), len(beats))
    assert ws_bytes > 0 and ws_bytes % 8 == 0
    return {"score": g.out((len(beats),), f"score.{tag}", torch.float64), "path": g.out((len(beats), T, 3), f"path.{tag}", torch.int32),
            "ws": g.out((ws_bytes // 8,), f"ws.{tag}", torch.float64)}


def call(logobs, lc, iv, wd, bt, n_frames, out, **override):
    a = dict(T=n_frames, K=len(iv), interval=iv, width=wd, beats=bt, n_models=len(bt))
    a.update(override)
    a["n_models"] = override.get("n_models", len(a["beats"]))
    ptr = lambda name, t: None if a.get("null") == name else t.data_ptr()  # noqa: E731
    return _lib.load().maua_bar_viterbi_f64(ptr("logobs", logobs), a["T"], i32(a["interval"]), i32(a["width"]), ptr("log_change", lc), a["K"],
                                            i32(a["beats"]), a["n_models"], ptr("ws", out["ws"]), ptr("score", out["score"]),
                                            ptr("path", out["path"]), _lib.stream_ptr(logobs.device))


def run_twice(gpu, ops, beats):
    lo, I, W, lc = ops
    with torch.cuda.device(gpu):
        g = Guard(gpu)
        d_lo, d_lc = g.inp(lo, "logobs"), g.inp(lc, "log_change", torch.float64)
        runs = []
        for tag in ("a", "b"):
            out = windows(g, len(lo), len(I), beats, tag)
            assert call(d_lo, d_lc, I, W, beats, len(lo), out) == 0
            runs.append(out)
        names = [f"{k}.{tag}" for tag in ("a", "b") for k in OUT]
        g.check(written=names, nonfinite_ok=names)
    return [{k: out[k].cpu().numpy() for k in OUT} for out in runs]


@pytest.mark.parametrize("case", r.gpu_cases(), ids=lambda c: c["name"])
def test_entry_bit_for_bit(gpu, case):
    ops = r.case_operands(case)
    want_score, want_path = r.decode(*ops, case["beats"])
    a, b = run_twice(gpu, ops, case["beats"])
    for key in OUT:
        assert r.same_bits(a[key], b[key]), f"{key}: two runs differ"
    wrong = int((a["path"] != want_path).any(-1).sum())
    print(f"{case['name']}: score {a['score'].tolist()} for {want_score.tolist()}, {wrong} of {want_path.shape[0] * want_path.shape[1]} path frames differ")
    assert r.same_bits(a["score"], want_score)
    assert r.same_bits(a["path"], want_path)
    if case["name"] in ("nan", "inf"):
        assert not np.isnan(want_score).any()
    else:
        assert np.isfinite(want_score).all()


def test_refusals_leave_the_outputs_untouched(gpu):
    lo, I, W, lc = r.random_operands([3, 4, 6], 10, 1)
    beats = (3, 4)
    refused = [dict(null=k) for k in ("logobs", "log_change", "ws", "score", "path")]
    refused += [dict(T=0), dict(T=-2), dict(T=(1 << 22) + 1), dict(K=0), dict(n_models=0), dict(n_models=9), dict(interval=[3, 3, 6]),
                dict(interval=[4, 3, 6]), dict(interval=[0, 4, 6]), dict(interval=[3, 4, 1025]), dict(width=[0, 2, 6]), dict(width=[1, 5, 6]),
                dict(beats=(0, 4)), dict(beats=(3, 9))]
    with torch.cuda.device(gpu):
        g = Guard(gpu)
        d_lo, d_lc = g.inp(lo, "logobs"), g.inp(lc, "log_change", torch.float64)
        for n, kw in enumerate(refused):
            out = windows(g, 10, 3, beats, f"r{n}")
            assert call(d_lo, d_lc, I, W, beats, 10, out, **kw) == EINVAL, kw
            assert all(g.untouched(f"{k}.r{n}") for k in OUT + ("ws",)), kw
        # a model over the LDS plan: 40 tempi of 61 .. 100 frames with an 8-beat bar are 320 rings of 100 doubles, 250 KiB
        big = r.random_operands(range(61, 101), 10, 2)
        assert _lib.load().maua_bar_lds_bytes(40, 8, 100) == 0 and _lib.load().maua_bar_lds_bytes(40, 3, 100) > 0
        d_lc40 = g.inp(big[3], "log_change40", torch.float64)
        out = windows(g, 10, 40, (3, 8), "big")
        assert call(d_lo, d_lc40, big[1], big[2], (3, 8), 10, out) == EINVAL
        assert all(g.untouched(f"{k}.big") for k in OUT + ("ws",))
        ok = windows(g, 10, 40, (3,), "fits")   # the same tempi with a 3-beat bar fit (and decode)
        assert call(d_lo, d_lc40, big[1], big[2], (3,), 10, ok) == 0
        g.check(written=["score.fits", "path.fits"])
        want = r.decode(lo, big[1], big[2], big[3], (3,))
        assert r.same_bits(ok["score"].cpu().numpy(), want[0]) and r.same_bits(ok["path"].cpu().numpy(), want[1])


def test_entry_is_capturable(gpu):
    """Captured into one hipGraph and replayed on new observations in the same buffers: each replay equals the eager call bit for bit,
    the second one the restatement."""
    first = r.random_operands([3, 4, 5, 7], 300, 21)
    other = r.random_operands([3, 4, 5, 7], 300, 22)
    beats = (3, 4)
    stream = torch.cuda.Stream(gpu)
    with torch.cuda.device(gpu):
        g = Guard(gpu)
        d_lo, d_lc = g.inp(first[0], "logobs"), g.inp(first[3], "log_change", torch.float64)
        cap = windows(g, 300, 4, beats, "graph")
        assert call(d_lo, d_lc, first[1], first[2], beats, 300, cap) == 0   # (a kernel's first launch sets its LDS attribute)
        torch.cuda.synchronize()
        with torch.cuda.stream(stream):
            with _lib.HipGraph() as graph:
                rc = call(d_lo, d_lc, first[1], first[2], beats, 300, cap)
            assert rc == 0
            replays = []
            for n, ops in enumerate((first, other)):
                d_lo.copy_(torch.from_numpy(ops[0]).to(gpu))
                d_lc.copy_(torch.from_numpy(ops[3]).to(gpu))
                stream.synchronize()
                graph.replay()
                stream.synchronize()
                replays.append({k: cap[k].cpu().numpy() for k in OUT})
                eager = windows(g, 300, 4, beats, f"eager{n}")
                assert call(d_lo, d_lc, first[1], first[2], beats, 300, eager) == 0
                stream.synchronize()
                for key in OUT:
                    assert r.same_bits(replays[-1][key], eager[key].cpu().numpy()), key
        torch.cuda.synchronize()
        g.check(written=[f"{k}.{tag}" for tag in ("graph", "eager0", "eager1") for k in OUT])
    assert not r.same_bits(replays[0]["path"], replays[1]["path"])
    want = r.decode(other[0], first[1], first[2], other[3], beats)
    assert r.same_bits(replays[1]["score"], want[0]) and r.same_bits(replays[1]["path"], want[1])


def test_wrapper_returns_device_tensors(gpu):
    import maua_stylegan2_amd.audioreactive as ar

    lo, I, W, lc = r.random_operands([3, 4, 5, 7], 120, 31)
    with torch.cuda.device(gpu):
        score, path = ar.bar_viterbi(lo, I, W, lc, beats_per_bar=(4, 3))
    assert score.is_cuda and score.dtype == torch.float64 and score.shape == (2,) and path.dtype == torch.int32 and path.shape == (2, 120, 3)
    want = r.decode(lo, I, W, lc, (4, 3))
    assert r.same_bits(score.cpu().numpy(), want[0]) and r.same_bits(path.cpu().numpy(), want[1])
    with pytest.raises(ValueError, match="raise tempo_min"):
        ar.bar_viterbi(lo, *ar.bar_model(r.FR, tempo_min=10))
