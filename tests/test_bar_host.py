"""CPU: tests/bar_ref.py — the numpy restatement of maua_bar_viterbi_f64 — against the dense tests/hmm_ref.viterbi on the model with
every state written out; the five deliberately wrong variants must each be told apart by the GPU test's own case list; known answers
on click envelopes with the default model (metre, beats, downbeats); and, through the built library without a device, the entry's
refusals and its two plan functions."""
import ctypes

import numpy as np
import pytest

import bar_ref as r
import hmm_ref
import pulse_ref as q
from maua_stylegan2_amd.audioreactive import bars

FR = r.FR
BEAT_TOL = 1.5 / FR   # 34.8 ms: one and a half envelope frames, the bound of tests/test_pulse_features_gpu.py


# ------------------------------------------------------------------------------------------------ the restatement is right
@pytest.mark.parametrize("intervals,B,T", r.DENSE_CASES, ids=[f"{'_'.join(map(str, iv))}-B{B}-T{T}" for iv, B, T in r.DENSE_CASES])
def test_restatement_against_the_dense_model(intervals, B, T):
    """Random widths, Dirichlet rows with an occasional -inf, observations 3 N(0, 1) in fp32, seed 0; at most 128 states.  The path is
    the dense decoder's.  The score may differ from the dense optimum by the reordering of one sum of 2 (T - 1) + 1 terms (prefix-sum
    differences instead of a chain along the path): at most 2 (T - 1) 2^-53 times the sum of the magnitudes of the terms on the
    path; the path re-scored under the dense model reaches the optimum within the same allowance."""
    lo, I, W, lc = r.random_operands(intervals, T, 0)
    lt, li, column, states = r.expand(I, W, lc, B)
    assert len(states) <= hmm_ref.MAX_STATES
    delta, _, dense = hmm_ref.viterbi(lo[:, column], lt, li)
    score, path = r.viterbi(lo, I, W, lc, B)
    assert np.array_equal(path, states[dense])
    rescored, magnitude = r.dense_score(lo, lt, column, states, path)
    allowance = 2 * (T - 1) * 2.0 ** -53 * magnitude
    print(f"score {score!r} dense {delta.max()!r} re-scored {rescored!r} allowance {allowance:.3g}")
    assert np.isfinite(score) and abs(score - delta.max()) <= allowance and abs(rescored - delta.max()) <= allowance


@pytest.fixture(scope="module")
def case_refs():
    return {c["name"]: (r.case_operands(c), c["beats"]) for c in r.gpu_cases()}


@pytest.mark.parametrize("variant", r.VARIANTS)
def test_the_gpu_cases_tell_every_wrong_variant_apart(variant, case_refs):
    caught = []
    for name, (ops, beats) in case_refs.items():
        if name in ("default-40s", "limit-tempi", "limit-beats"):
            continue  # (seconds each in numpy, and not needed: the small cases have to do it)
        want, got = r.decode(*ops, beats), r.decode(*ops, beats, variant=variant)
        if not (r.same_bits(want[0], got[0]) and r.same_bits(want[1], got[1])):
            caught.append(name)
    print(f"{variant}: told apart by {len(caught)} cases, first {caught[:3]}")
    assert caught


def test_case_list_and_corner_cases_of_the_definition():
    cases = r.gpu_cases()
    assert len({c["name"] for c in cases}) == len(cases)
    lanes = {len(c["intervals"]) * max(c["beats"]) for c in cases if c["intervals"]}
    assert {63, 64, 65} <= lanes
    for c in cases:
        lo, I, W, lc = r.case_operands(c)
        assert lo.dtype == np.float32 and lo.shape == (c["T"], 3) and lc.shape == (len(I),) * 2 and lc.dtype == np.float64
        assert np.all(np.diff(I) > 0) and np.all(W >= 1) and np.all(W <= I)
        assert r.lds_bytes(len(I), max(c["beats"]), int(I[-1])) > 0, c["name"]
    # K = 128 with B = 8 (the limits of both counts at once) cannot be decoded: strictly ascending intervals reach 128 frames, and 1024
    # rings of 128 doubles are 1 MiB; the largest models one CU holds are on the list instead (limit-tempi, limit-beats)
    assert r.lds_bytes(128, 8, 128) == 0 and r.lds_bytes(128, 1, 128) == 0
    assert r.lds_bytes(100, 1, 100) > 158 * 1024 and r.lds_bytes(101, 1, 101) == 0 and r.lds_bytes(40, 8, 40) > 64 * 1024
    # all ties: every compare is one, the path is the first state throughout and the model walks through interval[0]
    lo, I, W, lc = r.case_operands(next(c for c in cases if c["name"] == "all-ties"))
    score, path = r.viterbi(lo, I, W, lc, 4)
    assert score == 0 and path[-1].tolist() == [0, 0, 0] and set(path[:, 0].tolist()) == {0}
    # a NaN or +inf observation: nothing is chosen through a NaN; the score is -inf or finite, never NaN
    for name in ("nan", "inf"):
        lo, I, W, lc = r.case_operands(next(c for c in cases if c["name"] == name))
        score, path = r.viterbi(lo, I, W, lc, 3)
        assert not np.isnan(score) and path.min() >= 0
    # T = 1: the best single observation, and the first state that has it
    lo = np.array([[0.0, 1.0, 3.0]], np.float32)
    score, path = r.viterbi(lo, [2, 3], [1, 1], np.zeros((2, 2)), 2)
    assert score == 3.0 and path.tolist() == [[0, 0, 0]]
    lo = np.array([[4.0, 1.0, 3.0]], np.float32)
    score, path = r.viterbi(lo, [2, 3], [1, 1], np.zeros((2, 2)), 2)
    assert score == 4.0 and path.tolist() == [[0, 0, 1]]


# ------------------------------------------------------------------------------------------------ known answers
def test_bar_model():
    interval, width, lc = bars.bar_model(FR)
    assert interval.dtype == np.int32 and interval[0] == 13 and interval[-1] == 46 and np.all(np.diff(interval) == 1)
    assert 60 * FR / interval[0] <= 215 and 60 * FR / interval[-1] >= 55
    assert width.tolist() == [max(1, int(i) // 16) for i in interval]
    assert np.abs(np.exp(lc).sum(1) - 1).max() < 1e-12 and np.all(np.argmax(lc, 1) == np.arange(len(interval)))
    assert abs((lc[3, 5] - lc[3, 3]) + 40 * abs(interval[5] / interval[3] - 1)) < 1e-12
    assert r.lds_bytes(len(interval), 4, int(interval[-1])) < 64 * 1024
    for kw in (dict(tempo_min=0), dict(tempo_min=200, tempo_max=100), dict(observation_lambda=1), dict(transition_lambda=-1)):
        with pytest.raises(ValueError):
            bars.bar_model(FR, **kw)
    with pytest.raises(ValueError, match="no whole beat interval"):
        bars.bar_model(FR, tempo_min=199, tempo_max=200)


def decode_clicks(times, every, duration):
    interval, width, lc = bars.bar_model(FR)
    a, d, _ = r.accented_envelope(times, every, duration)
    score, path = r.decode(r.observations(a, d), interval, width, lc, (3, 4))
    best = int(np.argmax(score))
    beats, downs = r.path_events(path[best])
    return (3, 4)[best], abs(score[0] - score[1]), beats, downs


def judge(beats, downs, clicks, every, clear):
    """Every click has exactly one beat among the beats between the first and the last click; the worst offset on the ``clear`` clicks;
    the downbeats between the first and the last click fall on the accented clicks, one each."""
    lo, hi = clicks[0] - BEAT_TOL, clicks[-1] + BEAT_TOL
    beats, downs = beats[(beats >= lo) & (beats <= hi)], downs[(downs >= lo) & (downs <= hi)]
    owner = np.abs(beats[:, None] - clicks[None, :]).argmin(1)
    worst = np.abs(beats - clicks[owner])[clear[owner]].max()
    accents = clicks[::every]
    down_owner = np.abs(downs[:, None] - accents[None, :]).argmin(1)
    worst_down = np.abs(downs - accents[down_owner])[clear[::every][down_owner]].max()
    return (len(beats) == len(clicks) and np.array_equal(owner, np.arange(len(clicks))), worst,
            len(downs) == len(accents) and np.array_equal(down_owner, np.arange(len(accents))), worst_down)


@pytest.mark.parametrize("bpm,every", r.KNOWN_CLIPS, ids=[f"{int(b)}-{e}" for b, e in r.KNOWN_CLIPS])
def test_known_answers_on_click_envelopes(bpm, every):
    clicks = q.click_times(bpm, 20.0)
    found, margin, beats, downs = decode_clicks(clicks, every, 20.0)
    one_each, worst, downs_right, worst_down = judge(beats, downs, clicks, every, np.ones(len(clicks), bool))
    print(f"{bpm}/{every}: metre {found}, margin {margin:.1f} nats, worst beat {1e3 * worst:.1f} ms, worst downbeat {1e3 * worst_down:.1f} ms "
          f"(bound {1e3 * BEAT_TOL:.1f})")
    assert found == every and one_each and downs_right
    assert worst <= BEAT_TOL and worst_down <= BEAT_TOL


def test_known_answer_on_a_tempo_switch():
    first, second = q.switch_times(40, 20)   # 100 -> 150 BPM at 20 s
    clicks = np.concatenate([first, second])
    found, margin, beats, downs = decode_clicks(clicks, 4, 40.0)
    clear = np.abs(clicks - 20.0) > 1.0
    one_each, worst, downs_right, worst_down = judge(beats, downs, clicks, 4, clear)
    print(f"switch: metre {found}, margin {margin:.1f} nats, {len(clicks)} clicks, worst beat {1e3 * worst:.1f} ms and downbeat "
          f"{1e3 * worst_down:.1f} ms further than 1 s from the switch")
    assert len(clicks) == 83 and len(clicks[::4]) == 21
    assert found == 4 and one_each and downs_right and worst <= BEAT_TOL and worst_down <= BEAT_TOL


@pytest.mark.parametrize("name", list(r.AUDIO_CLIPS))
def test_the_audio_clips_of_the_feature_test_are_decided_by_the_restatement_alone(name):
    """The clips of tests/test_bar_features_gpu.py through the oracle's float64 spectrogram, the activations restated in numpy and
    the restatement of the decoder: the metre is decided with a margin of more than 5 nats (measured: 15.9, 13.5 and 22.2), every
    clear click has its beat and every clear accent its downbeat within two frames, with the envelope's lag of one frame taken off."""
    from oracle import signal_oracle as so

    audio, clicks, every, seconds, clear = r.audio_clip(name)
    edges = so._mel_to_hz_slaney(np.linspace(so._hz_to_mel_slaney(0.0), so._hz_to_mel_slaney(q.SR / 2.0), 130))[1:-1]
    a, d = r.activations_from_power(so.stft_power(audio), so.mel_filterbank(q.SR, 2048, 128), edges)
    score, path = r.decode(r.observations(a, d), *bars.bar_model(FR), (3, 4))
    best = int(np.argmax(score))
    beats, downs = r.path_events(path[best])
    beats, downs = beats - bars.ENVELOPE_LAG / FR, downs - bars.ENVELOPE_LAG / FR
    beats_ok, worst, downs_ok, worst_down = r.judge_events(beats, downs, clicks, every, clear, 2.0 / FR)
    print(f"{name}: metre {(3, 4)[best]}, margin {abs(score[0] - score[1]):.1f} nats, worst beat {1e3 * worst:.1f} ms, worst downbeat {1e3 * worst_down:.1f} ms")
    assert (3, 4)[best] == every and abs(score[0] - score[1]) > 5.0
    assert beats_ok and downs_ok and worst <= 2.0 / FR and worst_down <= 2.0 / FR


def test_observations():
    lo = r.observations([0.0, 0.5, 1.0], [0.0, 0.5, 1.0])
    assert lo.dtype == np.float32 and lo.shape == (3, 3)
    want = [[np.log(0.999 / 15), np.log(1e-3 * 0.95), np.log(1e-3 * 0.05)], [np.log(0.5 / 15), np.log(0.25), np.log(0.25)],
            [np.log(1e-3 / 15), np.log(0.999 * 0.05), np.log(0.999 * 0.95)]]
    assert np.abs(lo - np.array(want)).max() < 1e-6


# ------------------------------------------------------------------------------------------------ the entry, without a device
def test_entry_refuses_bad_arguments_without_a_gpu(built_lib):
    from maua_stylegan2_amd import _lib

    lib = _lib.load()
    fake = 0x1000  # never dereferenced
    i32 = lambda v: (ctypes.c_int32 * len(v))(*v)  # noqa: E731

    def call(**kw):
        interval, width, beats = kw.get("interval", [3, 4, 6]), kw.get("width", [1, 2, 6]), kw.get("beats", [3, 4])
        ptr = lambda name: None if kw.get("null") == name else fake  # noqa: E731
        host = lambda name, v: None if kw.get("null") == name else i32(v)  # noqa: E731
        return lib.maua_bar_viterbi_f64(ptr("logobs"), kw.get("T", 10), host("interval", interval), host("width", width), ptr("log_change"),
                                        kw.get("K", len(interval)), host("beats", beats), kw.get("n_models", len(beats)), ptr("ws"),
                                        ptr("score"), ptr("path"), None)

    for name in ("logobs", "interval", "width", "log_change", "beats", "ws", "score", "path"):
        assert call(null=name) == -22, name
    for kw in (dict(T=0), dict(T=-1), dict(T=(1 << 22) + 1), dict(K=0), dict(K=129), dict(n_models=0), dict(n_models=9),
               dict(interval=[3, 3, 6]), dict(interval=[4, 3, 6]), dict(interval=[0, 4, 6]), dict(interval=[3, 4, 1025], width=[1, 1, 1]),
               dict(width=[0, 2, 6]), dict(width=[1, 5, 6]), dict(width=[1, 2, 7]), dict(beats=[0, 4]), dict(beats=[3, 9]), dict(beats=[-1]),
               dict(interval=list(range(1, 102)), width=[1] * 101, beats=[1]),         # 101 tempi of 1 .. 101 frames: 161 KiB, over the plan
               dict(interval=[20, 100], width=[1, 1], beats=[3, 8] * 4),                # the widest bar of the call decides: 16 lanes x 100 frames fit,
               dict(interval=list(range(61, 101)), width=[1] * 40, beats=[3, 8]),       # ... 320 lanes x 100 frames do not
               dict(interval=list(range(1, 129)), width=[1] * 128, beats=[8])):         # both count limits at once: 1 MiB of ring
        if kw.get("interval") == [20, 100]:
            assert lib.maua_bar_lds_bytes(2, 8, 100) > 0   # (it would launch: not called, nothing here may touch a device)
            continue
        assert call(**kw) == -22, kw


def test_plan_functions_are_pure_functions_of_their_arguments(built_lib):
    from maua_stylegan2_amd import _lib

    lib = _lib.load()
    for K, B, I in [(1, 1, 1), (34, 4, 46), (34, 3, 46), (100, 1, 100), (101, 1, 101), (40, 8, 40), (128, 8, 128), (128, 1, 128), (97, 1, 97), (2, 8, 1000),
                    (2, 8, 1024), (20, 8, 100), (0, 1, 1), (129, 1, 1), (1, 0, 1), (1, 9, 1), (1, 1, 0), (1, 1, 1025), (128, 8, 1)]:
        got = [lib.maua_bar_lds_bytes(K, B, I) for _ in range(2)]
        assert got[0] == got[1] == r.lds_bytes(K, B, I), (K, B, I)
    assert lib.maua_bar_lds_bytes(34, 4, 46) == 8 * (34 * 35 + 2 * 136 + 136 * 46)     # 60.3 KiB: the default model with a 4-beat bar
    assert lib.maua_bar_lds_bytes(128, 8, 1) > 0 and lib.maua_bar_lds_bytes(40, 8, 100) == 0
    for T, K, B, M in [(1, 1, 1, 1), (1723, 34, 4, 2), (12920, 34, 4, 2), (100, 96, 1, 1), (1 << 22, 128, 8, 8)]:
        per_model = 24 * (T + 1) + 16 * (T + 1) + (T * K * B + 15) // 16 * 16
        assert lib.maua_bar_ws_bytes(T, K, B, M) == M * per_model == lib.maua_bar_ws_bytes(T, K, B, M)
    for bad in [(0, 1, 1, 1), ((1 << 22) + 1, 1, 1, 1), (10, 0, 1, 1), (10, 129, 1, 1), (10, 1, 9, 1), (10, 1, 1, 0), (10, 1, 1, 9)]:
        assert lib.maua_bar_ws_bytes(*bad) == -1, bad
    for fn, kw in ((bars.bar_viterbi, dict(logobs=np.zeros((4, 2), np.float32))), (bars.bar_viterbi, dict(logobs=np.zeros((0, 3), np.float32))),
                   (bars.bar_viterbi, dict(interval=[3, 3])), (bars.bar_viterbi, dict(width=[1, 9])), (bars.bar_viterbi, dict(beats_per_bar=(9,))),
                   (bars.bar_viterbi, dict(log_change=np.zeros((3, 3))))):
        args = dict(logobs=np.zeros((4, 3), np.float32), interval=[3, 4], width=[1, 1], log_change=np.zeros((2, 2)), beats_per_bar=(3, 4))
        args.update(kw)
        with pytest.raises(ValueError):   # raised from the shapes, before anything touches a device
            fn(**args)
    with pytest.raises(ValueError, match="raise tempo_min"):
        bars.bar_viterbi(np.zeros((4, 3), np.float32), *bars.bar_model(FR, tempo_min=10))
