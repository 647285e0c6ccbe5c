"""CPU: the reference of the soft masks (tests/separate_ref.py) against known answers, its fp32 emulation against the derived ceiling,
the comparison helper against deliberately wrong variants, the float64 chain's own SDR figures, the ``groups=`` resolution of
``ar.separate``, the refusals of the C entry (no device call is reached) and ``ar.save_audio``."""
import ctypes

import numpy as np
import pytest
import torch

import separate_ref as sr

CASES = sr.gpu_cases()


def test_the_case_list_covers_every_size():
    shapes = {(c["F"], c["T"], c["K"]) for c in CASES}
    assert (1025, 1, 32) in shapes and (1, 1000, 1) in shapes
    assert {c["power"] for c in CASES} == {1, 2} and {1, 2} <= {c["G"] for c in CASES}
    empty = interleaved = False
    for c in CASES:
        re, im, W, H, group = sr.make_case(c)
        assert re.dtype == im.dtype == W.dtype == H.dtype == np.float32 and group.dtype == np.int32 and group.shape == (c["K"],)
        assert group.min() >= 0 and group.max() < c["G"] and (W >= 0.5).all() and (H >= 0.5).all()
        empty |= len(set(group.tolist())) < c["G"]
        interleaved |= bool((np.diff(group) < 0).any())
    assert empty and interleaved


@pytest.mark.parametrize("case", CASES, ids=sr.case_id)
def test_the_float64_masks_are_a_partition_of_unity(case):
    _, _, W, H, group = sr.make_case(case)
    m = sr.masks(W, H, group, case["G"], case["power"])
    assert m.shape == (case["G"], case["F"], case["T"]) and (m >= 0).all()
    assert np.abs(m.sum(axis=0) - 1).max() <= 4 * case["G"] * 2.0 ** -53
    used = set(group.tolist())
    for g in range(case["G"]):
        assert (m[g] > 0).all() if g in used else (m[g] == 0).all()
    if case["G"] == 1:
        assert (m == 1).all()


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["float64", "float32"])
@pytest.mark.parametrize("power", [1, 2])
def test_the_equal_split_applies_where_the_model_is_silent(dtype, power):
    re, im, W, H, _ = sr.make_case(dict(F=7, T=20, K=6, G=3, layout="runs", seed=1))
    group = np.array([0, 0, 2, 2, 2, 0], np.int32)  # group 1 is empty
    H[:, [0, 7, 19]] = 0
    W[3] = 0
    m = sr.masks(W, H, group, 3, power, dtype)
    third = dtype(1) / dtype(3)
    assert (m[:, :, [0, 7, 19]] == third).all() and (m[:, 3] == third).all()
    live = np.ones((7, 20), bool)
    live[:, [0, 7, 19]], live[3] = False, False
    assert (m[1][live] == 0).all() and (m[0][live] > 0).all() and (m[2][live] > 0).all()
    out_re, out_im = sr.separate(re, im, W, H, group, 3, power, dtype)
    assert np.array_equal(out_re[1][~live], (third * re.astype(dtype))[~live]) and np.array_equal(out_im[0][3], third * im.astype(dtype)[3])


@pytest.mark.parametrize("case", CASES, ids=sr.case_id)
def test_the_emulation_stays_under_the_ceiling(case):
    ref, emu = sr.result(case), sr.result(case, np.float32)
    e = sr.pair_error(emu, ref)
    assert emu[0].dtype == np.float32 and e <= sr.ceiling(case["K"], case["G"], case["power"]) and 4 * e <= sr.MASK_TOL
    assert sr.compare(emu, ref, sr.tolerance(case)) == []
    if case["G"] == 1:  # q / q == 1: the input itself, bit for bit
        re, im = sr.make_case(case)[:2]
        assert np.array_equal(emu[0][0], re) and np.array_equal(emu[1][0], im)


def test_the_tolerance_is_four_times_the_worst_emulation_error():
    worst = max(sr.pair_error(sr.result(c, np.float32), sr.result(c)) for c in CASES)
    assert 4 * worst <= sr.MASK_TOL <= 4 * worst * 1.1, worst  # rounded up to two digits


DEFECT_CASES = [c for c in CASES if c["power"] == 2 and (c["F"], c["T"], c["K"]) in ((1025, 64, 3), (7, 64, 4), (7, 1000, 9), (7, 65, 32))]


@pytest.mark.parametrize("defect", ["window", "power_per_component", "swap_groups"])
@pytest.mark.parametrize("case", DEFECT_CASES, ids=sr.case_id)
def test_an_emulation_with_one_defect_fails_the_comparison(case, defect):
    """The comparison of the GPU test (compare at MASK_TOL) on an fp32 emulation that normalises over a window of the groups instead of
    over all of them, applies the power per component instead of per group, or swaps the group ids."""
    kw = {"window": dict(window=(0, case["G"] - 1)), "power_per_component": dict(power_per_component=True), "swap_groups": dict(swap_groups=True)}[defect]
    assert case["G"] >= 2
    bad = sr.result(case, np.float32, **kw)
    assert sr.compare(bad, sr.result(case)), defect
    assert sr.compare(sr.result(case, np.float32), sr.result(case)) == []


def test_the_float64_chain_separates_the_two_tones():
    """The figures the GPU floor of 25 dB is set against: 38.2 - 38.6 dB and 32.4 - 32.8 dB at every seed and power; 43 and 37 dB with
    four components in two groups; the stems add up to the plain round trip."""
    x, a, b = sr.two_tone_clip()
    assert x.shape == (88200,) and np.isclose(np.abs(a).max(), 0.5, atol=1e-3) and np.isclose(np.abs(b).max(), 0.3, atol=1e-3)
    back = sr.istft(sr.stft(x), len(x))
    assert np.abs(back - x).max() < 1e-14
    for seed in (0, 1, 2):
        for power in (1, 2):
            stems = sr.chain(x, 2, None, power, seed)
            s0, s1 = sr.sdr(stems[0], a), sr.sdr(stems[1], b)
            print(f"seed {seed} power {power}: SDR {s0:.2f} / {s1:.2f} dB")
            assert 38.15 <= s0 <= 38.65 and 32.35 <= s1 <= 32.85
            assert np.abs(stems.sum(axis=0) - back).max() < 1e-15
    for power in (1, 2):
        stems = sr.chain(x, 4, 2, power, 0)
        s0, s1 = sr.sdr(stems[0], a), sr.sdr(stems[1], b)
        print(f"K 4 in 2 groups, power {power}: SDR {s0:.2f} / {s1:.2f} dB")
        assert s0 >= 43 and s1 >= 37
    assert sr.SDR_FLOOR == 25.0


def test_groups_resolution_follows_array_split():
    from maua_stylegan2_amd.audioreactive.decompose import SEPARATE_MAX_GROUPS, _resolve_groups

    assert SEPARATE_MAX_GROUPS == 32
    group, G = _resolve_groups(None, 5)
    assert G == 5 and group.dtype == np.int32 and group.tolist() == [0, 1, 2, 3, 4]
    for K in (1, 3, 8, 9, 32):
        for G in range(1, K + 1):
            group, got = _resolve_groups(G, K)
            want = np.concatenate([np.full(len(run), g) for g, run in enumerate(np.array_split(np.arange(K), G))])
            assert got == G and group.dtype == np.int32 and np.array_equal(group, want) and np.array_equal(group, sr.split_runs(K, G))
    assert _resolve_groups(3, 8)[0].tolist() == [0, 0, 0, 1, 1, 1, 2, 2] and _resolve_groups(np.int64(2), 3)[0].tolist() == [0, 0, 1]
    group, G = _resolve_groups(5, 3)  # array_split's sizes 1, 1, 1, 0, 0: the last two stems are empty
    assert G == 5 and group.tolist() == [0, 1, 2] and np.array_equal(group, sr.split_runs(3, 5))
    for given in ([1, 0, 1, 3], (1, 0, 1, 3), np.array([1, 0, 1, 3]), torch.tensor([1, 0, 1, 3])):
        group, G = _resolve_groups(given, 4)
        assert G == 4 and group.dtype == np.int32 and group.tolist() == [1, 0, 1, 3]  # group 2 is empty: used as given
    for bad in (0, -1, 33, True, 2.0, "ab", [0, 1], [0, 1, 2, 3, 4], [0, -1, 0, 0], [0, 0.5, 1, 1], [0, 1, 2, 32], [[0, 1], [0, 1]], {0: 1}):
        with pytest.raises(ValueError, match="separate:"):
            _resolve_groups(bad, 4)


def test_separate_says_what_to_change():
    import maua_stylegan2_amd.audioreactive as ar

    y = np.zeros(4096, np.float32)
    for kw in (dict(power=3), dict(power=0), dict(power=1.5), dict(power=True), dict(groups=0), dict(groups=33), dict(groups=[0, 1])):
        with pytest.raises(ValueError, match="separate:"):
            ar.separate(y, 22050, **kw)
    for empty in (np.zeros(0, np.float32), torch.zeros(0), []):
        with pytest.raises(ValueError, match="separate: the audio is empty"):
            ar.separate(empty, 22050)
    assert callable(ar.save_audio)


def test_the_entry_refuses_bad_arguments_without_a_device(built_lib):
    """Validation comes before any HIP call: the device pointers are never dereferenced on the host, the group table is a host array."""
    from maua_stylegan2_amd import _lib

    lib = _lib.load()
    fake = 0x1000
    ok = dict(re=fake, im=fake, w=fake, h=fake, group=[0, 1, 1], F=8, T=9, K=3, G=2, power=2, g0=0, n_out=2, out_re=fake, out_im=fake)

    def call(**kw):
        a = dict(ok, **kw)
        table = None if a["group"] is None else (ctypes.c_int32 * len(a["group"]))(*a["group"])
        return lib.maua_nmf_separate_f32(a["re"], a["im"], a["w"], a["h"], table, a["F"], a["T"], a["K"], a["G"], a["power"], a["g0"], a["n_out"],
                                         a["out_re"], a["out_im"], None)

    refused = [dict(re=None), dict(im=None), dict(w=None), dict(h=None), dict(group=None), dict(out_re=None), dict(out_im=None),
               dict(F=0), dict(T=0), dict(K=0), dict(F=-1), dict(T=-3), dict(K=33, group=[0] * 33), dict(G=0), dict(G=-1), dict(G=33),
               dict(F=1 << 16, T=1 << 15), dict(power=0), dict(power=3), dict(power=-1), dict(g0=-1), dict(n_out=0), dict(n_out=-1),
               dict(g0=1, n_out=2), dict(g0=2, n_out=1), dict(n_out=3), dict(g0=2 ** 31 - 1, n_out=2 ** 31 - 1), dict(group=[0, 2, 1]),
               dict(group=[0, -1, 1]), dict(group=[0, 1, 1], G=1), dict(group=[0, 1, 32], G=32, n_out=32)]
    for kw in refused:
        assert call(**kw) == -22, kw
    assert lib.maua_abi_version() == 8 and "maua_nmf_separate_f32" in _lib.exported_symbols()


def test_save_audio_round_trips(tmp_path):
    import maua_stylegan2_amd.audioreactive as ar
    from maua_stylegan2_amd.audioreactive.signal import _read_audio_file

    rng = np.random.default_rng(3)
    x = np.concatenate([rng.uniform(-1, 1, 4000), [1.0, -1.0, 0.0, 0.999985, -0.999985, 1.0 / 65536, -1.0 / 65536]]).astype(np.float32)
    for name, audio in (("array.wav", x), ("tensor.wav", torch.from_numpy(x)), ("double.wav", x.astype(np.float64)), ("list.wav", x.tolist())):
        path = tmp_path / name
        ar.save_audio(path, audio, 22050)
        back, rate = _read_audio_file(path, 22050)
        assert rate == 22050 and back.dtype == np.float32 and back.shape == x.shape
        assert np.abs(back.astype(np.float64) - x.astype(np.float64)).max() <= 1.0 / 32768
    import scipy.io.wavfile

    rate, raw = scipy.io.wavfile.read(str(tmp_path / "array.wav"))
    assert rate == 22050 and raw.dtype == np.int16 and raw.ndim == 1
    loud = np.array([3.0, -2.5, 0.25], np.float32)
    ar.save_audio(tmp_path / "loud.wav", loud, 8000)
    back, _ = _read_audio_file(tmp_path / "loud.wav", 8000)
    assert np.abs(back - np.clip(loud, -1, 1)).max() <= 1.0 / 32768  # clipped, not wrapped
    ar.save_audio(str(tmp_path / "stereo_shaped.wav"), x.reshape(1, -1), 22050)  # flattened to mono
    assert _read_audio_file(tmp_path / "stereo_shaped.wav", 22050)[0].shape == x.shape
