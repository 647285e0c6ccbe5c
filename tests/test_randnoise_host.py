"""CPU: the definition of the counter-based noise (include/maua_hip.h, maua_randn_frames_f32) as restated in tests/philox_ref.py, and the
argument refusals of the C entry (validation runs before any HIP call).

Moment conditions (each <= 4 standard errors; conditions, not measurements).  The float64 reference alone, over the 2^22 values of seed
0x123456789ABCDEF0, frames 0-1 x slots 0-1, hw = 2^20, gives on the CPU
    |mean| sqrt(N) 0.643   |var - 1| sqrt(N/2) 0.365   |skew| sqrt(N/6) 0.006   |excess kurtosis| sqrt(N/24) 0.620
    lag-1 autocorrelation sqrt(N) 1.638   lag-4 0.173   largest correlation between two maps sqrt(hw) 1.400   max |z| 5.630
so this seed stays inside the bound with the 23-bit mapping and is kept."""
import numpy as np
import pytest

import philox_ref as pr

SEED = 0x123456789ABCDEF0


def _hex(words):
    return " ".join(f"{int(w):08x}" for w in words)


def test_philox4x32_10_known_answers():
    """The three known-answer vectors of the Random123 distribution (kat_vectors, philox4x32 10 rounds)."""
    assert _hex(pr.philox4x32_10((0, 0, 0, 0), (0, 0))) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    ones = 0xFFFFFFFF
    assert _hex(pr.philox4x32_10((ones,) * 4, (ones,) * 2)) == "408f276d 41c83b0e a20bc7c6 6d5451fd"
    assert _hex(pr.philox4x32_10((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0))) == \
        "d16cfe09 94fdcceb 5001e420 24126ea1"


def test_uniform_mapping_is_exact_in_float32_and_open():
    x = np.array([0, 1, 511, 512, 0xFFFFFFFF, 0xFFFFFE00, 0x80000000], dtype=np.uint64)
    u64 = ((x >> np.uint64(9)).astype(np.float64) + 0.5) * 2.0 ** -23
    u32 = ((x >> np.uint64(9)).astype(np.float32) + np.float32(0.5)) * np.float32(2.0 ** -23)
    assert np.array_equal(u32.astype(np.float64), u64)
    assert u64.min() == 2.0 ** -24 and u64.max() == 1.0 - 2.0 ** -24 and float(u32.max()) < 1.0
    assert abs(pr.Z_MAX - 5.768) < 1e-3


@pytest.mark.parametrize("hw", [1, 3, 5, 35])
def test_prefix_property(hw):
    full = pr.noise_map(SEED, 7, 3, 64)
    assert np.array_equal(pr.noise_map(SEED, 7, 3, hw), full[:hw])


def test_maps_depend_on_seed_frame_and_slot():
    base = pr.noise_map(SEED, 5, 2, 256)
    for other in (pr.noise_map(SEED + 1, 5, 2, 256), pr.noise_map(SEED ^ (1 << 40), 5, 2, 256), pr.noise_map(SEED, 6, 2, 256),
                  pr.noise_map(SEED, 5, 3, 256)):
        assert not np.any(other == base)
    assert np.array_equal(pr.noise_map(SEED, 5, 2, 256), base)


def test_moments_of_the_float64_reference():
    maps = np.stack([pr.noise_map(SEED, f, s, 1 << 20) for f in (0, 1) for s in (0, 1)])
    stats, z_max = pr.moment_statistics(maps)
    print({k: round(float(v), 3) for k, v in stats.items()}, z_max)
    for name, value in stats.items():
        assert value <= 4.0, (name, value)
    assert z_max <= pr.Z_MAX


def test_entry_refuses_bad_arguments_without_gpu(built_lib):
    from maua_stylegan2_amd import _lib

    lib = _lib.load()
    assert _lib.ABI_VERSION >= 7 and _lib.MAX_NOISE_SLOTS == 32
    import ctypes as ct
    assert ct.sizeof(_lib.RandnSlot) == 16
    fake = 0x1000  # never dereferenced: every call below is rejected during validation
    call = lambda table=fake, n=1, batch=1, seed=SEED, frame0=0, src=None: lib.maua_randn_frames_f32(table, n, batch, seed, frame0, src, None)  # noqa: E731
    assert call(table=None) == -22
    assert call(n=0) == -22 and call(n=33) == -22 and call(n=-1) == -22
    assert call(batch=0) == -22 and call(batch=-3) == -22
    assert call(frame0=-1) == -22 and call(frame0=-1, src=fake) == -22
