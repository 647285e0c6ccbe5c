"""Static check of the generated gfx950 code of the two pulse kernels (csrc/pulse.hip; no GPU needed: hipcc cross-compiles), from the
kernels' metadata alone: the complex accumulators of the tempogram kernel and the sums of the synthesis kernel stay in registers — no
spill, no scratch — and the static LDS of both stays under 64 KB."""
import os
import re
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
KERNELS = ("tempogram_peak_kernel", "pulse_synth_kernel")


@pytest.fixture(scope="module")
def pulse_asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    dst = str(tmp_path_factory.mktemp("isa") / "pulse.s")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", f"-I{REPO}/include",
                    f"{REPO}/maua_stylegan2_amd/csrc/pulse.hip", "-o", dst], check=True, capture_output=True)
    return open(dst).read()


def _metadata(asm, key):
    names = re.findall(r"^\s+\.name:\s+(\S+)", asm, flags=re.M)
    values = [int(v) for v in re.findall(rf"\.{key}:\s+(\d+)", asm)]
    assert names and len(names) == len(values), (len(names), len(values))
    return {n: v for n, v in zip(names, values) if any(k in n for k in KERNELS)}


def test_pulse_kernels_do_not_spill_and_use_no_scratch(pulse_asm):
    for key in ("vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size"):
        found = _metadata(pulse_asm, key)
        assert len(found) == len(KERNELS), sorted(found)
        assert all(v == 0 for v in found.values()), (key, found)
    vgpr, sgpr, lds = (_metadata(pulse_asm, k) for k in ("vgpr_count", "sgpr_count", "group_segment_fixed_size"))
    for name in sorted(vgpr):
        print(f"{name}: vgpr {vgpr[name]}, sgpr {sgpr[name]}, static LDS {lds[name]} bytes")
        assert lds[name] < 64 * 1024
