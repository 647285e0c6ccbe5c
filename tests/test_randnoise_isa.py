"""Static checks of the generated gfx950 code of the noise generator (csrc/noise.hip; no GPU needed: hipcc cross-compiles).  The kernel
is a store stream — 89 MB per batch of eight 1024^2 frames — behind ~100 ALU instructions per 16 bytes: a spill or a scratch array would
add memory traffic nothing accounts for, and maps stored dword by dword would quadruple the number of store instructions."""
import os
import re
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
KERNEL = "randn_frames_kernel"


@pytest.fixture(scope="module")
def noise_asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    dst = str(tmp_path_factory.mktemp("isa") / "noise.s")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", f"-I{REPO}/include",
                    f"{REPO}/maua_stylegan2_amd/csrc/noise.hip", "-o", dst], check=True, capture_output=True)
    return open(dst).read()


def _metadata(asm, key):
    names = re.findall(r"^\s+\.name:\s+(\S+)", asm, flags=re.M)
    values = [int(v) for v in re.findall(rf"\.{key}:\s+(\d+)", asm)]
    assert names and len(names) == len(values), (len(names), len(values))
    return {n: v for n, v in zip(names, values) if KERNEL in n}


def test_noise_kernel_does_not_spill_and_uses_no_scratch(noise_asm):
    for key in ("vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size"):
        found = _metadata(noise_asm, key)
        assert found, f"no {KERNEL} in the device code"
        assert all(v == 0 for v in found.values()), (key, found)
    assert "scratch_" not in noise_asm and "buffer_store" not in noise_asm


def test_noise_kernel_stores_the_maps_as_16_byte_vectors(noise_asm):
    body = noise_asm[noise_asm.index(KERNEL):]
    assert re.search(r"^\s+global_store_dwordx4\s", body, flags=re.M), "the maps must leave as global_store_dwordx4"
    # the frame source's pointer / stride words are ordinary 8-byte vector stores of one lane each
    assert len(re.findall(r"^\s+global_store_dwordx2\s", body, flags=re.M)) >= 2
