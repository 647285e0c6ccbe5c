"""Static checks of the generated gfx950 code of the pitch tracker (csrc/pitch.hip; no GPU needed: hipcc cross-compiles).  The kernel's
inner loop is 32 VALU instructions on 12 staged values per lane; a spill or a scratch array would put memory traffic into it that nothing
accounts for, and the staged frame has to be read back 16 bytes at a time (one ds_read_b128 per four samples and lag group)."""
import os
import re
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = "/opt/rocm/bin/hipcc"
KERNEL = "yin_kernel"


@pytest.fixture(scope="module")
def pitch_asm(tmp_path_factory):
    if not os.path.exists(HIPCC):
        pytest.skip("hipcc not available")
    dst = str(tmp_path_factory.mktemp("isa") / "pitch.s")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", f"-I{REPO}/include",
                    f"{REPO}/maua_stylegan2_amd/csrc/pitch.hip", "-o", dst], check=True, capture_output=True)
    return open(dst).read()


def _metadata(asm, key):
    names = re.findall(r"^\s+\.name:\s+(\S+)", asm, flags=re.M)
    values = [int(v) for v in re.findall(rf"\.{key}:\s+(\d+)", asm)]
    assert names and len(names) == len(values), (len(names), len(values))
    return {n: v for n, v in zip(names, values) if KERNEL in n}


def test_pitch_kernel_does_not_spill_and_uses_no_scratch(pitch_asm):
    for key in ("vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size"):
        found = _metadata(pitch_asm, key)
        assert found, f"no {KERNEL} in the device code"
        assert all(v == 0 for v in found.values()), (key, found)
    assert "scratch_" not in pitch_asm
    vgprs = _metadata(pitch_asm, "vgpr_count")
    print(f"{KERNEL}: vgpr {vgprs}, sgpr {_metadata(pitch_asm, 'sgpr_count')}, static LDS {_metadata(pitch_asm, 'group_segment_fixed_size')}")
    assert all(v <= 64 for v in vgprs.values()), vgprs  # eight waves a SIMD: a frame's workgroup never waits for registers


def test_pitch_kernel_reads_the_staged_frame_16_bytes_at_a_time(pitch_asm):
    body = pitch_asm[pitch_asm.index(KERNEL):]
    assert re.search(r"^\s+ds_read_b128\s", body, flags=re.M), "the lag window must come from LDS as ds_read_b128"
