"""Static check of the generated gfx950 code of csrc/feedback.hip (no GPU needed: hipcc cross-compiles), from the kernels' metadata alone:
the four instances — the warp kernel and the still kernel, each with 16-byte and with scalar accesses — keep everything in registers (no
spill, no scratch), use no LDS, and stay at eight waves a SIMD."""
import os
import re
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIPCC = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
N_KERNELS = 4


@pytest.fixture(scope="module")
def feedback_asm(tmp_path_factory):
    dst = str(tmp_path_factory.mktemp("isa") / "feedback.s")
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-S", "--cuda-device-only", f"-I{REPO}/include",
                    f"{REPO}/maua_stylegan2_amd/csrc/feedback.hip", "-o", dst], check=True, capture_output=True)
    return open(dst).read()


def _metadata(asm, key):
    names = re.findall(r"^\s+\.name:\s+(\S+)", asm, flags=re.M)
    values = [int(v) for v in re.findall(rf"\.{key}:\s+(\d+)", asm)]
    assert names and len(names) == len(values), (len(names), len(values))
    return dict(zip(names, values))


def test_feedback_kernels_keep_everything_in_registers(feedback_asm):
    vgpr, sgpr = _metadata(feedback_asm, "vgpr_count"), _metadata(feedback_asm, "sgpr_count")
    assert len(vgpr) == N_KERNELS, sorted(vgpr)
    kinds = {k: sorted(int(re.search(r"ILb([01])E", n).group(1)) for n in vgpr if k in n) for k in ("feedback_warp_kernel", "feedback_still_kernel")}
    assert kinds == {"feedback_warp_kernel": [0, 1], "feedback_still_kernel": [0, 1]}
    for key in ("vgpr_spill_count", "sgpr_spill_count", "private_segment_fixed_size", "group_segment_fixed_size"):
        found = _metadata(feedback_asm, key)
        assert len(found) == N_KERNELS and all(v == 0 for v in found.values()), (key, {n: v for n, v in found.items() if v})
    for name in sorted(vgpr):
        print(f"{name}: vgpr {vgpr[name]}, sgpr {sgpr[name]}")
        # Both kernels are memory-bound: what hides the gather's latency is waves in flight, so every instance stays at 64 VGPRs, eight
        # waves a SIMD.  The build gives the vector warp kernel 56 (4 pixels x 3 channels of the frame, and per pixel four tap offsets,
        # two weights and up to four taps in flight), the scalar one 42, the still kernel 32 / 16 (12 state values, 12 of the frame
        # and the addresses); the still kernel gets the margin of a few registers a compiler update may cost, the warp kernel the
        # occupancy step it must not cross.
        assert vgpr[name] <= (64 if "feedback_warp_kernel" in name else 40), (name, vgpr[name])
        assert sgpr[name] <= 100, (name, sgpr[name])  # (the row, and the still run's rows in flight, live in scalar registers)


def test_the_source_has_no_inline_assembly():
    src = open(f"{REPO}/maua_stylegan2_amd/csrc/feedback.hip").read()
    assert "asm" not in re.sub(r"//.*", "", src)
