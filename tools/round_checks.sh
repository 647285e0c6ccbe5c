#!/bin/bash
# Round-end robustness / end-to-end checks on the GPU box (through gpurun): generate() end to end (config 3, counting sink), the gathered
# region of bench.py on one GPU, the determinism / NaN-poison soak of every conv mode, and the GPU suite with the caching allocator off
# (freed memory is really released: a dangling pointer inside a captured graph faults).  Outputs under <outdir>, the first argument (relative to the repository root).
O=${1:?usage: tools/round_checks.sh <outdir>}
mkdir -p "$O"
python tools/e2e_config3.py --repeat 3 --stage-times > $O/e2e_config3.txt 2>&1; grep "rendered\|E2E\|preprocessing" $O/e2e_config3.txt
python bench.py --full --steps 12 --no-cpu-baseline --no-side-configs --no-breakdown --force-gather > $O/bench_force_gather.json 2> $O/bench_force_gather.err
python -c "
import json;p=json.load(open('$O/bench_force_gather.json'));print('force-gather', p['value'], 'synth-only', p['frames_per_sec_synth_only'])"
python tools/soak_conv.py > $O/soak.txt 2>&1; tail -3 $O/soak.txt
PYTORCH_NO_CUDA_MEMORY_CACHING=1 python -m pytest tests -q -m gpu -x --deselect tests/test_render_gpu.py::test_stylegan1_captured_forward_equals_eager --deselect tests/test_render_gpu.py::test_stylegan1_through_generate_and_render_vs_oracle > $O/pytest_nocache.log 2>&1; tail -2 $O/pytest_nocache.log
