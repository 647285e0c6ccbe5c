#!/bin/bash
# Round-end extras on the GPU box (through gpurun): the measured maxima of the whole-frame parity tests (pytest -s), bench.py with its side
# configurations, PMC of the split-bf16 side kernel.  Outputs under <outdir>, the first argument (relative to the repository root).
O=${1:?usage: tools/round_extras.sh <outdir>}
mkdir -p "$O"
python -m pytest tests/test_render_gpu.py -q -m gpu -s -k "bench_configuration or config5_bends_1024 or config3_900 or captured_bends_equal" 2>&1 | grep "^\[\|passed\|failed" > $O/parity_full_frames.txt
python -m pytest tests/test_layers_gpu.py -q -m gpu -s -k "split_bf16" 2>&1 | grep "^\[\|^\.\[\|passed\|failed" >> $O/parity_full_frames.txt
cat $O/parity_full_frames.txt
python bench.py --full --steps 20 --no-cpu-baseline > $O/bench.json 2> $O/bench.err
python -c "
import json;p=json.load(open('$O/bench.json'));print(p['value']);print(json.dumps(p['side_configs'],indent=1)[:3000]);print(p['roofline'].get('traffic'))"
bash tools/pmc_microbench.sh $O/pmc_sb sbf16 --split-bf16-min-cout 128 | grep "sbf16_kernel" | grep "GRBM\|MFMA_BUSY\|WAIT_ANY\|WAVE_CYCLES\|WAIT_INST_ANY"
