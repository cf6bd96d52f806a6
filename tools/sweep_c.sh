#!/bin/bash
# waves per individual (NGHMM_FAST_C) against ms per EM iteration: bash tools/sweep_c.sh "<C values>" [bench args]
CS=${1:-"40 49 56 64"}; shift
for c in $CS; do
  NGHMM_FAST_C=$c python bench.py --full --steps 20 --warmup 5 --no_cpu_baseline --no_exact_line --no_check "$@" \
    2>/dev/null | python -c "
import json,sys
d=json.loads(sys.stdin.read().strip().splitlines()[-1])
print('$c', round(d['ms_per_step'],3), {k:round(v,3) for k,v in d['per_step_kernel_ms'].items()}, flush=True)
"
done
