#!/bin/bash
# Two library builds doing the same work: HIP API call counts, then alternating bench.py runs.
# tools/ab_op_scope.sh OUTDIR libimgrec_parent.so libimgrec.so -> OUTDIR/calls_<lib>/ (rocprofv3
# --hip-trace --stats of tools/op_scope_calls.py, one fresh process per library) and OUTDIR/ab.txt
# (six alternating runs each: one query on configs 3 and 2, 1024 queries on config 3).
# Every GPU step runs under a time limit; the first failure ends the script.
set -u -o pipefail
OUT=$1; shift; mkdir -p "$OUT"
export PYTHONPATH=${PYTHONPATH:-$PWD}
for lib in "$@"; do
  IMGREC_LIB_NAME=$lib timeout -k 10 240 rocprofv3 --hip-trace --stats --output-format csv -d "$OUT/calls_$lib" -o calls \
    -- python tools/op_scope_calls.py > "$OUT/calls_$lib.txt" 2>&1 || { tail -20 "$OUT/calls_$lib.txt"; exit 1; }
done
one() {  # lib tag bench-args...
  local lib=$1 tag=$2; shift 2
  IMGREC_LIB_NAME=$lib timeout -k 10 200 python bench.py --gpus 1 "$@" > "$OUT/a.json" 2>> "$OUT/a.err" || { tail -5 "$OUT/a.err"; exit 1; }
  python3 -c "import json;d=json.loads(open('$OUT/a.json').read().strip().splitlines()[-1]);print('$lib $tag ms_per_step', round(d['ms_per_step'],5), 'value', round(d['value'],1))" | tee -a "$OUT/ab.txt"
}
for rep in 1 2 3 4 5 6; do
  for lib in "$@"; do
    one "$lib" cfg3_nq1 --config 3 --nq 1 --steps 500 --warmup 100 || exit 1
    one "$lib" cfg2_nq1 --config 2 --nq 1 --steps 500 --warmup 100 || exit 1
    one "$lib" cfg3_nq1024 --config 3 --nq 1024 --steps 20 --warmup 3 || exit 1
  done
done
