#!/bin/bash
# ON THE GPU BOX: same-box A/B of library build variants (build/libtransgo_hip_<v>.so copied over the product library in this scratch
# copy only; "prod" = the product build), bench lines interleaved, REPS (default 3) repetitions.
#   scripts/ab_lines.sh <tag> "<bench.py arguments>" <variant> [<variant> ...]
# One line per run in $AB_OUT/ab_<tag>.txt (AB_OUT: a directory the caller keeps, default build/ab): arm, value, ms_per_step, roofline.avg_launch_ms, roofline.frac and the error counters
# (extra.tree_errors / fp16_overflows / truncated_tree_blocks), the columns of profiles/ab_*.txt.
set -o pipefail
cd "${GRAFT_REPO_ROOT:-.}"
tag=$1; args=$2; shift 2
out=${AB_OUT:-build/ab}
mkdir -p $out
cp transgo_amd/libtransgo_hip.so /tmp/prod.so
for rep in $(seq ${REPS:-3}); do
  for v in "$@" prod; do
    if [ $v = prod ]; then cp /tmp/prod.so transgo_amd/libtransgo_hip.so; else cp build/libtransgo_hip_$v.so transgo_amd/libtransgo_hip.so; fi
    timeout -k 10 400 python3 bench.py --no-cpu-baseline $args 2> $out/ab_$tag.err | python3 -c "import sys,json; d=json.loads(sys.stdin.read().strip().splitlines()[-1]); r=d['roofline']; e=d['extra']; print('$v', 'value', d['value'], 'ms_per_step', d['ms_per_step'], 'avg_launch_ms', r['avg_launch_ms'], 'frac', r['frac'], 'errs', e['tree_errors'], e['fp16_overflows'], e['truncated_tree_blocks'])" | tee -a $out/ab_$tag.txt || { cp /tmp/prod.so transgo_amd/libtransgo_hip.so; exit 1; }
  done
done
cp /tmp/prod.so transgo_amd/libtransgo_hip.so
