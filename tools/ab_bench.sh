#!/bin/bash
# A/B several builds of libfsaempc on ONE device, interleaved rounds (guide rule 24).  Every run has a time limit of its own and
# the first run that fails ends the comparison: nothing more is started on a device after a fault or a hang.
# usage: tools/ab_bench.sh ROUNDS "bench args" lib1.so lib2.so ...
set -o pipefail
R=$1; shift; ARGS=$1; shift
for i in $(seq 1 $R); do
  for L in "$@"; do
    FSAEMPC_LIB=$L timeout -k 10 ${AB_RUN_LIMIT:-180} python bench.py --steps 5 --warmup 1 --no-cpu-baseline $ARGS 2>/dev/null | grep '^{' | python -c "import sys,json; d=json.loads(sys.stdin.read()); print('$L'.split('/')[-1], 'round $i', '%.0f QP/s' % d['value'], 'step %.3f ms' % d['ms_per_step'], 'prep %.3f ms' % d['config']['prep_kernel_ms'], 'kernel %.3f ms' % d['config']['solve_kernel_ms'], 'iters %.2f' % d['config']['mean_ipm_iterations'])" \
      || { echo "$L round $i: run failed (status ${PIPESTATUS[*]}), stopping"; exit 1; }
  done
done
