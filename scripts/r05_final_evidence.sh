#!/bin/bash
# GPU box: the round-5 evidence in one call -- rocprofv3 statistics and PMC passes (profile_r05.sh), the bench line with every leg (--full), the task
# logs of the three configurations, the forward errors.  Everything lands in gpurun_out/profiles_r05/; copy what is to be judged to profiles/.
export TMPDIR=/tmp
OUT=gpurun_out/profiles_r05
mkdir -p $OUT
bash scripts/profile_r05.sh r05 > gpurun_out/profile_r05.log 2>&1
timeout 900 python3 bench.py --full > $OUT/r05_bench.json 2> $OUT/r05_bench.err
for c in S-metric S-C3 S-C5; do
  rm -f /tmp/dflog.txt
  OKKT_DATAFLOW=1 OKKT_DEBUG_DATAFLOW=16 OKKT_DF_LOG=/tmp/dflog.txt timeout 600 python3 scripts/df_check.py --run $c /tmp/x.npz > /dev/null 2>&1
  python3 scripts/df_log.py /tmp/dflog.txt > $OUT/r05_dataflow_tasks_$c.txt 2>&1
done
: > $OUT/r05_forward_error.txt
for c in S-metric S-C3 S-C5; do timeout 600 python3 scripts/forward_error.py $c 2>&1 | grep "forward error" >> $OUT/r05_forward_error.txt; done
timeout 300 python3 scripts/sc5_err_probe.py S-C5 2>&1 | tail -2 >> $OUT/r05_forward_error.txt
ls -la $OUT; tail -3 $OUT/r05_bench.json | cut -c1-600
