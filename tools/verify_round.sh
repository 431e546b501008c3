#!/bin/bash
# Runs on the GPU box (through gpurun): the GPU test suite, smoke(), and the default bench line inside a rocprofv3 kernel trace
# (the short form of tools/profile_round.sh: no PMC passes, no extra configs).   usage: tools/verify_round.sh <tag>
TAG=${1:-verify}
R=${GRAFT_REPO_ROOT:-$(pwd)}
O=$R/gpurun_out/$TAG
mkdir -p $O
export TMPDIR=/tmp
cd $R
timeout 1200 python -m pytest tests -m gpu -x -q > $O/pytest_gpu.log 2>&1; tail -3 $O/pytest_gpu.log
timeout 300 python -c "import __graft_entry__ as g; g.smoke()" > $O/smoke.log 2>&1; tail -2 $O/smoke.log
cd /tmp
rm -rf /tmp/kt
timeout 900 rocprofv3 --kernel-trace --stats -d /tmp/kt -- python $R/bench.py --full > $O/bench_stdout.txt 2> $O/bench_default.err
grep '^{"metric"' $O/bench_stdout.txt | tail -1 > $O/bench_default.json
cut -c1-600 $O/bench_default.json
DB=$(find /tmp/kt -name "*results.db" | paste -sd, -)
python $R/tools/rocpd_summary.py "$DB" $O/kernel_trace_stats.csv "python bench.py --full (default: 32768 streams, 20 steps + 3 warm-up; MI355X); same run as bench_default.json"
head -8 $O/kernel_trace_stats.csv
