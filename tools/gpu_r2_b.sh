#!/bin/bash
# round-2 GPU pass B: the default bench line (driver's flags) + rocprofv3 kernel trace of the same command
R=$(cd "$(dirname "$0")/.." && pwd); cd "$R" || exit 1
O=${1:-out}     # output directory
export TMPDIR=/tmp
mkdir -p $O
( time timeout 900 python bench.py --full --gpus 1 --steps 20 --warmup 5 ) > $O/r2b_bench.json 2> $O/r2b_bench.err
echo "bench rc=$?" >> $O/r2b_bench.err
cat $O/r2b_bench.json; tail -5 $O/r2b_bench.err
rm -rf /tmp/prof_b; mkdir -p /tmp/prof_b
( cd /tmp && timeout 900 rocprofv3 --kernel-trace --stats -d /tmp/prof_b -o r2b -- python3 "$R/bench.py" --full --steps 20 --warmup 5 --no-cpu-baseline ) > $O/r2b_prof.log 2>&1
echo "prof rc=$?" >> $O/r2b_prof.log
find /tmp/prof_b -name "*kernel_stats*" -exec cp {} $O/r2b_kernel_stats.csv \;
tail -3 $O/r2b_prof.log; head -25 $O/r2b_kernel_stats.csv | cut -c1-200
