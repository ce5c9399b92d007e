#!/bin/bash
# round-2 GPU pass A: full GPU test-suite, smoke, the default bench line (driver's flags)
R=$(cd "$(dirname "$0")/.." && pwd); cd "$R" || exit 1
O=${1:-out}     # output directory
export TMPDIR=/tmp
mkdir -p $O
( time timeout 1500 python -m pytest tests -m gpu -x -q ) > $O/r2a_tests.log 2>&1
echo "tests rc=$?" >> $O/r2a_tests.log
( time timeout 300 python -c 'import __graft_entry__ as g; g.smoke()' ) > $O/r2a_smoke.log 2>&1
echo "smoke rc=$?" >> $O/r2a_smoke.log
( time timeout 900 python bench.py --full --gpus 1 --steps 20 --warmup 5 ) > $O/r2a_bench.json 2> $O/r2a_bench.err
echo "bench rc=$?" >> $O/r2a_bench.err
timeout 120 python bench.py --full --gpus 2 --steps 2 --warmup 1 > $O/r2a_bench_gpus2.out 2>&1
echo "gpus2 rc=$?" >> $O/r2a_bench_gpus2.out
tail -3 $O/r2a_tests.log; tail -3 $O/r2a_smoke.log; cat $O/r2a_bench.json; tail -5 $O/r2a_bench.err; tail -2 $O/r2a_bench_gpus2.out
