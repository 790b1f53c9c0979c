#!/bin/bash
# One GPU-box session: smoke, GPU parity tests, the full bench record (with per-layer table), rocprof kernel stats.
# Usage: OUT=<results dir> bash tools/gpu/round.sh [tag]
TAG=${1:-r01}
R=$(pwd)
OUT=${OUT:?set OUT to the directory the results go to}
mkdir -p $OUT
OUT=$(cd $OUT && pwd)
export TMPDIR=/tmp
( rocminfo | grep -E "Marketing Name|gfx|Compute Unit" | head -8; lscpu | grep -E "Model name|^CPU\(s\)|Thread|Core|Socket" ) > $OUT/${TAG}_hw.txt 2>&1
timeout 300 python -c "import __graft_entry__ as g; g.smoke()" > $OUT/${TAG}_smoke.log 2>&1; echo "smoke rc=$?" >> $OUT/${TAG}_smoke.log
timeout 1500 python -m pytest tests -m gpu -q --tb=short -p no:cacheprovider > $OUT/${TAG}_pytest_gpu.log 2>&1; echo "pytest rc=$?" >> $OUT/${TAG}_pytest_gpu.log
timeout 900 python bench.py --full --layer-table --save-plan $OUT/${TAG}_plan.json --detail-file $OUT/${TAG}_bench_detail.json > $OUT/${TAG}_bench.json 2> $OUT/${TAG}_bench.err; echo "bench rc=$?" >> $OUT/${TAG}_bench.err
cd /tmp && timeout 600 rocprofv3 --kernel-trace --stats --output-format csv -d $OUT/${TAG}_prof -o ${TAG} -- python $R/bench.py --steps 20 --warmup 5 --no-cpu-baseline --no-secondary --load-plan $OUT/${TAG}_plan.json > $OUT/${TAG}_prof_bench.json 2> $OUT/${TAG}_prof.err; echo "rocprof rc=$?" >> $OUT/${TAG}_prof.err
cd $R
(rocprofv3 -L 2>/dev/null | grep -E "^\s*(Name|Counter_Name|gpu|  *[A-Z_0-9]+)" | head -400) > $OUT/${TAG}_counters.txt 2>&1
find $OUT/${TAG}_prof -name "*stats*" | head; du -sh $OUT
# keep only the small stats summaries (the full kernel trace can be large)
find $OUT/${TAG}_prof -type f ! -name "*stats*" -size +2M -delete
tail -3 $OUT/${TAG}_smoke.log; tail -15 $OUT/${TAG}_pytest_gpu.log; cat $OUT/${TAG}_bench.json | head -c 3000; tail -5 $OUT/${TAG}_bench.err
