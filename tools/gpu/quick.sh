#!/bin/bash
# Shorter GPU session: GPU parity tests + the full bench record (no rocprof).
# Usage: OUT=<results dir> bash tools/gpu/quick.sh <tag> [pytest -k expr]
TAG=${1:-q}
KEXPR=${2:-}
OUT=${OUT:?set OUT to the directory the results go to}
mkdir -p $OUT
export TMPDIR=/tmp
if [ -n "$KEXPR" ]; then
  timeout 900 python -m pytest tests -m gpu -q --tb=short -p no:cacheprovider -k "$KEXPR" > $OUT/${TAG}_pytest_gpu.log 2>&1
else
  timeout 1200 python -m pytest tests -m gpu -q --tb=short -p no:cacheprovider > $OUT/${TAG}_pytest_gpu.log 2>&1
fi
echo "pytest rc=$?" >> $OUT/${TAG}_pytest_gpu.log
timeout 900 python bench.py --full --layer-table --save-plan $OUT/${TAG}_plan.json --detail-file $OUT/${TAG}_bench_detail.json > $OUT/${TAG}_bench.json 2> $OUT/${TAG}_bench.err; echo "bench rc=$?" >> $OUT/${TAG}_bench.err
tail -15 $OUT/${TAG}_pytest_gpu.log; head -c 2500 $OUT/${TAG}_bench.json; tail -5 $OUT/${TAG}_bench.err
