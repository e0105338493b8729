#!/bin/bash
# usage on the GPU box: bash tools/gpu_bench.sh <tag>
set -x
tag=${1:-r01}
OUT=${OUT:-out}; R=$PWD
mkdir -p $OUT/$tag
python bench.py --full > $OUT/$tag/bench.json 2> $OUT/$tag/bench.err
tail -c 3000 $OUT/$tag/bench.json
cd /tmp && export TMPDIR=/tmp
rocprofv3 --kernel-trace --stats --output-format csv -d $R/$OUT/$tag/prof -- python3 $R/bench.py --steps 30 --warmup 10 --no-cpu-baseline > $R/$OUT/$tag/prof.log 2>&1
cd $R
find $OUT/$tag/prof -name "*stats*" | head
