#!/bin/bash
# tools/r06_final.sh OUT_DIR -- the round's bench lines (bench.py --full: all legs), default (c3) and the other presets, into OUT_DIR
# (relative to the repository root)
OUT=${1:?usage: tools/r06_final.sh OUT_DIR}
ROOT=$(cd "$(dirname "$0")/.." && pwd); cd $ROOT; mkdir -p "$OUT"
( time python bench.py --full > $OUT/r06_bench.json 2> $OUT/r06_bench.err ) 2> $OUT/r06_bench.time
for p in c1 c2 c5; do python bench.py --full --preset $p > $OUT/r06_bench_$p.json 2> $OUT/r06_bench_$p.err; done
tail -c 600 $OUT/r06_bench.json; cat $OUT/r06_bench.time
