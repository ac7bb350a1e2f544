#!/bin/bash
# usage (GPU box): scripts/bench_rows.sh TAG [bench args]  -> $OUT_DIR/bench_TAG.json / .err (per-kernel table + per-op rows; OUT_DIR defaults to out/)
cd $GRAFT_REPO_ROOT
TAG=$1; shift
OUT_DIR=${OUT_DIR:-out}; mkdir -p $OUT_DIR
RCV_BENCH_ROWS=1 timeout -k 10 500 python bench.py --full --steps 20 --warmup 5 --breakdown --no-cpu-baseline "$@" > $OUT_DIR/bench_$TAG.json 2> $OUT_DIR/bench_$TAG.err
echo "bench exit=$?"; cat $OUT_DIR/bench_$TAG.json; grep -v amdgpu.ids $OUT_DIR/bench_$TAG.err | head -30
