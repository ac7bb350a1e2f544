#!/bin/bash
# usage (on the GPU box, from the repo root): scripts/gpu_check.sh TAG [bench args...]
# runs the GPU parity tests, then bench.py --full with the per-kernel breakdown; everything lands in $OUT_DIR (default out/)
TAG=${1:-x}; shift
OUT_DIR=${OUT_DIR:-out}; mkdir -p $OUT_DIR
timeout -k 10 400 python -m pytest tests -m gpu -q --timeout 240 -p no:cacheprovider > $OUT_DIR/test_$TAG.log 2>&1
echo "tests exit=$?"; tail -3 $OUT_DIR/test_$TAG.log
timeout -k 10 400 python bench.py --full --steps 20 --warmup 5 --breakdown --no-cpu-baseline "$@" > $OUT_DIR/bench_$TAG.json 2> $OUT_DIR/bench_$TAG.err
echo "bench exit=$?"; cat $OUT_DIR/bench_$TAG.json; grep -v amdgpu.ids $OUT_DIR/bench_$TAG.err | head -24
