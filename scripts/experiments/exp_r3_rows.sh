#!/bin/bash
# per-kernel table of the headline step (HIP-event timed op by op)
cd $GRAFT_REPO_ROOT
OUT_DIR=${OUT_DIR:-out}; mkdir -p $OUT_DIR
RCV_BENCH_ROWS=1 timeout -k 10 400 python bench.py --full --steps 20 --warmup 5 --no-cpu-baseline --breakdown > $OUT_DIR/rows.json 2> $OUT_DIR/rows.err
echo "exit=$?"; grep -v "^[BF] " $OUT_DIR/rows.err | tail -45
