#!/bin/bash
# One GPU call: parity tests, the full bench line, rocprofv3 kernel-trace stats of the bench.
# usage: [OUT=dir] tools/gpu_check.sh TAG [bench args...]   (outputs under $OUT, default out/)
set -u
TAG=$1; shift
export TMPDIR=/tmp
OUT=${OUT:-out}
mkdir -p $OUT
timeout -k 10 600 python -u -m pytest tests -m gpu -x -q --timeout 120 --timeout-method thread > $OUT/pytest_$TAG.log 2>&1
rc=$?; tail -5 $OUT/pytest_$TAG.log; [ $rc -ne 0 ] && exit $rc
timeout -k 10 600 python -u bench.py --full "$@" > $OUT/bench_$TAG.json 2> $OUT/bench_$TAG.err
rc=$?; cat $OUT/bench_$TAG.json; [ $rc -ne 0 ] && { tail -20 $OUT/bench_$TAG.err; exit $rc; }
timeout -k 10 400 rocprofv3 --kernel-trace --stats -d $OUT/prof_$TAG -o run --output-format csv -- python -u bench.py --full --no-cpu --no-latency --steps 5 --warmup 2 --parts 1 --ingest-images 32768 > $OUT/prof_$TAG.log 2>&1
rc=$?; echo "rocprof rc=$rc"; exit $rc
