#!/bin/bash
# Round-end measurement without the test run: the full bench line, rocprofv3 kernel stats of
# the bench (parts = 1), PMC passes + summary.  Raw traces are deleted once summarised, so
# what is left stays small.
# usage: [OUT=dir] tools/gpu_final.sh TAG   (outputs under $OUT, default out/)
set -u
TAG=$1
export TMPDIR=/tmp
OUT=${OUT:-out}
mkdir -p $OUT
if [ "${SKIP_BENCH:-0}" != "1" ]; then
timeout -k 10 600 python -u bench.py --full > $OUT/bench_$TAG.json 2> $OUT/bench_$TAG.err
rc=$?; cat $OUT/bench_$TAG.json; [ $rc -ne 0 ] && { tail -20 $OUT/bench_$TAG.err; exit $rc; }
fi
timeout -k 10 400 rocprofv3 --kernel-trace --stats -d $OUT/prof_$TAG -o run --output-format csv -- python -u bench.py --full --no-cpu --no-latency --steps 5 --warmup 2 --parts 1 --ingest-images 32768 > $OUT/prof_$TAG.log 2>&1
rc=$?; echo "rocprof rc=$rc"; [ $rc -ne 0 ] && exit $rc
find $OUT/prof_$TAG -name '*kernel_trace.csv' -delete
bash tools/pmc_collect.sh $OUT/pmc_$TAG -- python -u bench.py --full --no-cpu --no-latency --ingest-images 0 --jpeg-images 512 --steps 2 --warmup 1 --batch-reps 1 --search-queries 4 --parts 1 || exit $?
python tools/pmc_summary.py $OUT/pmc_$TAG --json $OUT/pmc_$TAG/summary.json --latest $OUT/pmc_$TAG/pmc_latest.json > $OUT/pmc_$TAG/summary.txt
echo "pmc summary rc=$?"
rm -rf $OUT/pmc_$TAG/p[0-9]*/
du -sh $OUT
