#!/bin/bash
# Round measurement on one GPU box: parity tests, the full bench line, kernel-trace stats,
# then PMC passes (separate runs, kernel-trace only) over a short bench.
# usage: [OUT=dir] tools/gpu_round.sh TAG   (outputs under $OUT, default out/)
set -u
TAG=$1
export TMPDIR=/tmp
export OUT=${OUT:-out}
mkdir -p $OUT
bash tools/gpu_check.sh "$TAG" || exit $?
bash tools/pmc_collect.sh $OUT/pmc_$TAG -- python -u bench.py --full --no-cpu --steps 2 --warmup 1 --batch-reps 1 --search-queries 4 --parts 1 || exit $?
python tools/pmc_summary.py $OUT/pmc_$TAG --json $OUT/pmc_$TAG/summary.json --latest $OUT/pmc_$TAG/pmc_latest.json > $OUT/pmc_$TAG/summary.txt
echo "pmc summary rc=$?"
