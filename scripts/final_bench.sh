#!/bin/bash
# the bench with every leg (--full) at --steps 20 --warmup 5 and at its defaults, rocprofv3 kernel stats
# of the bench and the PMC FETCH/WRITE passes of the sweep kernel (scripts/pmc.sh) and the request-size passes
# (scripts/pmc_sizes.sh) -> $OUT (default bench_out/)
cd $GRAFT_REPO_ROOT
ROOTDIR=$(pwd); export TMPDIR=/tmp
OUT=${OUT:-bench_out}; mkdir -p $OUT
timeout -k 10 300 python -u bench.py --gpus 1 --steps 20 --warmup 5 --full > $OUT/bench_driver_shape.json 2> $OUT/bench_driver_shape.err || { tail -20 $OUT/bench_driver_shape.err; exit 1; }
cut -c1-600 $OUT/bench_driver_shape.json
timeout -k 10 400 python -u bench.py --full > $OUT/bench_default.json 2> $OUT/bench_default.err || { tail -20 $OUT/bench_default.err; exit 1; }
cut -c1-300 $OUT/bench_default.json
(cd /tmp && timeout -k 10 300 rocprofv3 --kernel-trace --stats --output-format csv -d $ROOTDIR/$OUT/prof_final -o run -- python3 $ROOTDIR/bench.py --full --steps 60 --warmup 10 --no-cpu-baseline --mcmc-iters 0 > $ROOTDIR/$OUT/bench_prof_final.json 2> $ROOTDIR/$OUT/bench_prof_final.err) || exit 1
f=$(find $OUT/prof_final -name "*kernel_stats.csv" | head -1); head -6 "$f" | cut -c1-200
bash scripts/pmc.sh && bash scripts/pmc_sizes.sh
