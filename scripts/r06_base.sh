cd "$(dirname "$0")/.."; export TMPDIR=/tmp; OUT=${OUT:-bench_out}; mkdir -p $OUT
timeout -k 10 300 python -u bench.py --gpus 1 --steps 20 --warmup 5 --full --no-cpu-baseline > $OUT/r06_base_bench.json 2> $OUT/r06_base_bench.err || exit 1
cut -c1-400 $OUT/r06_base_bench.json
timeout -k 10 300 python -u scripts/timeline.py > $OUT/r06_base_timeline.txt 2>&1 || exit 1
tail -30 $OUT/r06_base_timeline.txt
