cd "$(dirname "$0")/.."; export TMPDIR=/tmp
OUT=${OUT:-bench_out}; mkdir -p $OUT
for k in 1 2; do timeout -k 10 300 python -u bench.py --gpus 1 --steps 20 --warmup 5 --full > $OUT/b200_$k.json 2> $OUT/b200_$k.err || { tail -5 $OUT/b200_$k.err; exit 1; }; python3 -c "import json; d=json.loads(open('$OUT/b200_$k.json').read().strip().splitlines()[-1]); print(round(d['value']), d['secondary'])"; done
