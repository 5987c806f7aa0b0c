# rocprofv3 kernel trace (+stats) of short bench runs with every leg: 1 chain and 3 chains -> $OUT
# (default bench_out/).
cd $GRAFT_REPO_ROOT
ROOTDIR=$(pwd)
export TMPDIR=/tmp
OUT=${OUT:-bench_out}; mkdir -p $OUT
for C in 1 3; do
  (cd /tmp && timeout -k 10 400 rocprofv3 --kernel-trace --stats --output-format csv -d "$ROOTDIR/$OUT/prof_c$C" -o run -- \
      python3 "$ROOTDIR/bench.py" --full --steps 40 --warmup 10 --no-cpu-baseline --no-single-chain --chains $C > "$ROOTDIR/$OUT/prof_c$C.json" 2> "$ROOTDIR/$OUT/prof_c$C.err") || exit 1
  f=$(find $OUT/prof_c$C -name "*kernel_stats.csv" | head -1)
  echo "== C=$C $f"; head -12 "$f" | cut -c1-220
done
