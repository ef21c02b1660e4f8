# Full BASELINE config bench (bench.py --full: every figure of the line) + rocprofv3 kernel
# stats of a shorter run of the plain command.  Output under $OUT_DIR (default out/).
set -o pipefail
cd "$(dirname "$0")/.."
export TMPDIR=/tmp
TAG=${TAG:-r01}
O=${OUT_DIR:-out}
mkdir -p $O
timeout -k 10 900 python bench.py --full ${BENCH_ARGS:-} > $O/bench_full_$TAG.json 2> $O/bench_full_$TAG.err
rc=$?; cat $O/bench_full_$TAG.json; tail -5 $O/bench_full_$TAG.err; echo "bench rc=$rc"
[ $rc -eq 0 ] || exit $rc
rm -rf /tmp/prof
timeout -k 10 900 rocprofv3 --kernel-trace --stats --output-format csv -d /tmp/prof -o trace -- \
    python3 bench.py --steps 1 --warmup 0 > $O/bench_prof_$TAG.json 2> $O/bench_prof_$TAG.err
rc=$?; echo "rocprof rc=$rc"; tail -3 $O/bench_prof_$TAG.err
mkdir -p $O/prof_$TAG
find /tmp/prof -name '*stats*.csv' -exec cp {} $O/prof_$TAG/ \;
ls -la $O/prof_$TAG
cat $O/prof_$TAG/*kernel_stats*.csv 2>/dev/null | head -20
exit $rc
