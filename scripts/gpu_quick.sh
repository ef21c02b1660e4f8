# parity suite + full-config bench (bench.py --full without the CPU baseline) — the inner
# optimisation loop.  Output under $OUT_DIR (default out/).
set -o pipefail
cd "$(dirname "$0")/.."
export TMPDIR=/tmp
TAG=${TAG:-quick}
O=${OUT_DIR:-out}
mkdir -p $O
timeout -k 10 900 python -m pytest tests -m gpu -x -q -p no:cacheprovider > $O/pytest_$TAG.log 2>&1
rc=$?; tail -5 $O/pytest_$TAG.log; echo "pytest rc=$rc"
[ $rc -eq 0 ] || exit $rc
timeout -k 10 900 python bench.py --full --no-cpu-baseline ${BENCH_ARGS:-} > $O/bench_$TAG.json 2> $O/bench_$TAG.err
rc=$?; cat $O/bench_$TAG.json; tail -3 $O/bench_$TAG.err; echo "bench rc=$rc"
exit $rc
