#!/bin/bash
# L7 bench line + rocprofv3 kernel-trace stats of the same command.
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
ROOT=$(pwd)
OUT="${OUT:-$(mktemp -d)}"; mkdir -p "$OUT"; echo "output in $OUT" >&2
set -o pipefail
timeout -k 10 900 python bench.py --full --steps 2 --warmup 1 > "$OUT/bench_l7.json" 2> "$OUT/bench_l7.err"
rc=$?; echo "bench rc=$rc" >&2; tail -5 "$OUT/bench_l7.err" >&2; cat "$OUT/bench_l7.json" >&2
[ $rc -eq 0 ] || exit $rc
cd /tmp && export TMPDIR=/tmp
timeout -k 10 900 rocprofv3 --kernel-trace --stats -d "$OUT/prof_l7" -o run --output-format csv -- \
  python "$ROOT/bench.py" --full --steps 2 --warmup 1 --no-cpu-baseline --no-secondary > "$OUT/prof_l7.out" 2> "$OUT/prof_l7.err"
rc=$?; echo "rocprof rc=$rc" >&2; tail -3 "$OUT/prof_l7.err" >&2
find "$OUT/prof_l7" -name "*stats*" >&2
exit $rc
