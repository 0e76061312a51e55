#!/bin/bash
# parity tests (incl. multigrid) -> bench L7 (MG) -> rocprofv3 stats (trace kept in /tmp, only summaries copied)
cd "${GRAFT_REPO_ROOT:-$(dirname "$0")/..}"
ROOT=$(pwd)
OUT="${OUT:-$(mktemp -d)}"; mkdir -p "$OUT"; echo "output in $OUT" >&2
step() {  # name timeout cmd...
  local name=$1 t=$2; shift 2
  echo "=== $name" >&2
  timeout -k 10 "$t" "$@" > "$OUT/$name.out" 2> "$OUT/$name.err"
  local rc=$?
  echo "=== $name rc=$rc" >&2; tail -n 12 "$OUT/$name.out" >&2; tail -n 6 "$OUT/$name.err" >&2
  if [ $rc -ne 0 ] && [ $rc -ne 1 ]; then echo "stop after $name" >&2; exit $rc; fi
}
step pytest_gpu 900 python -m pytest tests -m gpu -x -q
step bench_l7 900 python bench.py --full
cd /tmp && export TMPDIR=/tmp
echo "=== rocprof" >&2
timeout -k 10 900 rocprofv3 --kernel-trace --stats -d /tmp/prof_l7 -o run --output-format csv -- \
  python "$ROOT/bench.py" --full > "$OUT/prof_l7.out" 2> "$OUT/prof_l7.err"
rc=$?; echo "rocprof rc=$rc" >&2; tail -3 "$OUT/prof_l7.err" >&2
mkdir -p "$OUT/prof_l7"
find /tmp/prof_l7 -name "*stats*.csv" -exec cp {} "$OUT/prof_l7/" \;
ls -la "$OUT/prof_l7" >&2
exit $rc
