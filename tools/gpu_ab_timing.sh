cd "${GRAFT_REPO_ROOT}"
export OUT="${OUT:-$(mktemp -d)}"; mkdir -p "$OUT"; echo "output in $OUT" >&2
for i in 1 2; do
  timeout -k 10 300 python bench.py --full --no-cpu-baseline --no-secondary --warmup 5 --steps 20 --steady-after 0 > "$OUT/kt$i.out" 2>/dev/null || exit 1
  timeout -k 10 300 python bench.py --full --no-cpu-baseline --no-secondary --warmup 5 --steps 20 --steady-after 0 --no-kernel-timing > "$OUT/nokt$i.out" 2>/dev/null || exit 1
done
python - <<'PY'
import json, os
for n in ("kt1","nokt1","kt2","nokt2"):
    r=json.loads(open(os.path.join(os.environ["OUT"], f"{n}.out")).read().strip().splitlines()[-1])
    print(n, round(r["value"],2))
PY
