#!/bin/bash
# plink_score by weight-column count, then plink_pca, on the GPU box: tools/score_sweep.sh <tag> [out-dir]
cd "$GRAFT_REPO_ROOT"
TAG=${1:-sweep}
OUT=${2:-${TMPDIR:-/tmp}}/$TAG
mkdir -p "$OUT"
for c in 1 2 4 8 16; do
  python bench.py --full --workload score --score-cols $c --cpu-seconds 0 > "$OUT/score$c.json" 2> "$OUT/score$c.err" || { tail -3 "$OUT/score$c.err"; exit 1; }
done
python bench.py --full --workload pca --steps 2 --warmup 1 --cpu-seconds 0 > "$OUT/pca.json" 2> "$OUT/pca.err" || { tail -3 "$OUT/pca.err"; exit 1; }
python - "$OUT" <<'PY'
import json, sys, glob
for f in sorted(glob.glob(f"{sys.argv[1]}/*.json"), key=lambda p: (len(p), p)):
    d = json.load(open(f)); r = d["roofline"]
    print(f"{d['metric']:70s} {d['ms_per_step']:8.2f} ms  verified={d['verified']}  {r['bound']} frac {r['frac']:.3f}")
PY
