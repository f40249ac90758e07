#!/usr/bin/env python3
"""Times pgh_king_table and pgh_king_counts (Dataset.king_table / Dataset.king_counts) on pgh_synth_create data
(2 % missing calls), in the style of tools/glm_multi_bench.py.

Cases (samples x variants; "small": a quick check of the tool itself):
  table10k   king_table(min_kinship=0.0884) at 10,000 x 100,000
  table50k   king_table(min_kinship=0.0884) at 50,000 x 100,000
  rect8k     king_counts of one 8,192 x 8,192 rectangle at 50,000 x 100,000 (the transpose still covers all samples;
             the call ends with 1.3 GB of counts copied to pageable host memory)
Before anything is timed a 200 x 200 rectangle over 1,000 variants is compared with a numpy brute force of the same
rows; its result is in every line ("check").  Per case: seconds per call (median of --reps after one warm-up call), and
the int8 rate by the model 2 ops x 5 products x n_var x pairs issued, where pairs issued counts whole 128 x 128 tiles
(the wasted half of the diagonal tiles included), over the 5e15 op/s dense int8 peak.  The rate is the whole call's
(upload, transpose, kernel, copy and sort), not the kernel's: the kernel's own time is in a rocprofv3 kernel trace of
this tool.  One JSON line per case."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import plinking_duck_amd.lib as L  # noqa: E402

INT8_PEAK = 5e15
TILE = L.KING_TILE
CASES = {
    "table10k": ("table", 10_000, 100_000), "table50k": ("table", 50_000, 100_000), "rect8k": ("rect", 50_000, 100_000),
    "small_table": ("table", 3_000, 20_000), "small_rect": ("rect", 3_000, 20_000),
}

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--cases", default="table10k,table50k,rect8k", help="comma list of: " + ", ".join(CASES))
ap.add_argument("--min-kinship", type=float, default=0.0884)
args = ap.parse_args()


def check(ds):
    """One small rectangle against numpy, from the dataset's own rows."""
    n, v = ds.n_samples, min(1000, ds.v_end)
    rows = ds.copy_rows_to_host(0, v)
    codes = ((rows[:, :, None] >> np.array([0, 2, 4, 6], dtype=np.uint8)) & 3).reshape(v, -1)[:, :n]
    i0, i1, j0, j1 = 0, min(200, n), max(0, min(300, n - 200)), min(500, n)
    a, b = codes[:, i0:i1], codes[:, j0:j1]
    f = np.float64
    het_a, het_b = (a == 1).astype(f), (b == 1).astype(f)
    hom_a, hom_b = ((a == 0) | (a == 2)).astype(f), ((b == 0) | (b == 2)).astype(f)
    exp = np.stack([(a != 3).astype(f).T @ (b != 3).astype(f), het_a.T @ het_b,
                    (a == 0).astype(f).T @ (b == 2).astype(f) + (a == 2).astype(f).T @ (b == 0).astype(f),
                    het_a.T @ hom_b, hom_a.T @ het_b]).astype(np.uint32)
    got = ds.king_counts(v_begin=0, v_end=v, i_range=(i0, i1), j_range=(j0, j1))
    return "ok" if np.array_equal(got, exp) else "MISMATCH"


datasets = {}
for name in args.cases.split(","):
    kind, n, m = CASES[name]
    if (n, m) not in datasets:
        for d in datasets.values():
            d[0].close()
        datasets.clear()
        ds = L.Dataset.synth(0, m, n, 20261016, 0.02)
        datasets[(n, m)] = (ds, check(ds))
    ds, checked = datasets[(n, m)]
    if kind == "table":
        tiles = (n + TILE - 1) // TILE
        issued = tiles * (tiles + 1) // 2 * TILE * TILE

        def call():
            return len(ds.king_table(min_kinship=args.min_kinship))
    else:
        side = min(8192, n)
        issued = ((side + TILE - 1) // TILE) ** 2 * TILE * TILE

        def call():
            return int(ds.king_counts(i_range=(0, side), j_range=(n - side, n))[0, 0, 0])
    result = call()  # warm-up (code objects, block cache)
    times = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        result = call()
        times.append(time.perf_counter() - t0)
    t = float(np.median(times))
    ops = 2 * 5 * m * issued
    rec = {
        "case": name, "shape": f"{n}x{m}", "kind": kind, "check": checked, "seconds_per_call": round(t, 6),
        "times": [round(x, 6) for x in times], "pairs_issued": issued, "int8_ops": ops,
        "int8_ops_per_second": ops / t, "int8_peak_fraction": round(ops / t / INT8_PEAK, 4),
    }
    if kind == "table":
        rec["min_kinship"] = args.min_kinship
        rec["pairs_found"] = result
    print(json.dumps(rec), flush=True)
for d in datasets.values():
    d[0].close()
