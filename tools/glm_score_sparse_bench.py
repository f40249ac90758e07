#!/usr/bin/env python3
"""Times pgh_glm_score_sparse (Dataset.glm_score_sparse) on the sparse-resident dataset of a rare-variant file and, in
the same run, pgh_glm_sparse (Dataset.glm_sparse) over the same rows: the linear fit is the figure to set the score
test against, since both walk the same entries (pgh_glm_score_sparse).  A third timing, a call
over one variant, is the cost of the null fit (the Newton steps of the covariates-only model), which every call pays.

The file is tools/glm_sparse_bench.py's: written straight from carrier lists (tools/sparse_bench.py), never through a
dense matrix, and shared with it when --dir is the same.  The phenotype is Bernoulli with about --cases cases and
depends on the covariates.  Per call: seconds (median of --reps after one warm-up call) and entries per second.
One JSON line.

usage: python tools/glm_score_sparse_bench.py [--samples 500000] [--variants 1000000] [--rate 0.001] [--covar 10]
                                              [--cases 0.2] [--reps 3] [--dir DIR]"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import plinking_duck_amd.lib as L  # noqa: E402
from tools.sparse_bench import carrier_rows, write_carrier_pfile  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--samples", type=int, default=500_000)
ap.add_argument("--variants", type=int, default=1_000_000)
ap.add_argument("--rate", type=float, default=0.001)
ap.add_argument("--covar", type=int, default=10)
ap.add_argument("--cases", type=float, default=0.2)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--dir", default="/tmp/glm_sparse_bench")
args = ap.parse_args()

m, n, k = args.variants, args.samples, args.covar
os.makedirs(args.dir, exist_ok=True)
prefix = os.path.join(args.dir, f"carriers_{m}x{n}")
t0 = time.perf_counter()
if not os.path.exists(prefix + ".pgen"):
    write_carrier_pfile(prefix, m, n, carrier_rows(m, n, args.rate, 13))
rec = {"shape": f"{m}x{n}", "carrier_rate_max": 2 * args.rate, "covariates": k,
       "file_bytes": os.path.getsize(prefix + ".pgen"), "write_s": round(time.perf_counter() - t0, 1)}

rng = np.random.default_rng(1)
z = rng.standard_normal((k, n)) if k else None
eta = math.log(args.cases / (1 - args.cases)) + (z.sum(axis=0) * 0.2 if k else 0.0)
y = (rng.random(n) < 1 / (1 + np.exp(-eta))).astype(np.float64)
y[rng.random(n) < 0.01] = np.nan
rec["case_fraction"] = round(float(np.nanmean(y)), 4)


def timed(call):
    out = call()  # warm-up (scratch growth, code objects)
    times = []
    for _ in range(args.reps):
        t = time.perf_counter()
        out = call()
        times.append(time.perf_counter() - t)
    return out, float(np.median(times)), [round(x, 6) for x in times]


t0 = time.perf_counter()
sp = L.Dataset.open(prefix + ".pgen", sparse=True)
rec["sparse_open_s"] = round(time.perf_counter() - t0, 2)
info = sp.sparse_info()
rec.update(entries=int(info.entry_ct), sparse_rows=int(info.sparse_variant_ct), dense_rows=int(info.dense_variant_ct))
score, t_score, rec["score_times"] = timed(lambda: sp.glm_score_sparse(y, z))
linear, t_linear, rec["linear_times"] = timed(lambda: sp.glm_sparse(y, z))
_, t_null, rec["one_variant_times"] = timed(lambda: sp.glm_score_sparse(y, z, v_begin=sp.v_begin, v_end=sp.v_begin + 1))
again = sp.glm_score_sparse(y, z)
sp.close()

# the two calls count the same samples, and a repeated call returns the same bytes
assert score["obs_ct"].tolist() == linear["obs_ct"].tolist(), "obs_ct"
assert np.array_equal(score["a1_freq"], linear["a1_freq"], equal_nan=True), "a1_freq"
for key in ("beta", "se", "stat", "p"):
    assert score[key].tobytes() == again[key].tobytes(), key
errs = {}
for e in score["errcode"]:
    errs[str(e)] = errs.get(str(e), 0) + 1
rec.update(score_seconds_per_call=round(t_score, 6), linear_seconds_per_call=round(t_linear, 6),
           null_fit_seconds=round(t_null, 6), score_over_linear=round(t_score / t_linear, 3),
           score_entries_per_s=info.entry_ct / t_score, linear_entries_per_s=info.entry_ct / t_linear, errcodes=errs)
print(json.dumps(rec), flush=True)
