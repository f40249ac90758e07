#!/usr/bin/env python3
"""Times pgh_glm_score_sparse_spa (Dataset.glm_score_sparse_spa) on the sparse-resident dataset of a rare-variant file
and, in the same run, pgh_glm_score_sparse over the same rows: the difference is what the saddlepoint p-values cost
(pgh_glm_score_sparse_spa).  Also the share of rows in states 1 and 2.

The file is tools/glm_sparse_bench.py's: written straight from carrier lists (tools/sparse_bench.py), never through a
dense matrix, and shared with it when --dir is the same.  The phenotype is Bernoulli with about --cases cases (several
values: one record each) and depends on the covariates.  Per call: seconds (median of --reps after one warm-up call).
One JSON line per case fraction.

usage: python tools/glm_score_sparse_spa_bench.py [--samples 500000] [--variants 1000000] [--rate 0.001] [--covar 10]
                                                  [--cases 0.2 0.01] [--cutoff 2] [--reps 3] [--dir DIR]"""
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
ap.add_argument("--cases", type=float, nargs="+", default=[0.2, 0.01])
ap.add_argument("--cutoff", type=float, default=2.0)
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
rec.update(entries=int(info.entry_ct), sparse_rows=int(info.sparse_variant_ct), dense_rows=int(info.dense_variant_ct),
           cutoff=args.cutoff)
for cases in args.cases:
    rng = np.random.default_rng(1)
    z = rng.standard_normal((k, n)) if k else None
    eta = math.log(cases / (1 - cases)) + (z.sum(axis=0) * 0.2 if k else 0.0)
    y = (rng.random(n) < 1 / (1 + np.exp(-eta))).astype(np.float64)
    y[rng.random(n) < 0.01] = np.nan
    out = dict(rec, case_fraction=round(float(np.nanmean(y)), 4))
    score, t_score, out["score_times"] = timed(lambda: sp.glm_score_sparse(y, z))
    spa, t_spa, out["spa_times"] = timed(lambda: sp.glm_score_sparse_spa(y, z, cutoff=args.cutoff))
    again = sp.glm_score_sparse_spa(y, z, cutoff=args.cutoff)
    # the rows are the score test's, and a repeated call returns the same bytes
    for key in ("beta", "se", "stat", "p"):
        assert score[key].tobytes() == spa[key].tobytes(), key
    for key in ("p_spa", "spa_state"):
        assert spa[key].tobytes() == again[key].tobytes(), key
    fitted = int((spa["errcode"] == None).sum())  # noqa: E711
    applied, failed = int((spa["spa_state"] == 1).sum()), int((spa["spa_state"] == 2).sum())
    ratio = spa["p_spa"][spa["spa_state"] == 1] / spa["p"][spa["spa_state"] == 1]
    out.update(score_seconds_per_call=round(t_score, 6), spa_seconds_per_call=round(t_spa, 6),
               spa_over_score=round(t_spa / t_score, 3), fitted_rows=fitted, applied_rows=applied, failed_rows=failed,
               applied_share=round(applied / max(1, len(spa["p"])), 5),
               failed_share=round(failed / max(1, len(spa["p"])), 5),
               extra_us_per_attempted_row=round(1e6 * (t_spa - t_score) / max(1, applied + failed), 3),
               applied_beyond_2x=int(((ratio < 0.5) | (ratio > 2.0)).sum()))
    print(json.dumps(out), flush=True)
sp.close()
