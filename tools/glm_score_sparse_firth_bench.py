#!/usr/bin/env python3
"""Times pgh_glm_score_sparse_firth (Dataset.glm_score_sparse_firth) on the sparse-resident dataset of a rare-variant
file beside pgh_glm_score_sparse and pgh_glm_score_sparse_spa over the same rows in the same run: what the Firth step
adds to the score test, next to what the saddlepoint step adds (pgh_glm_score_sparse_firth).
Also the shares of rows in states 1 and 2 and whether a repeated call returns the same bytes.

The file is tools/glm_sparse_bench.py's: written straight from carrier lists (tools/sparse_bench.py), never through a
dense matrix, and shared with it when --dir is the same.  The phenotype is tools/glm_score_sparse_spa_bench.py's:
Bernoulli with about --cases cases and dependent on the covariates.  Per case fraction, after one warm-up call of each:
--reps calls of each, the three alternating, a host clock around calls that end in a device synchronise; the medians.
One JSON line per case fraction.
--write-only: write the carrier file (no device work) and stop.
--profile: one call of pgh_glm_score_sparse_firth at the first case fraction and nothing else, for a kernel trace.

One process per case fraction, each under a time limit of its own, a step starting only when the one before it ended
well (16 CPUs at the most: the tool starts no threads of its own):
  timeout -k 10 600 python tools/glm_score_sparse_firth_bench.py --write-only &&
  timeout -k 10 300 python tools/glm_score_sparse_firth_bench.py --cases 0.2 &&
  timeout -k 10 300 python tools/glm_score_sparse_firth_bench.py --cases 0.01

usage: python tools/glm_score_sparse_firth_bench.py [--samples 500000] [--variants 1000000] [--rate 0.001] [--covar 10]
                                                    [--cases 0.2 0.01] [--cutoff 2] [--reps 3] [--dir DIR]
                                                    [--write-only | --profile]"""
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
ap.add_argument("--write-only", action="store_true")
ap.add_argument("--profile", action="store_true")
args = ap.parse_args()

m, n, k = args.variants, args.samples, args.covar
os.makedirs(args.dir, exist_ok=True)
prefix = os.path.join(args.dir, f"carriers_{m}x{n}")
t0 = time.perf_counter()
if not os.path.exists(prefix + ".pgen"):
    write_carrier_pfile(prefix, m, n, carrier_rows(m, n, args.rate, 13))
rec = {"shape": f"{m}x{n}", "carrier_rate_max": 2 * args.rate, "covariates": k,
       "file_bytes": os.path.getsize(prefix + ".pgen"), "write_s": round(time.perf_counter() - t0, 1)}
if args.write_only:
    print(json.dumps(rec), flush=True)
    sys.exit(0)


def inputs(cases):
    rng = np.random.default_rng(1)
    z = rng.standard_normal((k, n)) if k else None
    eta = math.log(cases / (1 - cases)) + (z.sum(axis=0) * 0.2 if k else 0.0)
    y = (rng.random(n) < 1 / (1 + np.exp(-eta))).astype(np.float64)
    y[rng.random(n) < 0.01] = np.nan
    return y, z


t0 = time.perf_counter()
sp = L.Dataset.open(prefix + ".pgen", sparse=True)
rec["sparse_open_s"] = round(time.perf_counter() - t0, 2)
if args.profile:
    y, z = inputs(args.cases[0])
    sp.glm_score_sparse_firth(y, z, firth_cutoff=args.cutoff)
    sp.close()
    sys.exit(0)

info = sp.sparse_info()
rec.update(entries=int(info.entry_ct), sparse_rows=int(info.sparse_variant_ct), dense_rows=int(info.dense_variant_ct),
           cutoff=args.cutoff)
for cases in args.cases:
    y, z = inputs(cases)
    out = dict(rec, case_fraction=round(float(np.nanmean(y)), 4))
    calls = (lambda: sp.glm_score_sparse(y, z), lambda: sp.glm_score_sparse_spa(y, z, cutoff=args.cutoff),
             lambda: sp.glm_score_sparse_firth(y, z, firth_cutoff=args.cutoff))
    results = [call() for call in calls]  # warm-up (scratch growth, code objects)
    times = [[], [], []]
    for _ in range(args.reps):
        for j, call in enumerate(calls):
            t = time.perf_counter()
            results[j] = call()
            times[j].append(time.perf_counter() - t)
    score, spa, firth = results
    again = calls[2]()
    # the rows are the score test's, and a repeated call returns the same bytes
    for key in ("beta", "se", "stat", "p"):
        assert score[key].tobytes() == firth[key].tobytes() == spa[key].tobytes(), key
    same = all(firth[key].tobytes() == again[key].tobytes()
               for key in ("beta_firth", "se_firth", "p_firth", "firth_state", "beta", "se", "stat", "p"))
    a, b, c = (float(np.median(t)) for t in times)
    on = firth["firth_state"] == 1
    failed = int((firth["firth_state"] == 2).sum())
    out.update(score_times=[round(x, 6) for x in times[0]], spa_times=[round(x, 6) for x in times[1]],
               firth_times=[round(x, 6) for x in times[2]],
               score_seconds_per_call=round(a, 6), spa_seconds_per_call=round(b, 6), firth_seconds_per_call=round(c, 6),
               spa_extra_seconds=round(b - a, 6), firth_extra_seconds=round(c - a, 6),
               firth_extra_over_spa_extra=round((c - a) / (b - a), 4) if b != a else None,
               firth_over_score=round(c / a, 3),
               fitted_rows=int((firth["errcode"] == None).sum()),  # noqa: E711
               applied_rows=int(on.sum()), failed_rows=failed,
               applied_share=round(float(on.mean()), 5), failed_share=round(failed / max(1, on.size), 5),
               spa_applied_rows=int((spa["spa_state"] == 1).sum()), spa_failed_rows=int((spa["spa_state"] == 2).sum()),
               extra_us_per_attempted_row=round(1e6 * (c - a) / max(1, int(on.sum()) + failed), 3),
               other_sign_share_of_applied=round(float((firth["beta_firth"][on] * firth["beta"][on] < 0).mean()), 6)
               if on.any() else None,
               repeat_is_bit_identical=bool(same))
    print(json.dumps(out), flush=True)
sp.close()
