#!/usr/bin/env python3
"""Times pgh_glm_score_multi_firth (Dataset.glm_score_multi_firth, cutoff 2) beside pgh_glm_score_multi and
pgh_glm_score_multi_spa in the same run, on pgh_synth_create data in the shape of tools/glm_score_multi_spa_bench.py.

Shape: 100K variants x 500K samples ("small": 20K x 50K, a quick check of the tool itself), 2 % missing calls, 10
covariates, P = 1, 8, 64 phenotypes with about 1 % cases and 1 % missing values each (every phenotype its own
missing-value pattern).  Per P, after one warm-up call of each: --reps calls of each, the three alternating, a host
clock around calls that end in a device synchronise; the medians, what the saddlepoint and the Firth step each add to
the plain call and the ratio of the two additions; the share of the rows where Firth was applied (state 1) and where it
failed (state 2); and whether `out` is the plain call's bit for bit.  One JSON line per P.
--profile: one P = 64 call of pgh_glm_score_multi_firth and nothing else, for a kernel trace.

One process per P, each under a time limit of its own, a step starting only when the one before it ended well:
  timeout -k 10 300 python tools/glm_score_multi_firth_bench.py --phenotypes 1 &&
  timeout -k 10 300 python tools/glm_score_multi_firth_bench.py --phenotypes 8 &&
  timeout -k 10 600 python tools/glm_score_multi_firth_bench.py --phenotypes 64"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import plinking_duck_amd.lib as L  # noqa: E402

K = 10
CUTOFF = 2.0
CASE_RATE = 0.01

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--phenotypes", default="1,8,64")
ap.add_argument("--shape", default="large", choices=["large", "small"])
ap.add_argument("--profile", action="store_true")
args = ap.parse_args()

m, n = (100_000, 500_000) if args.shape == "large" else (20_000, 50_000)
ds = L.Dataset.synth(0, m, n, 20261019, 0.02)
rng = np.random.default_rng(1)
z = rng.standard_normal((K, n))
counts = [64] if args.profile else [int(p) for p in args.phenotypes.split(",")]
# the phenotypes of tools/glm_score_multi_spa_bench.py at P = 64, whatever P this process times
p_max = max(64, max(counts))
eta = np.log(CASE_RATE / (1 - CASE_RATE)) + 0.2 * z.sum(axis=0) / np.sqrt(K)
Y_all = (rng.random((p_max, n)) < 1 / (1 + np.exp(-eta))).astype(np.float64)
Y_all[rng.random((p_max, n)) < 0.01] = np.nan

if args.profile:
    ds.glm_score_multi_firth(Y_all, z, firth_cutoff=CUTOFF)
    ds.close()
    sys.exit(0)

for P in counts:
    Y = np.ascontiguousarray(Y_all[:P])
    plain = ds.glm_score_multi(Y, z)  # warm-up (scratch growth, code objects)
    spa = ds.glm_score_multi_spa(Y, z, spa_cutoff=CUTOFF)
    firth = ds.glm_score_multi_firth(Y, z, firth_cutoff=CUTOFF)
    t_plain, t_spa, t_firth = [], [], []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        plain = ds.glm_score_multi(Y, z)
        t_plain.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        spa = ds.glm_score_multi_spa(Y, z, spa_cutoff=CUTOFF)
        t_spa.append(time.perf_counter() - t0)
        t0 = time.perf_counter()
        firth = ds.glm_score_multi_firth(Y, z, firth_cutoff=CUTOFF)
        t_firth.append(time.perf_counter() - t0)
    a, b, c = float(np.median(t_plain)), float(np.median(t_spa)), float(np.median(t_firth))
    same = all(np.array_equal(plain[key], firth[key], equal_nan=True) for key in ("beta", "se", "stat", "p", "a1_freq")) \
        and all(np.array_equal(plain[key], firth[key]) for key in ("obs_ct", "errcode", "firth"))
    on = firth["firth_state"] == 1
    codes, ct = np.unique(firth["errcode"].astype(str), return_counts=True)
    rec = {
        "phenotypes": P, "shape": f"{m}x{n}", "covariates": K, "case_rate": round(float(np.nanmean(Y)), 4),
        "cutoff": CUTOFF,
        "score_multi_seconds": round(a, 6), "score_multi_times": [round(x, 6) for x in t_plain],
        "score_multi_spa_seconds": round(b, 6), "score_multi_spa_times": [round(x, 6) for x in t_spa],
        "score_multi_firth_seconds": round(c, 6), "score_multi_firth_times": [round(x, 6) for x in t_firth],
        "spa_extra_seconds": round(b - a, 6), "firth_extra_seconds": round(c - a, 6),
        "firth_extra_over_spa_extra": round((c - a) / (b - a), 4),
        "firth_extra_over_score_multi": round((c - a) / a, 4),
        "rows": int(on.size), "fitted_rows": int((firth["errcode"] == None).sum()),  # noqa: E711
        "applied_share": round(float(on.mean()), 6),
        "failed_share": round(float((firth["firth_state"] == 2).mean()), 6),
        "other_sign_share_of_applied": round(float((firth["beta_firth"][on] * firth["beta"][on] < 0).mean()), 6)
        if on.any() else None,
        "out_equals_score_multi": bool(same),
        "errcodes": dict(zip(codes.tolist(), ct.tolist())),
    }
    print(json.dumps(rec), flush=True)
ds.close()
