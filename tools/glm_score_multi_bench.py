#!/usr/bin/env python3
"""Times pgh_glm_score_multi (Dataset.glm_score_multi) against the only other dense route for binary phenotypes, one
pgh_glm logistic call (firth off) per phenotype, on pgh_synth_create data, modelled on tools/glm_multi_bench.py.

Shape: 100K variants x 500K samples ("small": 20K x 50K, a quick check of the tool itself), 2 % missing calls, 10
covariates, P = 1, 8, 64 phenotypes with about 20 % cases and 1 % missing values each (every phenotype its own
missing-value pattern).  Per P: seconds per call (median of --reps after one warm-up call); the seconds of the same
call over ONE variant, which is the null fits and their staging, and its share of the whole call; the FLOP of the
contraction, 2 V n_raw P (k + 3), over the whole call's time against the FP64 matrix peak (78.6 TFLOP/s, AMD's
published MI355X figure) -- a lower bound of the kernel's own rate, which a kernel trace of --profile gives.
The single calls are timed for --singles phenotypes, once each after a warm-up call, and scaled to P.
--profile: one P = 64 call and nothing else, for a kernel trace.  One JSON line per P."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import plinking_duck_amd.lib as L  # noqa: E402

FP64_MATRIX_PEAK = 78.6e12
K = 10

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--singles", type=int, default=8, help="single pgh_glm logistic calls timed (0: none)")
ap.add_argument("--phenotypes", default="1,8,64")
ap.add_argument("--shape", default="large", choices=["large", "small"])
ap.add_argument("--profile", action="store_true")
args = ap.parse_args()

m, n = (100_000, 500_000) if args.shape == "large" else (20_000, 50_000)
ds = L.Dataset.synth(0, m, n, 20261019, 0.02)
rng = np.random.default_rng(1)
z = rng.standard_normal((K, n))
counts = [64] if args.profile else [int(p) for p in args.phenotypes.split(",")]
p_max = max(counts)
eta = np.log(0.2 / 0.8) + 0.2 * z.sum(axis=0) / np.sqrt(K)
Y_all = (rng.random((p_max, n)) < 1 / (1 + np.exp(-eta))).astype(np.float64)
Y_all[rng.random((p_max, n)) < 0.01] = np.nan

if args.profile:
    ds.glm_score_multi(Y_all, z)
    ds.close()
    sys.exit(0)

single_each = None
if args.singles:
    ds.glm(Y_all[0], z, model="logistic", firth=False)  # warm-up
    t0 = time.perf_counter()
    for p in range(args.singles):
        ds.glm(Y_all[p % p_max], z, model="logistic", firth=False)
    single_each = (time.perf_counter() - t0) / args.singles


def median_call(Y, **kw):
    out = ds.glm_score_multi(Y, z, **kw)  # warm-up (scratch growth, code objects)
    times = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        out = ds.glm_score_multi(Y, z, **kw)
        times.append(time.perf_counter() - t0)
    return float(np.median(times)), times, out


for P in counts:
    Y = np.ascontiguousarray(Y_all[:P])
    t, times, out = median_call(Y)
    t_null, _, _ = median_call(Y, v_begin=0, v_end=1)
    codes, ct = np.unique(out["errcode"].astype(str), return_counts=True)
    rec = {
        "phenotypes": P, "shape": f"{m}x{n}", "covariates": K, "case_rate": round(float(np.nanmean(Y)), 4),
        "seconds_per_call": round(t, 6), "times": [round(x, 6) for x in times],
        "null_fit_seconds": round(t_null, 6), "null_fit_share": round(t_null / t, 4),
        "single_calls_seconds": None if single_each is None else round(single_each * P, 6),
        "singles_timed": args.singles,
        "speedup": None if single_each is None else round(single_each * P / t, 2),
        "contraction_flop": 2.0 * m * n * P * (K + 3),
        "fp64_matrix_peak_fraction_of_call": 2.0 * m * n * P * (K + 3) / t / FP64_MATRIX_PEAK,
        "errcodes": dict(zip(codes.tolist(), ct.tolist())),
    }
    print(json.dumps(rec), flush=True)
ds.close()
