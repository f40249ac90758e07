#!/usr/bin/env python3
"""Times pgh_glm (Dataset.glm) on pgh_synth_create data.

Shapes: SURVEY's 30K variants x 10K samples (linear and logistic, no covariates) and 100K x 500K (linear with 10
covariates, logistic with 2).  The reference's own planning figures for 30K x 10K -- 1.8 s for its plink_glm, 61 ms
for plink2 -- are quoted for comparison only; neither was measured here.

Per shape: seconds per call (median of --reps after one warm-up call), genotypes (variants x samples) per second,
and the fraction of the FP64 vector peak (78.6 TFLOP/s, AMD's published MI355X figure) under a stated FLOP model:
  linear    2 (k + 4) FLOP per genotype (the per-variant sums; the Gram, corrections and solves are not counted)
  logistic  2 (p (p + 1) / 2 + 2 p) FLOP per genotype and Newton pass, p = k + 2, reported per pass
            (the fit count and passes per fit depend on the data; the figure is per pass over every variant).
One JSON line per shape."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import plinking_duck_amd.lib as L  # noqa: E402

FP64_PEAK = 78.6e12

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--shapes", default="survey,large", help="comma list of: survey, large")
args = ap.parse_args()

SHAPES = {
    "survey": [(30_000, 10_000, "linear", 0), (30_000, 10_000, "logistic", 0)],
    "large": [(100_000, 500_000, "linear", 10), (100_000, 500_000, "logistic", 2)],
}

for name in args.shapes.split(","):
    for m, n, model, k in SHAPES[name]:
        ds = L.Dataset.synth(0, m, n, 20261016, 0.02)
        rng = np.random.default_rng(1)
        z = rng.standard_normal((k, n)) if k else None
        eta = (z.sum(axis=0) * 0.2 if k else 0.0) + rng.standard_normal(n)
        y = eta if model == "linear" else (rng.random(n) < 1 / (1 + np.exp(-eta))).astype(np.float64)
        y[rng.random(n) < 0.01] = np.nan
        out = ds.glm(y, z, model=model)  # warm-up (scratch growth, code objects)
        times = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            out = ds.glm(y, z, model=model)
            times.append(time.perf_counter() - t0)
        t = float(np.median(times))
        p = k + 2
        flop = 2 * (k + 4) if model == "linear" else 2 * (p * (p + 1) // 2 + 2 * p)
        errs = {}
        for e in out["errcode"]:
            errs[str(e)] = errs.get(str(e), 0) + 1
        rec = {
            "shape": f"{m}x{n}", "model": model, "covariates": k, "seconds_per_call": round(t, 6),
            "times": [round(x, 6) for x in times], "genotypes_per_s": m * n / t,
            ("fp64_peak_fraction" if model == "linear" else "fp64_peak_fraction_per_pass"): m * n * flop / t / FP64_PEAK,
            "firth_rows": int(out["firth"].sum()), "errcodes": errs,
        }
        print(json.dumps(rec), flush=True)
        ds.close()
