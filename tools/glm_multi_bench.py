#!/usr/bin/env python3
"""Times pgh_glm_multi (Dataset.glm_multi) against the same phenotypes through one pgh_glm (Dataset.glm) call each,
on pgh_synth_create data (2 % missing calls), modelled on tools/glm_bench.py.

Cases at 100K variants x 500K samples ("small": 20K x 50K, a quick check of the tool itself):
  linear    10 covariates, P = 1, 8, 64, 256 phenotypes sharing one missing-value pattern (1 % missing),
            and P = 64 spread over 4 patterns (16 phenotypes each)
  logistic  2 covariates, P = 1, 8, one pattern
Per case: seconds per multi call (median of --reps after one warm-up call) and seconds for the P single calls.  The
single calls are timed for min(P, --singles) phenotypes, once each after a warm-up call, and scaled to P
("singles_timed" says how many ran).  FLOP model of the linear multi call: 2 P FLOP per genotype for the sum x y_p
GEMM (the shared sums, corrections and solves are not counted), against the FP64 vector peak (78.6 TFLOP/s, AMD's
published MI355X figure).  One JSON line per case."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import plinking_duck_amd.lib as L  # noqa: E402

FP64_PEAK = 78.6e12
CASES = {
    "linear1": ("linear", 10, 1, 1), "linear8": ("linear", 10, 8, 1), "linear64": ("linear", 10, 64, 1),
    "linear256": ("linear", 10, 256, 1), "linear64x4": ("linear", 10, 64, 4),
    "logistic1": ("logistic", 2, 1, 1), "logistic8": ("logistic", 2, 8, 1),
}

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--singles", type=int, default=8, help="single calls timed per case (0: none)")
ap.add_argument("--cases", default=",".join(CASES), help="comma list of: " + ", ".join(CASES))
ap.add_argument("--shape", default="large", choices=["large", "small"])
args = ap.parse_args()

m, n = (100_000, 500_000) if args.shape == "large" else (20_000, 50_000)
ds = L.Dataset.synth(0, m, n, 20261016, 0.02)
rng = np.random.default_rng(1)
Z = {k: rng.standard_normal((k, n)) for k in (2, 10)}
masks = [rng.random(n) < 0.01 for _ in range(4)]

for name in args.cases.split(","):
    model, k, P, n_pat = CASES[name]
    z = Z[k]
    eta = z.sum(axis=0) * 0.2 + rng.standard_normal((P, n))
    Y = eta if model == "linear" else (rng.random((P, n)) < 1 / (1 + np.exp(-eta))).astype(np.float64)
    for p in range(P):
        Y[p, masks[p % n_pat]] = np.nan
    out = ds.glm_multi(Y, z, model=model)  # warm-up (scratch growth, code objects)
    times = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        out = ds.glm_multi(Y, z, model=model)
        times.append(time.perf_counter() - t0)
    t = float(np.median(times))
    n_single = min(P, args.singles)
    single_s = None
    if n_single:
        ds.glm(Y[0], z, model=model)  # warm-up
        t0 = time.perf_counter()
        for p in range(n_single):
            ds.glm(Y[p], z, model=model)
        single_s = (time.perf_counter() - t0) * P / n_single
    errs = {}
    for e in out["errcode"].ravel():
        errs[str(e)] = errs.get(str(e), 0) + 1
    rec = {
        "case": name, "shape": f"{m}x{n}", "model": model, "covariates": k, "phenotypes": P, "patterns": n_pat,
        "seconds_per_call": round(t, 6), "times": [round(x, 6) for x in times],
        "single_calls_seconds": None if single_s is None else round(single_s, 6), "singles_timed": n_single,
        "speedup": None if single_s is None else round(single_s / t, 2),
        "firth_rows": int(out["firth"].sum()), "errcodes": errs,
    }
    if model == "linear":
        rec["gemm_fp64_peak_fraction"] = m * n * 2 * P / t / FP64_PEAK
    print(json.dumps(rec), flush=True)
ds.close()
