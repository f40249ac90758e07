#!/usr/bin/env python3
"""Times pgh_glm_score_multi_dosage (Dataset.glm_score_multi_dosage) on pgh_synth_create data with synthetic dosage
tracks, modelled on tools/glm_score_multi_bench.py, against two references taken in the same run:
  (a) pgh_glm logistic (firth off) over the same dosage dataset, the only other route for a binary phenotype over
      dosages: --singles phenotypes over the first --slice variants, once each after a warm-up call, scaled to the
      whole range and to P;
  (b) pgh_glm_score_multi over the same synthetic calls without tracks: the hardcall ceiling.

Shape: 20K variants x 500K samples ("small": 2K x 50K, a quick check of the tool itself), 2 % missing calls, every
variant with a track whose samples carry an explicit dosage at --rates (1.0: an imputed panel, 0.1: sparse tracks), 10
covariates, P = 1, 8, 64 phenotypes with about 20 % cases and 1 % missing values each.  Per rate and P: seconds per call
(median of --reps after one warm-up call), the ratio to (a) and to (b).  One JSON line each.
--profile RATE: one P = 64 call at that rate and nothing else, for a kernel trace."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import plinking_duck_amd.lib as L  # noqa: E402

K = 10
SEED = 20261020

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--singles", type=int, default=4, help="single pgh_glm logistic calls timed, 8 at most (0: none)")
ap.add_argument("--slice", type=int, default=2000, help="variants of the single pgh_glm calls")
ap.add_argument("--phenotypes", default="1,8,64")
ap.add_argument("--rates", default="1.0,0.1")
ap.add_argument("--shape", default="large", choices=["large", "small"])
ap.add_argument("--profile", type=float, default=None, metavar="RATE")
args = ap.parse_args()

m, n = (20_000, 500_000) if args.shape == "large" else (2_000, 50_000)
rng = np.random.default_rng(1)
z = rng.standard_normal((K, n))
counts = [64] if args.profile is not None else [int(p) for p in args.phenotypes.split(",")]
p_max = max(counts)
eta = np.log(0.2 / 0.8) + 0.2 * z.sum(axis=0) / np.sqrt(K)
Y_all = (rng.random((p_max, n)) < 1 / (1 + np.exp(-eta))).astype(np.float64)
Y_all[rng.random((p_max, n)) < 0.01] = np.nan


def tracks(rate):
    ds = L.Dataset.synth(0, m, n, SEED, 0.02)
    ds.synth_add_dosage(rate, SEED + 1)
    assert ds.info.dosage_variant_ct == m
    return ds


if args.profile is not None:
    ds = tracks(args.profile)
    ds.glm_score_multi_dosage(Y_all, z)
    ds.close()
    sys.exit(0)


def median_call(call, Y):
    out = call(Y, z)  # warm-up (scratch growth, code objects)
    times = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        out = call(Y, z)
        times.append(time.perf_counter() - t0)
    return float(np.median(times)), times, out


# (b) the same calls without tracks
hard = L.Dataset.synth(0, m, n, SEED, 0.02)
hard_seconds = {P: median_call(hard.glm_score_multi, np.ascontiguousarray(Y_all[:P]))[0] for P in counts}
hard.close()

for rate in (float(r) for r in args.rates.split(",")):
    ds = tracks(rate)
    single_each = None
    singles = min(args.singles, 8)
    v_slice = min(args.slice, m)
    if singles:
        ds.glm(Y_all[0], z, model="logistic", firth=False, v_begin=0, v_end=v_slice)  # warm-up
        t0 = time.perf_counter()
        for p in range(singles):
            ds.glm(Y_all[p % p_max], z, model="logistic", firth=False, v_begin=0, v_end=v_slice)
        single_each = (time.perf_counter() - t0) / singles * (m / v_slice)
    for P in counts:
        t, times, out = median_call(ds.glm_score_multi_dosage, np.ascontiguousarray(Y_all[:P]))
        codes, ct = np.unique(out["errcode"].astype(str), return_counts=True)
        rec = {
            "dosage_rate": rate, "phenotypes": P, "shape": f"{m}x{n}", "covariates": K,
            "case_rate": round(float(np.nanmean(Y_all[:P])), 4),
            "seconds_per_call": round(t, 6), "times": [round(x, 6) for x in times],
            "single_glm_calls_seconds": None if single_each is None else round(single_each * P, 6),
            "singles_timed": singles, "singles_slice": v_slice,
            "speedup_over_single_glm_calls": None if single_each is None else round(single_each * P / t, 2),
            "hardcall_score_multi_seconds": round(hard_seconds[P], 6),
            "ratio_to_hardcall_score_multi": round(t / hard_seconds[P], 3),
            "errcodes": dict(zip(codes.tolist(), ct.tolist())),
        }
        print(json.dumps(rec), flush=True)
    ds.close()
