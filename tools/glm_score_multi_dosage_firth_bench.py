#!/usr/bin/env python3
"""Times pgh_glm_score_multi_dosage_firth (Dataset.glm_score_multi_dosage_firth, cutoff 2) beside
pgh_glm_score_multi_dosage and pgh_glm_score_multi_dosage_spa in the same run, on pgh_synth_create data with synthetic
dosage tracks, modelled on tools/glm_score_multi_dosage_spa_bench.py (the data, the phenotypes and what is timed).

Shape: 20K variants x 500K samples ("small": 2K x 50K, a quick check of the tool itself), 2 % missing calls, every
variant with a track whose samples carry an explicit dosage at --rates (1.0: an imputed panel, where E is all of N and
every evaluation passes over every sample of an applied row; 0.1: sparse tracks), 10 covariates, P = 1, 8, 64 phenotypes
with about 1 % cases and 1 % missing values each.  Per rate and P, after one warm-up call of each: --reps calls of each,
the three in turn, a host clock around calls that end in a device synchronise; the medians, what the Firth step adds to
the plain call and its ratio to it; the share of the rows where Firth was applied (state 1) and where it failed (state
2); and whether `out` is the plain call's bit for bit.  One JSON line each.
--profile RATE: one P = 64 call of pgh_glm_score_multi_dosage_firth at that rate and nothing else, for a kernel trace."""
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
SEED = 20261021

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=3)
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
eta = np.log(CASE_RATE / (1 - CASE_RATE)) + 0.2 * z.sum(axis=0) / np.sqrt(K)
Y_all = (rng.random((p_max, n)) < 1 / (1 + np.exp(-eta))).astype(np.float64)
Y_all[rng.random((p_max, n)) < 0.01] = np.nan


def tracks(rate):
    ds = L.Dataset.synth(0, m, n, SEED, 0.02)
    ds.synth_add_dosage(rate, SEED + 1)
    assert ds.info.dosage_variant_ct == m
    return ds


if args.profile is not None:
    ds = tracks(args.profile)
    ds.glm_score_multi_dosage_firth(Y_all, z, firth_cutoff=CUTOFF)
    ds.close()
    sys.exit(0)

for rate in (float(r) for r in args.rates.split(",")):
    ds = tracks(rate)
    for P in counts:
        Y = np.ascontiguousarray(Y_all[:P])
        calls = (("score_multi_dosage", lambda: ds.glm_score_multi_dosage(Y, z)),
                 ("score_multi_dosage_spa", lambda: ds.glm_score_multi_dosage_spa(Y, z, spa_cutoff=CUTOFF)),
                 ("score_multi_dosage_firth", lambda: ds.glm_score_multi_dosage_firth(Y, z, firth_cutoff=CUTOFF)))
        got = {name: call() for name, call in calls}  # warm-up (scratch growth, code objects)
        times = {name: [] for name, _ in calls}
        for _ in range(args.reps):
            for name, call in calls:
                t0 = time.perf_counter()
                got[name] = call()
                times[name].append(time.perf_counter() - t0)
        med = {name: float(np.median(t)) for name, t in times.items()}
        plain, firth = got["score_multi_dosage"], got["score_multi_dosage_firth"]
        same = all(np.array_equal(plain[key], firth[key], equal_nan=True) for key in ("beta", "se", "stat", "p", "a1_freq")) \
            and all(np.array_equal(plain[key], firth[key]) for key in ("obs_ct", "errcode", "firth"))
        codes, ct = np.unique(firth["errcode"].astype(str), return_counts=True)
        a, b = med["score_multi_dosage"], med["score_multi_dosage_firth"]
        rec = {
            "dosage_rate": rate, "phenotypes": P, "shape": f"{m}x{n}", "covariates": K,
            "case_rate": round(float(np.nanmean(Y)), 4), "cutoff": CUTOFF,
        }
        for name, _ in calls:
            rec[name + "_seconds"] = round(med[name], 6)
            rec[name + "_times"] = [round(x, 6) for x in times[name]]
        rec.update({
            "firth_extra_seconds": round(b - a, 6), "firth_extra_over_score_multi_dosage": round((b - a) / a, 4),
            "rows": int(firth["firth_state"].size), "fitted_rows": int((firth["errcode"] == None).sum()),  # noqa: E711
            "applied_share": round(float((firth["firth_state"] == 1).mean()), 6),
            "failed_share": round(float((firth["firth_state"] == 2).mean()), 6),
            "out_equals_score_multi_dosage": bool(same),
            "errcodes": dict(zip(codes.tolist(), ct.tolist())),
        })
        print(json.dumps(rec), flush=True)
    ds.close()
