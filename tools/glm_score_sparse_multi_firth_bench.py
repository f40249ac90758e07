#!/usr/bin/env python3
"""Times pgh_glm_score_sparse_multi_firth (Dataset.glm_score_sparse_multi_firth) on the sparse-resident dataset of a
rare-variant file and, in the same run, pgh_glm_score_sparse_multi and pgh_glm_score_sparse_multi_spa over the same rows
and the one-phenotype route pgh_glm_score_sparse_firth, a call per phenotype; it has the shape of
tools/glm_score_sparse_multi_spa_bench.py (pgh_glm_score_sparse_multi_firth).

The file is tools/glm_sparse_bench.py's (written straight from carrier lists, shared when --dir is the same).  Shape:
500K samples x 1M variants at about 0.1 % carriers, 10 covariates, cutoff 2, P = 1, 8, 64 phenotypes with about
--cases cases (several values: a record per value and P) and 1 % missing values each, every phenotype its own
missing-value pattern.  Per P: seconds per call of the three many-phenotype entry points (median of --reps after one
warm-up call).  The single Firth calls are timed for --singles phenotypes, once each after a warm-up call, and scaled to
P.  From them:
  speedup             P single Firth calls over the one many-phenotype Firth call
  firth_adds_seconds  what the Firth step adds to the many-phenotype score call, beside
  spa_adds_seconds    what the saddlepoint step adds to it
Also the shares of the rows in states 0, 1 and 2, and whether a repeated call returned the same bytes.
--profile: one P = 64 call after a warm-up call of one variant and nothing else, for a kernel trace.
One JSON line per case fraction and P.

usage: python tools/glm_score_sparse_multi_firth_bench.py [--samples 500000] [--variants 1000000] [--rate 0.001]
                                                          [--cases 0.2 0.01] [--phenotypes 1,8,64] [--cutoff 2]
                                                          [--reps 3] [--singles 4] [--dir DIR]"""
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

K = 10
FIRTH_KEYS = ("beta_firth", "se_firth", "p_firth", "firth_state")

ap = argparse.ArgumentParser()
ap.add_argument("--samples", type=int, default=500_000)
ap.add_argument("--variants", type=int, default=1_000_000)
ap.add_argument("--rate", type=float, default=0.001)
ap.add_argument("--cases", type=float, nargs="+", default=[0.2, 0.01])
ap.add_argument("--cutoff", type=float, default=2.0)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--singles", type=int, default=4, help="single calls of the one-phenotype Firth route timed")
ap.add_argument("--phenotypes", default="1,8,64")
ap.add_argument("--profile", action="store_true")
ap.add_argument("--dir", default="/tmp/glm_sparse_bench")
args = ap.parse_args()

m, n = args.variants, args.samples
os.makedirs(args.dir, exist_ok=True)
prefix = os.path.join(args.dir, f"carriers_{m}x{n}")
if not os.path.exists(prefix + ".pgen"):
    write_carrier_pfile(prefix, m, n, carrier_rows(m, n, args.rate, 13))

counts = [64] if args.profile else [int(p) for p in args.phenotypes.split(",")]
p_max = max(counts)
sp = L.Dataset.open(prefix + ".pgen", sparse=True)
info = sp.sparse_info()


def inputs(cases):
    rng = np.random.default_rng(1)
    z = rng.standard_normal((K, n))
    eta = math.log(cases / (1 - cases)) + 0.2 * z.sum(axis=0)
    Y = (rng.random((p_max, n)) < 1 / (1 + np.exp(-eta))).astype(np.float64)
    Y[rng.random((p_max, n)) < 0.01] = np.nan
    return z, Y


if args.profile:
    z, Y_all = inputs(args.cases[0])
    sp.glm_score_sparse_multi_firth(Y_all, z, firth_cutoff=args.cutoff, v_begin=sp.v_begin, v_end=sp.v_begin + 1)
    sp.glm_score_sparse_multi_firth(Y_all, z, firth_cutoff=args.cutoff)
    sp.close()
    sys.exit(0)


def median_call(call):
    out = call()  # warm-up (scratch growth, code objects)
    times = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        out = call()
        times.append(time.perf_counter() - t0)
    return float(np.median(times)), [round(x, 6) for x in times], out


def each_single(call):
    call(0)  # warm-up
    t0 = time.perf_counter()
    for p in range(args.singles):
        call(p % p_max)
    return (time.perf_counter() - t0) / args.singles


for cases in args.cases:
    z, Y_all = inputs(cases)
    one_firth = each_single(lambda p: sp.glm_score_sparse_firth(Y_all[p], z, firth_cutoff=args.cutoff))
    for P in counts:
        Y = np.ascontiguousarray(Y_all[:P])
        t_score, score_times, score = median_call(lambda: sp.glm_score_sparse_multi(Y, z))
        t_spa, spa_times, _ = median_call(lambda: sp.glm_score_sparse_multi_spa(Y, z, spa_cutoff=args.cutoff))
        t_firth, firth_times, firth = median_call(lambda: sp.glm_score_sparse_multi_firth(Y, z, firth_cutoff=args.cutoff))
        again = sp.glm_score_sparse_multi_firth(Y, z, firth_cutoff=args.cutoff)
        # the rows are the score test's
        for key in ("beta", "se", "stat", "p"):
            assert score[key].tobytes() == firth[key].tobytes(), key
        same = all(firth[key].tobytes() == again[key].tobytes() for key in FIRTH_KEYS + ("beta", "se", "p", "stat"))
        rows = firth["firth_state"].size
        rec = {
            "phenotypes": P, "shape": f"{m}x{n}", "entries": int(info.entry_ct), "covariates": K, "cutoff": args.cutoff,
            "case_rate": round(float(np.nanmean(Y)), 4),
            "score_seconds_per_call": round(t_score, 6), "score_times": score_times,
            "spa_seconds_per_call": round(t_spa, 6), "spa_times": spa_times,
            "firth_seconds_per_call": round(t_firth, 6), "firth_times": firth_times,
            "single_firth_call_seconds": round(one_firth, 6), "singles_timed": args.singles,
            "single_firth_calls_seconds": round(one_firth * P, 6),
            "speedup": round(one_firth * P / t_firth, 2),
            "firth_adds_seconds": round(t_firth - t_score, 6),
            "spa_adds_seconds": round(t_spa - t_score, 6),
            "fitted_share": round(float(np.mean(firth["errcode"] == None)), 5),  # noqa: E711
            "state0_share": round(float((firth["firth_state"] == 0).sum()) / rows, 5),
            "applied_share": round(float((firth["firth_state"] == 1).sum()) / rows, 5),
            "failed_share": round(float((firth["firth_state"] == 2).sum()) / rows, 7),
            "same_bytes_again": bool(same),
        }
        print(json.dumps(rec), flush=True)
sp.close()
