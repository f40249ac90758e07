#!/usr/bin/env python3
"""Times pgh_glm_score_sparse_multi (Dataset.glm_score_sparse_multi) on the sparse-resident dataset of a rare-variant
file against the only other route for many binary phenotypes over carrier lists, one pgh_glm_score_sparse call per
phenotype, in the same process; modelled on tools/glm_score_sparse_bench.py and tools/glm_score_multi_bench.py.

The file is tools/glm_sparse_bench.py's (written straight from carrier lists, shared when --dir is the same).  Shape:
500K samples x 1M variants at about 0.1 % carriers, 10 covariates, P = 1, 8, 64 phenotypes with about 20 % cases and
1 % missing values each (every phenotype its own missing-value pattern).  Per P: seconds per call (median of --reps
after one warm-up call); the seconds of the same call over ONE variant, which is the null fits and their staging, and
its share of the whole call; the rest of the call against the algorithmic traffic of the walk, entries x (16 P + 8 kp
+ 4) bytes.  The single calls are timed for --singles phenotypes, once each after a warm-up call, and scaled to P.
--profile: one P = 64 call after a warm-up call of one variant and nothing else, for a kernel trace.
One JSON line per P.

usage: python tools/glm_score_sparse_multi_bench.py [--samples 500000] [--variants 1000000] [--rate 0.001]
                                                    [--phenotypes 1,8,64] [--reps 3] [--singles 8] [--dir DIR]"""
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

ap = argparse.ArgumentParser()
ap.add_argument("--samples", type=int, default=500_000)
ap.add_argument("--variants", type=int, default=1_000_000)
ap.add_argument("--rate", type=float, default=0.001)
ap.add_argument("--cases", type=float, default=0.2)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--singles", type=int, default=8, help="single pgh_glm_score_sparse calls timed (0: none)")
ap.add_argument("--phenotypes", default="1,8,64")
ap.add_argument("--profile", action="store_true")
ap.add_argument("--dir", default="/tmp/glm_sparse_bench")
args = ap.parse_args()

m, n = args.variants, args.samples
os.makedirs(args.dir, exist_ok=True)
prefix = os.path.join(args.dir, f"carriers_{m}x{n}")
if not os.path.exists(prefix + ".pgen"):
    write_carrier_pfile(prefix, m, n, carrier_rows(m, n, args.rate, 13))

rng = np.random.default_rng(1)
z = rng.standard_normal((K, n))
counts = [64] if args.profile else [int(p) for p in args.phenotypes.split(",")]
p_max = max(counts)
eta = math.log(args.cases / (1 - args.cases)) + 0.2 * z.sum(axis=0)
Y_all = (rng.random((p_max, n)) < 1 / (1 + np.exp(-eta))).astype(np.float64)
Y_all[rng.random((p_max, n)) < 0.01] = np.nan

sp = L.Dataset.open(prefix + ".pgen", sparse=True)
info = sp.sparse_info()

if args.profile:
    sp.glm_score_sparse_multi(Y_all, z, v_begin=sp.v_begin, v_end=sp.v_begin + 1)
    sp.glm_score_sparse_multi(Y_all, z)
    sp.close()
    sys.exit(0)

single_each = None
if args.singles:
    sp.glm_score_sparse(Y_all[0], z)  # warm-up
    t0 = time.perf_counter()
    for p in range(args.singles):
        sp.glm_score_sparse(Y_all[p % p_max], z)
    single_each = (time.perf_counter() - t0) / args.singles


def median_call(Y, **kw):
    out = sp.glm_score_sparse_multi(Y, z, **kw)  # warm-up (scratch growth, code objects)
    times = []
    for _ in range(args.reps):
        t0 = time.perf_counter()
        out = sp.glm_score_sparse_multi(Y, z, **kw)
        times.append(time.perf_counter() - t0)
    return float(np.median(times)), times, out


kp = next(w for w in (0, 1, 2, 4, 8, 12, 16, 20) if w >= K)
for P in counts:
    Y = np.ascontiguousarray(Y_all[:P])
    t, times, out = median_call(Y)
    t_null, _, _ = median_call(Y, v_begin=sp.v_begin, v_end=sp.v_begin + 1)
    codes, ct = np.unique(out["errcode"].astype(str), return_counts=True)
    blocks = (P + 63) // 64
    walk_bytes = float(info.entry_ct) * sum(16 * min(64, P - 64 * b) + 8 * kp + 4 for b in range(blocks))
    rec = {
        "phenotypes": P, "shape": f"{m}x{n}", "entries": int(info.entry_ct), "covariates": K,
        "case_rate": round(float(np.nanmean(Y)), 4),
        "seconds_per_call": round(t, 6), "times": [round(x, 6) for x in times],
        "null_fit_seconds": round(t_null, 6), "null_fit_share": round(t_null / t, 4),
        "single_calls_seconds": None if single_each is None else round(single_each * P, 6),
        "single_call_seconds": None if single_each is None else round(single_each, 6),
        "singles_timed": args.singles,
        "speedup": None if single_each is None else round(single_each * P / t, 2),
        "walk_bytes": walk_bytes, "walk_bytes_per_s_of_the_rest": walk_bytes / max(t - t_null, 1e-9),
        "errcodes": dict(zip(codes.tolist(), ct.tolist())),
    }
    print(json.dumps(rec), flush=True)
sp.close()
