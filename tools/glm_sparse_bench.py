#!/usr/bin/env python3
"""Times pgh_glm_sparse (Dataset.glm_sparse) on the sparse-resident dataset of a rare-variant file against pgh_glm's
linear fit (Dataset.glm) on the dense dataset of the same file, in one run (pgh_glm_sparse).

The file is written straight from carrier lists (tools/sparse_bench.py: type-4 records against hom-ref, carriers
~ Binomial(samples, U(0, 2 rate)) per variant, mostly het, some hom-alt and missing), never through a dense matrix.
Per call: seconds (median of --reps after one warm-up call); for the sparse call also entries per second.  The rows
of the two calls are compared (errcode, obs_ct and a1_freq equal, estimates within 1e-9).
One JSON line.

usage: python tools/glm_sparse_bench.py [--samples 500000] [--variants 1000000] [--rate 0.001] [--covar 10]
                                        [--reps 3] [--dir DIR]"""
import argparse
import json
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

rng = np.random.default_rng(1)
z = rng.standard_normal((k, n)) if k else None
y = (z.sum(axis=0) * 0.2 if k else 0.0) + rng.standard_normal(n)
y[rng.random(n) < 0.01] = np.nan


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
           sparse_resident_bytes=int(info.resident_bytes), dense_bytes=int(info.dense_bytes))
got, t_sparse, rec["sparse_times"] = timed(lambda: sp.glm_sparse(y, z))
sp.close()
L.trim_device_cache()

t0 = time.perf_counter()
ds = L.Dataset.open(prefix + ".pgen")
rec["dense_open_s"] = round(time.perf_counter() - t0, 2)
want, t_dense, rec["dense_times"] = timed(lambda: ds.glm(y, z, model="linear"))
ds.close()

for key in ("obs_ct", "errcode"):
    assert list(got[key]) == list(want[key]), key
assert np.array_equal(got["a1_freq"], want["a1_freq"], equal_nan=True), "a1_freq"
se = np.nan_to_num(want["se"], nan=0.0)
worst = 0.0
for key in ("beta", "se", "stat", "p"):
    g, e = got[key], want[key]
    assert np.array_equal(np.isnan(g), np.isnan(e)), key
    scale = np.abs(e) + (se if key == "beta" else 1.0 if key == "stat" else 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        rel = np.where(np.isnan(e) | (g == e), 0.0, np.abs(g - e) / scale)
    worst = max(worst, float(rel.max(initial=0.0)))
errs = {}
for e in got["errcode"]:
    errs[str(e)] = errs.get(str(e), 0) + 1
rec.update(sparse_seconds_per_call=round(t_sparse, 6), dense_seconds_per_call=round(t_dense, 6),
           dense_over_sparse=round(t_dense / t_sparse, 2), entries_per_s=info.entry_ct / t_sparse,
           dense_genotypes_per_s=m * n / t_dense, worst_relative_difference=worst, errcodes=errs)
print(json.dumps(rec), flush=True)
assert worst <= 1e-9, worst
