#!/usr/bin/env python3
"""Times pgh_skat_sparse (Dataset.skat_sparse) on the sparse-resident dataset of a rare-variant file, and
pgh_burden_sparse (Dataset.burden_sparse) over the same sets in the same run as the figure to set it against
(pgh_skat_sparse).

The file is tools/glm_sparse_bench.py's: written straight from carrier lists, never through a dense matrix.  The sets
are --set-size consecutive variants each (default: as many sets as the file holds), weights U(0.25, 25); the phenotype
is 0 / 1 with about --case-rate cases for pgh_skat_sparse and quantitative for pgh_burden_sparse.
Per call: seconds (median of --reps after one warm-up call) and entries per second over the entries of the variants
the sets cover.  The host finish is timed apart, from outside: the same call with every weight 0.0 stages, fits the
null model, runs the kernel, copies its sums and builds Phi as the weighted call does, but its K is zero, so the
eigenvalue iteration ends at once and no p-value is taken; the difference of the two calls is the eigenvalues and the
p-values of the weighted one.  The rows of the timed calls are compared byte for byte.
One JSON line.

usage: python tools/skat_sparse_bench.py [--samples 500000] [--variants 1000000] [--rate 0.001] [--covar 10]
                                         [--set-size 50] [--sets N] [--case-rate 0.2] [--reps 3] [--dir DIR]"""
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
ap.add_argument("--set-size", type=int, default=50)
ap.add_argument("--sets", type=int, default=0)
ap.add_argument("--case-rate", type=float, default=0.2)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--dir", default="/tmp/glm_sparse_bench")
args = ap.parse_args()

m, n, k = args.variants, args.samples, args.covar
n_sets = args.sets or m // args.set_size
covered = n_sets * args.set_size
assert 1 <= n_sets and covered <= m and args.set_size <= L.SKAT_MAX_SET, (n_sets, args.set_size, m)
os.makedirs(args.dir, exist_ok=True)
prefix = os.path.join(args.dir, f"carriers_{m}x{n}")
t0 = time.perf_counter()
if not os.path.exists(prefix + ".pgen"):
    write_carrier_pfile(prefix, m, n, carrier_rows(m, n, args.rate, 13))
rec = {"shape": f"{m}x{n}", "carrier_rate_max": 2 * args.rate, "covariates": k, "sets": n_sets,
       "set_size": args.set_size, "file_bytes": os.path.getsize(prefix + ".pgen"),
       "write_s": round(time.perf_counter() - t0, 1)}

rng = np.random.default_rng(1)
z = rng.standard_normal((k, n)) if k else None
eta = z.sum(axis=0) * 0.2 if k else np.zeros(n)
y_lin = eta + rng.standard_normal(n)
y_bin = (rng.random(n) < 1.0 / (1.0 + np.exp(-(eta + np.log(args.case_rate / (1.0 - args.case_rate)))))).astype(np.float64)
gone = rng.random(n) < 0.01
y_lin[gone] = np.nan
y_bin[gone] = np.nan
set_off = np.arange(n_sets + 1, dtype=np.uint64) * np.uint64(args.set_size)
set_vidx = np.arange(covered, dtype=np.uint32)
weights = rng.uniform(0.25, 25.0, covered)


def timed(call):
    out = call()  # warm-up (scratch growth, code objects)
    times = []
    for _ in range(args.reps):
        t = time.perf_counter()
        again = call()
        times.append(time.perf_counter() - t)
        assert np.asarray(out).tobytes() == np.asarray(again).tobytes()
    return out, float(np.median(times)), [round(x, 6) for x in times]


t0 = time.perf_counter()
sp = L.Dataset.open(prefix + ".pgen", sparse=True)
rec["sparse_open_s"] = round(time.perf_counter() - t0, 2)
info = sp.sparse_info()
rec.update(entries=int(info.entry_ct), sparse_rows=int(info.sparse_variant_ct), dense_rows=int(info.dense_variant_ct),
           sparse_resident_bytes=int(info.resident_bytes), cases=int(np.nansum(y_bin)))
# the entries of the covered variants: per-variant counts of the calls off the base code (hom-ref in this file)
counts = sp.counts_range(0, covered).astype(np.int64)
covered_entries = int((counts.sum(axis=1) - counts.max(axis=1)).sum())
rows, t_skat, rec["skat_times"] = timed(lambda: sp.skat_sparse(y_bin, set_off, set_vidx, weights, z))
_, t_zero, rec["skat_zero_weight_times"] = timed(lambda: sp.skat_sparse(y_bin, set_off, set_vidx, np.zeros(covered), z))
_, t_burden, rec["burden_times"] = timed(lambda: sp.burden_sparse(y_lin, set_off, set_vidx, weights, z))
sp.close()

errs, states = {}, {}
for c in rows["errcode"]:
    errs[str(L.GLM_ERRCODES[c])] = errs.get(str(L.GLM_ERRCODES[c]), 0) + 1
for c in rows["p_state"]:
    states[int(c)] = states.get(int(c), 0) + 1
rec.update(covered_variants=covered, covered_entries=covered_entries,
           skat_seconds_per_call=round(t_skat, 6), skat_zero_weight_seconds_per_call=round(t_zero, 6),
           skat_eigen_and_p_seconds=round(t_skat - t_zero, 6), burden_seconds_per_call=round(t_burden, 6),
           skat_entries_per_s=covered_entries / t_skat, burden_entries_per_s=covered_entries / t_burden,
           skat_over_burden=round(t_skat / t_burden, 2), errcodes=errs, p_states=states,
           mean_n_carriers=float(rows["n_carriers"].mean()), mean_n_lambda=float(rows["n_lambda"].mean()))
print(json.dumps(rec), flush=True)
